/* eqf_batch_ensemble_follow.h — particle ensembles against batch slots (eqf_batch_ensemble.h) on the MI355X (gfx950): clouds that FOLLOW THEIR SLOT'S LANDMARK
 * TURNOVER. A vision step that drops a track and starts another one, or eqf_batch_augment, changes the slot's landmark ids; eqf_bens_nees, _errors and
 * _covariance then refuse the slot's cloud ("a filter id the cloud does not hold"). After eqf_bens_follow every listed cloud is again a cloud over its slot's
 * current landmarks, made on the device: NOTHING P-SIZED CROSSES THE BUS.
 *
 * Per entry, with F the slot's ids in state order (N of them), G the cloud's ids (in any order), K = F and G the kept ids, D = G \ F the dropped ones and
 * A = F \ G the added ones, after an accepted entry:
 *  - the cloud's id list is F, in the slot's order; P is what it was; THE 23 SENSOR PLANES ARE UNTOUCHED bit for bit;
 *  - the three point planes of every kept landmark hold, at its new place, THE BYTES THEY HELD at its old one; the dropped landmarks are gone;
 *  - every added landmark is drawn from the slot's belief CONDITIONAL ON WHAT THE PARTICLE ALREADY IS. With n = 21 + 3 N, n_K = 21 + 3 |K|, Sigma_slot = L L^T,
 *    eps_K computeNEES's error of the particle over the sensor rows and the kept landmarks in the slot's chart, z_K = L_KK^-1 eps_K and
 *    Xi = normals(seed, stream, n, P) of eqf_ensemble_random.h (eqf_bens_sample_seeded's counter map; only rows n_K .. n - 1 are used, generated in the kernel
 *    that reads them): eps_A = L_AK z_K + L_AA Xi_A and p_i = Q_i^-1 chart^-1(eps_A,i ; q0_i), as eqf_bens_sample_seeded forms a point. That is
 *    eps_A | eps_K ~ N(Sigma_AK Sigma_KK^-1 eps_K, the Schur complement), WITHOUT EVER FORMING THE SCHUR COMPLEMENT. For a landmark the step or
 *    eqf_batch_augment has just created Sigma_AK = 0: the draw is N(0, Sigma_AA) around q0, generateInitialStateParticles restricted to the new block. A cloud
 *    drawn by eqf_bens_sample_seeded(seed, stream), cut back to its first landmarks and followed with the same (seed, stream) gets its own points back.
 *
 * THE SUFFIX RULE. An entry is accepted only if A is a suffix of F: every id the cloud lacks sits behind every id it holds, in the slot's order. That is what
 * the product itself always produces: a step keeps the staying landmarks in state order, and both the step and eqf_batch_augment append new landmarks at the
 * end - so a cloud that was ever in step with its slot satisfies the rule, however many frames ago that was. Under the rule the slot's own order is "K first,
 * A last", the factor of Sigma_slot as it stands is the one needed and no permuted factorisation is built. A cloud put together by eqf_bens_set that breaks
 * the rule gets EQF_E_UNSUPPORTED for its entry.
 *
 * The other rules are those of every eqf_bens compute call:
 *  - arguments are checked BEFORE ANY DEVICE WORK, also on a machine without a GPU, and the call gives a status per entry. A refused entry leaves its cloud
 *    (ids included), its kept weights and its n_dropped / n_added outputs untouched bit for bit while the other entries run. The call returns 0 when it ran
 *    (whatever the per-entry codes) or count == 0, EQF_E_BAD_ARG for null entries or status or count < 0, EQF_E_CAPACITY when the device memory of the call could
 *    not be allocated (it is allocated at first use and freed by eqf_bens_destroy; the clouds are then untouched), or a HIP error;
 *  - the SLOT IS READ ONLY; synchronous, on the batch's stream; the ensemble and its batch are used from one thread at a time;
 *  - no kernel communicates between workgroups; every sum has a fixed order; A PARTICLE'S BYTES DEPEND ON ITS SLOT'S DATA, ITS OWN DATA AND (SEED, STREAM)
 *    ALONE: not on P, the entry's position or the company, and on its place in the cloud only in that its index k selects its column of the normals (the
 *    kept points do not depend on it at all);
 *  - per-entry codes: EQF_E_BAD_ARG a slot out of range or listed twice, or an empty cloud (P = 0); EQF_E_UNSUPPORTED the suffix rule is broken; EQF_E_NOT_SPD
 *    a pivot <= 0 or non-finite in the factorisation of that entry's Sigma, found on the device - the cloud's ids change only after the flags have been read,
 *    and that entry's planes have not moved.
 * ENTRIES THAT DO LESS. A = D = empty and G already in F's order: accepted, a no-op - nothing is touched, the kept weights stay valid, no factorisation is
 * counted. A = empty: no errors, no factor, no random numbers, only the move (or, where no kept landmark changes its place, only the id list); no factorisation
 * is counted. Every other accepted entry counts one factorisation in eqf_bens_stats; every accepted entry but the no-op INVALIDATES the slot's kept weights, as
 * eqf_bens_set, _sample_seeded and _integrate do.
 * LAUNCHES PER CALL, whatever the number of entries, any P and any N (counted by eqf_bens_stats): 3 when any accepted entry adds (eqf_bens_errors' kernel
 * over the kept landmarks; the factor; z_K, the normals and eps_A in one kernel: the blocked forward substitution and the triangular product both on
 * v_mfma_f64_16x16x4_f64), + 1 when any accepted entry moves a kept landmark (the kept planes into the slot's second place, the one of
 * eqf_batch_ensemble_output.h, allocated with it), + 1 when either holds (the kept planes back at their new places, the added points from eps_A). So 4, 2, 5 or
 * 0. The call is one packet to the device and one small copy back (the pivot flags of the adding entries).
 * Out of scope: caller-supplied normals; clouds whose missing ids are not a suffix of the slot's order; a weighted (un-resampled) covariance or NEES.
 * This header stands beside its implementation (eqvio_amd/csrc) and includes include/eqf_batch_ensemble.h: compile with both directories on the include path.
 */
#ifndef EQF_BATCH_ENSEMBLE_FOLLOW_H
#define EQF_BATCH_ENSEMBLE_FOLLOW_H
#include "eqf_batch_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eqf_bens_follow_entry {
    int slot;
    unsigned long long seed, stream; /* read only when the entry adds a landmark */
} eqf_bens_follow_entry;
/* n_dropped[e] = |D| and n_added[e] = |A| of every accepted entry; either may be null. */
int eqf_bens_follow(eqf_bens* e, int count, const eqf_bens_follow_entry* entries, int* n_dropped, int* n_added, int* status);

#ifdef __cplusplus
}
#endif
#endif
