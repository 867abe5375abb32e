/* eqf_batch_ensemble_output.h — the measurement side of the particle ensembles against batch slots (eqf_batch_ensemble.h) on the MI355X (gfx950): the
 * likelihood of one measurement per slot under every particle of that slot's cloud, the reference's weightedResample on those weights, and
 * estimateParticleCovariance, for every listed slot of an eqf_bens per call.
 *
 * With eqf_bens_sample_seeded, _integrate and _nees these three calls complete the reference's statistical suite (test/test_FilterStatistics.cpp) for B slots per
 * launch: its fourth check, outputDistribution (lines 140-168), weighs every particle by the measurement likelihood, runs weightedResample, lets the filter take
 * the measurement and asks for the mean NEES again; estimateParticleCovariance is lines 63-75. NOTHING P-SIZED CROSSES THE BUS except the results the caller
 * asks for (a null output is not copied).
 *
 * Per entry, eqf_bens_likelihood IS eqf_ensemble_likelihood (eqf_ensemble_output.h) of that slot's cloud and eqf_bens_resample_weighted_seeded IS
 * eqf_ensemble_resample_weighted_seeded (eqf_ensemble_random.h) on the kept weights: the same definitions, THE SAME ORDERS OF THE SUMS, the likelihood formed IN
 * THE LOG DOMAIN, the same counter map of the uniforms.
 *
 * Rules of the three calls - those of every eqf_bens compute call:
 *  - a list of entries and a status per entry. Arguments are checked BEFORE ANY DEVICE WORK, also on a machine without a GPU. A refused entry leaves its cloud,
 *    its kept weights and its output rows untouched bit for bit while the other entries run. The call returns 0 when it ran (whatever the per-entry codes) or
 *    count == 0, EQF_E_BAD_ARG for null arguments or count < 0, EQF_E_CAPACITY when the device memory of these calls could not be allocated (it is allocated
 *    at their first use; the clouds are then untouched), or a HIP error;
 *  - the SLOT IS READ ONLY; synchronous, on the batch's stream; the ensemble and its batch are used from one thread at a time;
 *  - no kernel communicates between workgroups; every sum has a fixed order; A PARTICLE'S VALUE DEPENDS ON ITS OWN DATA AND ITS ENTRY'S ALONE: the same bytes
 *    from run to run, at any entry position and whatever else the call lists;
 *  - LAUNCHES PER CALL, whatever the entries, P, M and N (counted by eqf_bens_stats): likelihood 2 (the log-likelihoods of all entries; the weights, one
 *    workgroup per entry), resample_weighted_seeded 3 (the choice, with its uniforms; the gather into the slot's second place; the copy back), covariance 2
 *    (eqf_bens_errors' kernel; the product). Every call is one packet to the device and at most one copy back.
 *  - THE KEPT WEIGHTS: eqf_bens_likelihood keeps an accepted entry's running sums per slot on the device. eqf_bens_set, eqf_bens_sample_seeded,
 *    eqf_bens_integrate (accepted entries) and eqf_bens_resample_weighted_seeded INVALIDATE them for the slots they touch.
 * MEMORY PER SLOT, on top of eqf_batch_ensemble.h's and allocated at the first of these calls: 8 (215 + 1 + 2) ldp + 4 ldp bytes - the gather's second place
 * (23 + 192 planes), the running sums, and the slot's share of the per-entry rows (log-likelihoods, weights, indices): 1.8 MB at max_particles = 1000, 0.5 MB at
 * 256. eqf_bens_covariance stages count * 213 * 213 doubles, allocated on first use and grown to the largest count seen.
 * Out of scope: caller-supplied uniforms or weights; a weighted (un-resampled) covariance or NEES; P beyond what one workgroup per entry normalises in a few
 * microseconds. Clouds that follow a slot's landmark turnover are the call of eqf_batch_ensemble_follow.h, which shares the gather's second place.
 */
#ifndef EQF_BATCH_ENSEMBLE_OUTPUT_H
#define EQF_BATCH_ENSEMBLE_OUTPUT_H
#include "eqf_batch_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

/* loglik[k] = -1/2 (sum_j |y_j - projectPoint(p_{k, ids[j]})|^2) / meas_var for particle k of the slot's cloud (y_j = y[2 j], y[2 j + 1]); lane group g of 8
 * adds the squared residuals (u then v, fused multiply-add) of j = g, g + 8, ... in ascending order and the partial sums are added as
 * ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)). weights[k] = exp(loglik[k] - max) / sum, logsumexp = max + log(sum), ess = 1 / sum_k weights[k]^2, the
 * runs, offsets and running sums over 256 lanes in eqf_ensemble_output.h's order, fixed by P alone, c_(P-1) = 1 exactly. cam: any of the three models.
 * Measurement ids are MATCHED BY ID to the cloud's: any subset, in any order. M = 0: loglik +0.0, uniform weights. A NON-FINITE loglik counts as -infinity and
 * gets weight 0; an entry with no finite particle gets EQF_E_NONFINITE and KEEPS NOTHING (weights kept for its slot by an earlier call are gone too), the other
 * entries are unaffected. Row e of loglik_out / weights_out starts at e * max_particles and holds P values; the rest of the row is not written. logsumexp_out[e]
 * and ess_out[e] per entry. Any output may be null. The particles are read only.
 * EQF_E_BAD_ARG per entry: a slot out of range or listed twice, null cam / ids / y with M > 0, a camera model outside the enum, M < 0, an empty cloud, meas_var
 * <= 0 or not finite, an id the cloud does not hold or a repeated id. */
typedef struct eqf_bens_likelihood_entry {
    int slot;
    const eqvio_camera* cam;
    const int* ids;
    const double* y;
    int M;
    double meas_var;
} eqf_bens_likelihood_entry;
int eqf_bens_likelihood(eqf_bens* e, int count, const eqf_bens_likelihood_entry* entries, double* loglik_out, double* weights_out, double* logsumexp_out,
                        double* ess_out, int* status);

/* weightedResample (testing_utilities.h:55-74) on the slot's kept weights with u = uniforms(seed, stream, P_new) of eqf_ensemble_random.h, generated in the
 * kernel that reads them (draw i is word i & 3 of the block of counter (i >> 2, 0, 0, 1)): new particle k is old particle
 * src_k = min{ j : c_j >= (u_k + k) / P_new }, or P - 1 if there is none (a binary search per new particle). The cloud then holds P_new particles: all 23 sensor
 * planes and 3 N point planes are gathered on the device through the slot's second place. Row e of src_out (or null), at e * max_particles, receives the P_new
 * indices. The slot's kept weights are invalid afterwards.
 * Per entry EQF_E_BAD_ARG: a slot out of range or listed twice, P_new < 1, no valid kept weights; EQF_E_CAPACITY: P_new > max_particles. */
typedef struct eqf_bens_resample_entry {
    int slot;
    int P_new;
    unsigned long long seed, stream;
} eqf_bens_resample_entry;
int eqf_bens_resample_weighted_seeded(eqf_bens* e, int count, const eqf_bens_resample_entry* entries, int* src_out, int* status);

/* estimateParticleCovariance: C = (1 / P) sum_k eps_k eps_k^T with eps computeNEES's error of particle k in the slot's chart, matched BY ID as eqf_bens_nees
 * (a filter id the cloud does not hold, or an empty cloud, is EQF_E_BAD_ARG for that entry). Entry e's matrix is n_e x n_e column-major with leading dimension
 * n_e (n_e = 21 + 3 N of slots[e]) at cov_out + e * 213 * 213; the rest of that block is not written. The product runs on v_mfma_f64_16x16x4_f64 over the 16 x 16
 * tiles of the lower triangle, particles in ascending steps of 4; the upper half is written from the lower half's registers: C == C^T exactly. No factorisation.
 * The clouds and the kept weights are what they were. */
int eqf_bens_covariance(eqf_bens* e, int count, const int* slots, double* cov_out, int* status);

#ifdef __cplusplus
}
#endif
#endif
