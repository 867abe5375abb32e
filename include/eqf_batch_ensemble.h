/* eqf_batch_ensemble.h — particle ensembles against batch slots on the MI355X (gfx950): one cloud of P hypotheses of the TRUE state per slot of an
 * eqf_batch, B clouds sampled, moved and judged per call.
 *
 * eqf_batch_nees judges every slot against ONE true state; an eqf_ensemble (eqf_ensemble.h) judges ONE context against P. An eqf_bens joins them: it is
 * created against one eqf_batch with a fixed max_particles and holds, for EVERY slot of that batch, up to max_particles particles over one list of N <= 64
 * landmark ids per slot. One call samples a cloud from every listed slot's Sigma, one call moves every listed cloud with its slot's own IMU sample, one call
 * returns every particle's NEES against its slot - in all three charts (a Normal-chart slot is served like the others).
 *
 *   ONE FACTORISATION OF SIGMA PER (ENTRY, CALL), and a number of kernel launches and copies per call that depends neither on the number of entries nor on
 *   any P (eqf_bens_stats): sample_seeded 3 launches (factor, eps = L Xi, the chart inverses and group action), nees 3 (errors, factor, solve), integrate 2
 *   (sensor step, points), errors 1; every compute call is one packet to the device and one copy back.
 *
 * EVERYTHING OF A CLOUD IS ON THE DEVICE: the 23 sensor doubles of every particle as 23 planes (particles contiguous), the camera-frame points as 3 x 64
 * planes, the error coordinates E (np x P, np = n padded to even, n = 21 + 3 N <= 213) and one Cholesky factor L (np x np). The sensor part of sampling,
 * integration and the error - host work in eqf_ensemble.h - runs one lane per (entry, particle); the points one lane per (entry, particle, landmark). The
 * sensor error uses the cancellation-free logarithm of the single-filter ensemble (the (th / 2) cot(th / 2) form of so3_Vinv's coefficient).
 * MEMORY PER SLOT: 8 (23 + 192 + 214 + 1) ldp + 8 * 214 * 216 bytes with ldp = max_particles rounded up to 16 (+ 16 at multiples of 128): 3.8 MB at
 * max_particles = 1000, 1.3 MB at 256; times the slots of the batch. eqf_bens_create returns EQF_E_CAPACITY when an allocation fails, as eqf_batch_create.
 *
 * Rules of every call:
 *  - synchronous, on the batch's stream; the ensemble and its batch are used from one thread at a time;
 *  - the compute calls (sample_seeded, integrate, nees) take a list of entries, as every batch call does, and give a status per entry. Arguments are checked
 *    BEFORE ANY DEVICE WORK, also on a machine without a GPU. A refused entry leaves its cloud (and its output rows) untouched bit for bit; the other entries
 *    run. The call returns 0 when it ran (whatever the per-entry codes) or count == 0, EQF_E_BAD_ARG for null arguments or count < 0, or a HIP error;
 *  - the SLOT IS READ ONLY in every call: Sigma, the landmark planes, xi0 and X, the settings, the innovation totals, the last result and the current-buffer
 *    index are afterwards what they were; the slot's scratch area is not used;
 *  - per-entry codes: EQF_E_BAD_ARG a slot out of range or listed twice in the call, null pointers, sizes below 1 (P < 1, an empty cloud), or (errors, nees)
 *    a filter landmark id the cloud does not hold; EQF_E_CAPACITY P beyond max_particles or N beyond 64; EQF_E_NOT_SPD a pivot <= 0 or non-finite in the
 *    factorisation of that entry's Sigma (sample_seeded, nees) - there is NO partial-pivot fallback here, eqf_batch_nees keeps its own;
 *  - no kernel communicates between workgroups: no flags polled, no spinning, no co-residency. The pivot flag of an entry is written by the factor launch
 *    and read by the launches behind it;
 *  - every sum has a fixed order and A PARTICLE'S VALUE DEPENDS ON ITS SLOT'S DATA AND ITS OWN DATA ALONE: the same bytes from run to run, at any P, at any
 *    place in the cloud, at any entry position and whatever else the call lists.
 * Out of scope: caller-supplied normals. After a step has changed the slot's ids, nees and errors match by id as stated below and refuse an entry whose
 * cloud lacks one: clouds that follow a slot's landmark turnover are the call of eqf_batch_ensemble_follow.h on the same object. The measurement likelihood,
 * weightedResample and the particle covariance against slots are the three calls of eqf_batch_ensemble_output.h on the same object.
 */
#ifndef EQF_BATCH_ENSEMBLE_H
#define EQF_BATCH_ENSEMBLE_H
#include "eqf_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eqf_bens eqf_bens;

/* Room for 1 <= max_particles particles in every slot of `batch` (fixed). Every cloud is empty (P = N = 0) after creation. The batch must outlive the
 * ensemble. EQF_E_BAD_ARG: null out or batch, max_particles < 1; EQF_E_NO_DEVICE: no gfx950 device; EQF_E_CAPACITY: an allocation failed. */
int eqf_bens_create(eqf_bens** out, eqf_batch* batch, int max_particles);
void eqf_bens_destroy(eqf_bens* e);
/* particles and landmarks of the slot's cloud (null outputs are skipped) */
int eqf_bens_size(const eqf_bens* e, int slot, int* P, int* N);
/* kernel launches and factorisations of Sigma since the last reset (null outputs are skipped); a factorisation counts once per (entry, call) */
int eqf_bens_stats(eqf_bens* e, long* launches, long* factorisations, int reset);

/* One slot's cloud from / to the host, in eqf_ensemble_set's layouts: ids[N] (distinct), sensor 23 x P (particle k at sensor + 23 k), p 3 x N x P (point i of
 * particle k at p + 3 (N k + i)). get returns P (>= 0) or < 0; capP / capN are the room of the caller's arrays; null outputs are skipped. Byte-exact both
 * ways. EQF_E_BAD_ARG: bad slot, null arrays that are needed, P or N < 0, repeated ids; EQF_E_CAPACITY: P > max_particles, N > 64, or arrays too small. */
int eqf_bens_set(eqf_bens* e, int slot, int P, int N, const int* ids, const double* sensor, const double* p);
int eqf_bens_get(eqf_bens* e, int slot, int* ids, double* sensor, double* p, int capP, int capN);

/* generateInitialStateParticles for every listed slot: with Sigma_slot = L L^T (lower Cholesky factor) and Xi = normals(seed, stream, n, P) of
 * eqf_ensemble_random.h (the same Philox4x64-10 counter map and Box-Muller, generated in the kernel that reads them: nothing n x P crosses the bus),
 * eps = L Xi and particle k = stateGroupAction(X, stateChart^-1(eps_k ; xi0)) in the slot's chart, over the slot's ids in the slot's order. The slot's cloud
 * then holds P particles. eps = L Xi is a triangular product on v_mfma_f64_16x16x4_f64. */
typedef struct eqf_bens_sample_entry {
    int slot;
    int P;
    unsigned long long seed, stream;
} eqf_bens_sample_entry;
int eqf_bens_sample_seeded(eqf_bens* e, int count, const eqf_bens_sample_entry* entries, int* status);

/* integrateSystemFunction(particle_k, imu, dt) (VIOState.cpp:28-68) for every particle of every listed slot with that slot's own sample; imu13 = IMUVelocity.
 * With sigma6 (six standard deviations: gyr xyz, acc xyz) particle k is driven by gyr + sigma6[0:3] * z[0:3, k] and acc + sigma6[3:6] * z[3:6, k] with
 * z = normals(seed, stream, 6, P) (eqf_ensemble_integrate_seeded's definition); sigma6 == null: the sample as it is, seed and stream are not read. */
typedef struct eqf_bens_integrate_entry {
    int slot;
    const double* imu13;
    double dt;
    const double* sigma6;
    unsigned long long seed, stream;
} eqf_bens_integrate_entry;
int eqf_bens_integrate(eqf_bens* e, int count, const eqf_bens_integrate_entry* entries, int* status);

/* computeNEES's eps (VIO_eqf.cpp:153-165) of every particle of ONE slot in the slot's chart, n x P column-major (n the slot's dimension): a read-back for
 * tests and tools. Matched by id as eqf_bens_nees. Returns 0 or the entry's code. */
int eqf_bens_errors(eqf_bens* e, int slot, double* eps);

/* nees_out[e * max_particles + k] = eps_k^T Sigma^-1 eps_k / n for particle k of slots[e] (row e for entry e; the rest of a row is not written) and
 * mean_out[e] = (sum over k in index order) / P; either may be null. eps is computeNEES's error in the slot's chart; the particles' landmarks are matched to
 * the slot's ids BY ID - the cloud may hold more landmarks, in any order; a filter id it does not hold is EQF_E_BAD_ARG for that entry. Sigma is factorised
 * once per entry; a blocked forward substitution E^T L^-T (off-diagonal updates on v_mfma_f64_16x16x4_f64) and the rows' sums of squares share one launch. */
int eqf_bens_nees(eqf_bens* e, int count, const int* slots, double* nees_out, double* mean_out, int* status);

#ifdef __cplusplus
}
#endif
#endif
