/* eqf_ensemble.h — particle ensembles on the MI355X (gfx950): P hypotheses of the TRUE state, held on the device, judged against one eqf_ctx.
 *
 * The reference's statistical suite (test/test_FilterStatistics.cpp) holds one filter against a cloud of particles: it samples them from the filter's
 * Sigma (generateInitialStateParticles), integrates each with the true or a disturbed input (integrateSystemFunction), resamples them by a measurement
 * likelihood (weightedResample) and asks for the mean NEES and the particle covariance (estimateParticleCovariance). eqf_compute_nees answers that for
 * ONE true state per call - one factorisation of Sigma and one round trip each. An ensemble answers it for all P at once:
 *
 *   ONE FACTORISATION PER CALL. eqf_ensemble_nees and eqf_ensemble_sample factorise Sigma once, whatever P is; the P right-hand sides ride through the
 *   factorisation chain as extra rows of its work matrix. The number of launches and copies of every call does not depend on P (eqf_ensemble_stats).
 *
 * A particle is a VIOState: the 23 sensor doubles of eqvio_types.h (host resident, as a context's are) and N camera-frame points (device resident) over ONE
 * list of N landmark ids shared by all particles. Matrices are column-major; n = 21 + 3 N_ctx is the context's dimension.
 *
 * Rules of every call that takes a context:
 *  - arguments are checked before any device work; a refused call leaves the ensemble and the context untouched bit for bit;
 *  - the context is entered as eqf_compute_nees / eqf_get_state enter it (an unsettled update settled, a pending reshape applied) and is READ ONLY:
 *    Sigma, X, the landmark planes, every counter, the kept Gamma and the innovation totals are afterwards what they were;
 *  - refusal codes (eqf_hip.h): EQF_E_BAD_ARG a null pointer, a size out of range, an ensemble and a context on different devices, or (errors, nees,
 *    covariance) a filter landmark id the ensemble does not hold; EQF_E_CAPACITY P or N beyond the ensemble's capacity (or an output array too small);
 *    EQF_E_UNSUPPORTED a context with the float Sigma store (EQF_OPT_SIGMA_FP32 = 2); EQF_E_NOT_SPD a pivot <= 0 in the factorisation of Sigma
 *    (sample, nees) - there is NO partial-pivot fallback here: eqf_compute_nees keeps its own; EQF_E_NO_DEVICE no gfx950 device.
 *  - the kernels of this header do not communicate between workgroups (no flags, no spinning, no co-residency); the factorisation is the launch chain
 *    (one launch per 32-column panel), never the look-ahead kernel.
 * An ensemble is bound to one device and must be used from one thread at a time; every call returns with its work complete.
 * The random draws of sample, integrate and weighted resampling can be generated on the device from a seed: eqf_ensemble_random.h.
 */
#ifndef EQF_ENSEMBLE_H
#define EQF_ENSEMBLE_H
#include "eqf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eqf_ensemble eqf_ensemble;

/* Room for max_particles >= 1 particles of max_landmarks >= 0 landmarks (fixed: an ensemble does not grow). Empty (P = N = 0) after creation. */
int eqf_ensemble_create(eqf_ensemble** out, int device, int max_particles, int max_landmarks);
void eqf_ensemble_destroy(eqf_ensemble* e);
int eqf_ensemble_size(const eqf_ensemble* e, int* P, int* N);

/* The particles from / to the host: ids[N] (distinct), sensor 23 x P, p 3 x N x P (point i of particle k at p + 3 (N k + i)). get returns P (>= 0) or < 0;
 * capP / capN are the room of the caller's arrays in particles and landmarks; null outputs are skipped. Bit-exact both ways. */
int eqf_ensemble_set(eqf_ensemble* e, int P, int N, const int* ids, const double* sensor, const double* p);
int eqf_ensemble_get(eqf_ensemble* e, int* ids, double* sensor, double* p, int capP, int capN);

/* generateInitialStateParticles (test_FilterStatistics.cpp) for any X and with the exact inverse chart: with Sigma = L L^T (lower Cholesky factor) and the
 * caller's standard normals xi (n x P), eps_k = L xi_k and particle_k = stateGroupAction(X, stateChart^-1(eps_k ; xi0)). The ensemble then holds P particles
 * over the context's ids in the context's order. L comes from ONE run of the factorisation chain on [Sigma ; Sigma] (the rows below the square leave as
 * Sigma L^-T = L), eps = L Xi is a triangular product on v_mfma_f64_16x16x4_f64, the chart inverses and the group action run one lane per (particle, landmark),
 * the 21 sensor coordinates of each particle on the host. A pivot <= 0: EQF_E_NOT_SPD, the ensemble untouched. */
int eqf_ensemble_sample(eqf_ensemble* e, eqf_ctx* ctx, int P, const double* xi);

/* integrateSystemFunction(particle_k, imu, dt) (VIOState.cpp:28-68) for every particle; imu13 = IMUVelocity. imu_offset (6 x P, or null): particle k is driven by
 * gyr + imu_offset[0:3, k] and acc + imu_offset[3:6, k]. The points run one lane per (particle, landmark). */
int eqf_ensemble_integrate(eqf_ensemble* e, const double* imu13, double dt, const double* imu_offset);

/* computeNEES's eps (VIO_eqf.cpp:153-165) for every particle, in the context's chart: eps_k = stateChart(stateGroupAction(X^-1, particle_k restricted to the
 * filter's ids) ; xi0), eps n x P. Matched by id: the particles may hold more landmarks than the filter, in any order. */
int eqf_ensemble_errors(eqf_ensemble* e, eqf_ctx* ctx, double* eps);

/* nees[k] = eps_k^T Sigma^-1 eps_k / n for every particle and *mean = (sum over k in index order) / P (either may be null). eps is formed on the device and Sigma
 * is factorised ONCE per call: Z = [Sigma padded to an even dimension ; E^T] goes through the chain with np + P rows, the rows below the square leave as
 * E^T L^-T, and one kernel sums each row's squares in a fixed order. The value of a particle does not depend on run, on P, or on its place in the ensemble. */
int eqf_ensemble_nees(eqf_ensemble* e, eqf_ctx* ctx, double* nees, double* mean);

/* estimateParticleCovariance: C = (1 / P) sum_k eps_k eps_k^T (n x n), a tiled product over the particles on fp64 MFMA, summed in particle order; the upper half
 * is written from the values of the lower half (exactly symmetric). */
int eqf_ensemble_covariance(eqf_ensemble* e, eqf_ctx* ctx, double* cov);

/* The ensemble becomes particles src[0 .. P_new) of the current one (any indices in [0, P), repeats allowed, 1 <= P_new <= capacity): a gather through the
 * second particle buffer. weightedResample's random draws and the measurement likelihood stay with the caller (or: eqf_ensemble_output.h forms the likelihood
 * and runs weightedResample on the device from the caller's uniforms). */
int eqf_ensemble_resample(eqf_ensemble* e, int P_new, const int* src);

/* kernel launches and factorisations of Sigma since the last reset (null outputs are skipped) */
int eqf_ensemble_stats(eqf_ensemble* e, long* launches, long* factorisations, int reset);

#ifdef __cplusplus
}
#endif
#endif
