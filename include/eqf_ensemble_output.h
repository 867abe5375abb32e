/* eqf_ensemble_output.h — the measurement side of a particle ensemble (eqf_ensemble.h) on the MI355X (gfx950): what every particle would measure, the
 * likelihood of one measurement under every particle, and the reference's weightedResample, all on the device.
 *
 * The reference's fourth statistical check (test/test_FilterStatistics.cpp:140-168, outputDistribution) weighs every particle by exp(-1/2 e^T R^-1 e) and
 * resamples by those weights. Its plain formula does not survive the sizes an ensemble is built for: at 40 landmarks and 1000 particles the weights sum to a
 * denormal, at 70 landmarks the sum is exactly 0 and every weight NaN. Here the likelihood is formed IN THE LOG DOMAIN: the weights are exp(loglik - max),
 * divided by their sum.
 *
 * Matrices are column-major. cam is an eqvio_camera of any of the three models. Measurement ids are MATCHED BY ID to the ensemble's: any subset of them, in any
 * order; an id the ensemble does not hold, or a repeated id, is EQF_E_BAD_ARG.
 *
 * Contract of the three calls:
 *  - A particle's loglik is summed over j IN A FIXED ORDER (below) and depends on that particle's own points alone: the same bits run to run, at any P and at
 *    any place in the ensemble - the property eqf_ensemble_nees has.
 *  - M = 0: loglik is 0 (+0.0) and the weights are uniform.
 *  - A NON-FINITE loglik (a point with z = 0, a NaN coordinate) COUNTS AS -INFINITY and gets weight 0; loglik[k] is returned as -infinity. (The reference would
 *    return NaN for every weight.) If no particle is finite the call returns EQF_E_NONFINITE and KEEPS NOTHING: weights kept by an earlier call are gone too.
 *  - The maximum, the sum, ess and the running sums are each formed IN ONE FIXED ORDER, fixed by P alone, and have the same bits run to run:
 *      lane l of the one workgroup of 256 owns the contiguous run [l R, min(P, (l + 1) R)), R = ceil(P / 256);
 *      max: over the finite logliks (order-free);
 *      t_l = the run's e_j = exp(loglik_j - max) added in ascending j from 0; o_l = t_0 + ... + t_(l-1) added in ascending l from 0; sum = o_255 + t_255;
 *      running sum c_j = (o_l + (e_(l R) + ... + e_j, ascending from 0)) / sum: non-decreasing in j, and c_(P-1) = 1 exactly;
 *      weights[j] = e_j / sum; sum of squares: each run in ascending j, the 256 run values by the halving tree s[l] += s[l + h], h = 128, 64, ..., 1.
 *  - THE KEPT WEIGHTS: eqf_ensemble_likelihood keeps its normalised weights and running sums on the device. eqf_ensemble_set, _sample, _integrate, _resample and
 *    _resample_weighted INVALIDATE them; eqf_ensemble_resample_weighted(weights = null) without valid kept weights is EQF_E_BAD_ARG.
 *  - Arguments are CHECKED BEFORE ANY DEVICE WORK (a null ensemble, cam, ids, y or u; a camera model outside the enum; M < 0; an empty ensemble; meas_var <= 0 or
 *    not finite; a u outside [0, 1); P_new < 1; a weight that is negative or not finite, or weights that are all zero: EQF_E_BAD_ARG. P_new beyond the ensemble's
 *    capacity: EQF_E_CAPACITY). A refused call leaves the ensemble, and the kept weights, untouched bit for bit.
 *  - The number of LAUNCHES AND COPIES per call DEPENDS ON NEITHER P NOR M: measure 1 launch, 1 copy in, 1 out (nothing at all at M = 0); likelihood 2 launches, 2 copies in (none at M = 0), 1 out;
 *    resample_weighted 2 launches (3 with the caller's weights; one fewer in an ensemble without landmarks: nothing to gather), 1 copy in (2), 1 out.
 *    eqf_ensemble_stats counts these launches.
 *  - No kernel talks to another workgroup, and NO CALL TAKES OR TOUCHES A CONTEXT.
 * Every call returns with its work complete; an ensemble is used from one thread at a time.
 */
#ifndef EQF_ENSEMBLE_OUTPUT_H
#define EQF_ENSEMBLE_OUTPUT_H
#include "eqf_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

/* measureSystemState (VIOState.cpp:70-78) of every particle: y_out[2 (M k + j) + c] = cam.projectPoint(p_{k, ids[j]})[c], a lane per (particle, measured
 * landmark). M >= 0. Read only: the ensemble and the kept weights are what they were. */
int eqf_ensemble_measure(eqf_ensemble* e, const eqvio_camera* cam, const int* ids, int M, double* y_out);

/* loglik[k] = -1/2 * (sum_j |y_j - projectPoint(p_{k, ids[j]})|^2) / meas_var  (outputGain = meas_var I, as eqf_vision_update's; y_j = y[2 j], y[2 j + 1]),
 * weights[k] = exp(loglik[k] - max) / sum_k exp(loglik[k] - max), *logsumexp = max + log(sum), *ess = 1 / sum_k weights[k]^2. Any output may be null.
 * The sum over j: lane group g of 8 adds the squared residuals (u then v, fused multiply-add) of j = g, g + 8, g + 16, ... in ascending order, and the eight
 * partial sums are added as ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)). The normalised weights are KEPT on the device for
 * eqf_ensemble_resample_weighted. The particles themselves are read only. */
int eqf_ensemble_likelihood(eqf_ensemble* e, const eqvio_camera* cam, const int* ids, const double* y, int M, double meas_var, double* loglik, double* weights,
                            double* logsumexp, double* ess);

/* weightedResample (testing_utilities.h:55-74) with the caller's uniforms u[P_new] in [0, 1): new particle k is old particle
 * src_k = min{ j : c_j >= (u[k] + k) / P_new }, or P - 1 if there is none, c_j the running sums above (a binary search per new particle; the thresholds increase
 * with k, so this is what the reference's running loop returns on the same running sums). weights == null: the kept ones; otherwise weights[P] >= 0, finite, not
 * all zero, divided on the device by their sum (e_j = weights[j] in the orders above). The ensemble then holds P_new particles (the points gathered on the device
 * through the second particle buffer, the 23 sensor doubles on the host); src_out[P_new] (or null) receives the indices. */
int eqf_ensemble_resample_weighted(eqf_ensemble* e, int P_new, const double* weights, const double* u, int* src_out);

#ifdef __cplusplus
}
#endif
#endif
