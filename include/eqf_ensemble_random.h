/* eqf_ensemble_random.h — the random draws of a particle ensemble (eqf_ensemble.h, eqf_ensemble_output.h) generated on the MI355X (gfx950) from a seed: the
 * standard normals eqf_ensemble_sample consumes, the uniforms of eqf_ensemble_resample_weighted and the input disturbances of eqf_ensemble_integrate, none of
 * which crosses the bus any more, and all of which any caller of this header reproduces from two 64-bit words.
 *
 * THE GENERATOR is Philox4x64-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the generator of numpy's np.random.Philox:
 *   multipliers M0 = 0xD2E7470EE14C6C93, M1 = 0xCA5A826395121157; key increments 0x9E3779B97F4A7C15 (k0), 0xBB67AE8584CAA73B (k1); ten rounds;
 *   a round is (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped after each round;
 *   KEY = (seed, stream), the caller's two words; the four output words of a counter are x0 .. x3.
 *   np.random.Philox(key=[seed, stream], counter=c - 1).random_raw(4) is the block of counter c (numpy increments before it generates).
 *
 * WORD TO UNIFORM: U(x) = (2 (x >> 12) + 1) 2^-53, an odd multiple of 2^-53: exact in fp64, strictly inside (0, 1), symmetric about 1/2 (U(x) + U(~x) = 1).
 * A logarithm never sees 0.
 *
 * COUNTER MAP.
 *   normals:  rows 4 j .. 4 j + 3 of particle k come from counter (j, k, 0, 0). BOX-MULLER pairing: words (x0, x1) give r = sqrt(-2 log U(x0)),
 *             z(4 j) = r cospi(2 U(x1)), z(4 j + 1) = r sinpi(2 U(x1)); words (x2, x3) give rows 4 j + 2 and 4 j + 3 the same way. 2 U is exact, so the device's
 *             sincospi gets an exact argument; log, sqrt and sincospi are the plain fp64 functions.
 *   uniforms: draw i is U(word i & 3 of counter (i >> 2, 0, 0, 1)).
 *
 * Contract:
 *  - A value depends on seed, stream, row and particle alone: the same bits run to run, at any P, at any number of rows and at any place in the ensemble. Entry
 *    (r, k) is one value in every request that contains it.
 *  - Choosing DISTINCT STREAMS FOR DISTINCT DRAWS is the caller's business: two calls with the same (seed, stream) draw the same numbers.
 *  - THE THREE EQUALITIES, each byte for byte:
 *      eqf_ensemble_sample_seeded(e, ctx, P, seed, stream)                    == eqf_ensemble_sample(e, ctx, P, xi), xi = eqf_ensemble_normals(seed, stream, n, P);
 *      eqf_ensemble_resample_weighted_seeded(e, P_new, w, seed, stream, src)  == eqf_ensemble_resample_weighted(e, P_new, w, u, src), u = eqf_ensemble_uniforms(seed, stream, P_new);
 *      eqf_ensemble_integrate_seeded(e, imu13, dt, sigma6, seed, stream)      == eqf_ensemble_integrate(e, imu13, dt, off),
 *                                                                                off[c + 6 k] = sigma6[c] * eqf_ensemble_normals(seed, stream, 6, P)[c + 6 k].
 *  - Arguments are CHECKED BEFORE ANY DEVICE WORK: EQF_E_BAD_ARG for a null pointer or a size below 1, EQF_E_CAPACITY beyond the capacities, and everything
 *    eqf_ensemble_sample, eqf_ensemble_resample_weighted and eqf_ensemble_integrate refuse, with their codes. A refused call leaves the ensemble, the kept weights
 *    and the context untouched bit for bit.
 *  - LAUNCHES AND COPIES, none depending on P: normals and uniforms 1 launch, 1 copy out; sample_seeded the launches of eqf_ensemble_sample + 1, one
 *    factorisation, and NO n x P COPY; resample_weighted_seeded the launches of eqf_ensemble_resample_weighted + 1 and no copy of uniforms; integrate_seeded the
 *    launches of eqf_ensemble_integrate + 1 and one copy out of 6 P doubles. eqf_ensemble_stats counts these launches.
 *  - No kernel uses LDS or talks to another workgroup.
 * Every call returns with its work complete; an ensemble is used from one thread at a time.
 */
#ifndef EQF_ENSEMBLE_RANDOM_H
#define EQF_ENSEMBLE_RANDOM_H
#include "eqf_ensemble_output.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The generator read back: out[r + rows k] (rows x P, column-major) standard normals, 1 <= rows <= the ensemble's padded state capacity (21 + 3 max_landmarks,
 * made even), 1 <= P <= max_particles. The particles and the kept weights are what they were. */
int eqf_ensemble_normals(eqf_ensemble* e, unsigned long long seed, unsigned long long stream, int rows, int P, double* out);

/* out[i], i < count, uniforms in (0, 1); 1 <= count <= max_particles. The particles and the kept weights are what they were. */
int eqf_ensemble_uniforms(eqf_ensemble* e, unsigned long long seed, unsigned long long stream, int count, double* out);

/* eqf_ensemble_sample with xi = the n x P normals of (seed, stream), generated on the context's stream into the device array the upload used to land in. */
int eqf_ensemble_sample_seeded(eqf_ensemble* e, eqf_ctx* ctx, int P, unsigned long long seed, unsigned long long stream);

/* eqf_ensemble_resample_weighted with u = the P_new uniforms of (seed, stream), generated into the array the index choice reads. weights == null: the kept ones
 * (EQF_E_BAD_ARG without valid kept weights). src_out[P_new] or null. */
int eqf_ensemble_resample_weighted_seeded(eqf_ensemble* e, int P_new, const double* weights, unsigned long long seed, unsigned long long stream, int* src_out);

/* eqf_ensemble_integrate with imu_offset[c + 6 k] = sigma6[c] * normals(seed, stream, 6, P)[c + 6 k]; sigma6: six standard deviations, gyr xyz then acc xyz.
 * The 6 x P normals come back in one copy and the product is one IEEE multiply on the host, where the sensor step runs. */
int eqf_ensemble_integrate_seeded(eqf_ensemble* e, const double* imu13, double dt, const double* sigma6, unsigned long long seed, unsigned long long stream);

#ifdef __cplusplus
}
#endif
#endif
