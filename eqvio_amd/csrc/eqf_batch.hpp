// Filter batch (include/eqf_batch.h): B independent filters of at most 64 landmarks, one workgroup per slot, ONE launch per frame of all of them.
// The device side: the packet structs and the kernels. The host side (the batch object, its packet buffers, the entry points) is eqf_batch_host.hpp;
// eqf_hip.hip includes both. Every piece of EqF arithmetic below is a helper of eqf_kernels.hpp / eqf_math.hpp, called unchanged.
//
// Per slot s, in HBM (fp64): two Sigma buffers (n x n column-major, leading dimension ld, n <= 21 + 3 * 64), two landmark buffers (35 SoA planes of stride
// BATCH_L: q0 and its chart constants - the layout ld_cc expects -, Qq, Qa) and one scratch area (F Sigma, then [T ; yTilde^T] -> [W^T ; z^T] and L dense,
// the statistics): 1.2 MB per slot, more than the Infinity Cache holds at 256 slots.
// The slot's current buffers are named by the host (BatchIn::cur); the frame ends in the same pair or, when removeInvalidLandmarks drops a landmark, in the other.
// A workgroup only ever touches its own slot's memory: no flags, no spin, no co-residency needed; the grid may exceed the compute units.
// The filter settings a frame reads (chart, output, lifts, depth choice, thresholds, R, initial variance and depth, Q, P) are the SLOT's: BatchIn::ss, copied by
// the host from the slot's settings into the packet entry of every step (eqf_batch_set_slot_settings), so one launch runs B different tunings.
//
// The phases of k_batch_frame (VIOFilter::processVisionData, fast Riccati, src/VIOFilter.cpp:194-241; its body is eqf_batch_frame_body.inc). With accurate
// Riccati (eqf_batch_step_accurate) k_batch_riccati does what phases 0 and 1 do - one accurate Riccati step per IMU sample between the observer steps - and
// k_batch_frame_tail, the same body from phase 2 on, the rest; with the discrete state matrix (eqf_batch_step_discrete) k_batch_discrete stands in k_batch_riccati's place:
//   0  rows of A and B of the surviving landmarks (assemble_landmark, sensor_Ass_entry / sensor_Bs_entry) into LDS; origin planes copied to the other
//      buffer; the observer steps' landmark part (observer_chain) applied on the way. Landmarks the host found unmeasured (removeOldLandmarks) are not copied:
//      the propagation is block triangular, so marginalising a landmark before or after it leaves every other entry the same.
//   1  Sigma' = F Sigma F^T + dt (B Q B^T + P), F = I + dt A (integrateRiccatiStateFast): G = F Sigma into scratch, then Sigma' = G F^T (lower half, mirrored).
//   2  removeOutliers: statistics (outlier_stats_body), ranking (absolute outliers first by error, then probabilistic ones), at most max_outliers discarded.
//   3  addNewLandmarks: median of the squared depths (the nth_element element) or the fixed depth; the survivors, then the new landmarks (Q = identity,
//      initialPointVariance I) go back to the first buffer pair.
//   4  performVisionUpdate: C / yTilde (measure_one), T = Sigma C^T (bz_T_pair), S = C Sigma C^T + R (bz_S_block, packed lower triangle in LDS), Cholesky
//      S = L L^T, W = L^-1 T^T and z = L^-1 yTilde by a blocked solve (MFMA products, VALU diagonal triangles), the innovation statistics NIS = |z|^2 and
//      log det S = 2 sum log L_kk (batch_wave_sum, from LDS), Gamma = W^T z, Sigma -= W^T W in MFMA tiles, landmark lift (lift_landmark); Gamma's 21 sensor
//      rows go back to the host, which lifts the sensor part.
//   5  removeInvalidLandmarks: flagged by the lift, compacted into the other buffer pair.
// A pivot <= 0 (EQF_E_NOT_SPD) or a non-finite Gamma (EQF_E_NONFINITE) ends the frame before anything of the update is written: the slot then holds the frame's
// propagation and landmark bookkeeping (phases 0 - 3) without the update.
#pragma once
#include "eqf_batch.h"
#include "eqf_kernels.hpp"

namespace eqf {

constexpr int BATCH_T = 256;                  // threads per workgroup (one slot)
constexpr int BATCH_L = 64;                   // landmarks per slot at most; plane stride of the landmark buffers
constexpr int BATCH_MAXM = 2 * BATCH_L;       // rows of S at most
constexpr int BATCH_NMAX = 21 + 3 * BATCH_L;  // state dimension at most
constexpr int BATCH_QQ = CC_OFF + CC_PLANES;  // plane of Qq (4 planes) in a landmark buffer
constexpr int BATCH_QA = BATCH_QQ + 4;        // plane of Qa
constexpr int BATCH_PLANES = BATCH_QA + 1;    // 35 planes
constexpr int BATCH_SPACK = BATCH_MAXM * (BATCH_MAXM + 1) / 2;

// result flags (BatchOut::did)
enum { BATCH_DID_OUTLIERS = 1, BATCH_DID_ADDED = 2, BATCH_DID_UPDATE = 4, BATCH_DID_INVALID = 8, BATCH_DID_EMPTY = 16 };

// The settings a slot's frame reads (eqf_batch_set_slot_settings): the slot's own values, carried by its packet entry, so one launch runs B different tunings.
struct BatchSlotSet {
    int chart, star, discrete, median;
    double thrAbs, thrProb, meas_var, init_var, init_depth;
    double Qd[12], Pd[8];
};
// one slot's frame, prepared by the host (eqf_batch_step)
struct BatchIn {
    int slot, cur;
    int Ns;           // landmarks that survive removeOldLandmarks
    int M;            // features of the measurement (ascending id)
    int nnew;         // of those, ids not in the state
    int k, obs_off;   // observer steps: ba.steps[obs_off .. obs_off + k)
    int max_outliers; // (size_t)((1 - featureRetention) * M)
    int surv[BATCH_L]; // state index (before the frame) of surviving landmark i
    int midx[BATCH_L]; // feature j: surviving landmark index, or -(1 + r) for the r-th new id
    double y[2 * BATCH_L];
    double bear[3 * BATCH_L]; // undistorted bearing of the r-th new id
    double dt;                // dt_total of the Riccati step
    Cam cam;
    CommonK ck;               // sensor-level terms of A and B at the current X (compute_common)
    BatchSlotSet ss;          // the slot's settings
};
struct BatchOut {
    int status, N, cur, did;
    unsigned long long outliers; // bits: surviving landmark index discarded by removeOutliers
    unsigned long long invalid;  // bits: landmark index (after addNewLandmarks) removed by removeInvalidLandmarks
    double gamma[21];            // sensor rows of Gamma
    double depth;                // depth the new landmarks got
    int dof;                     // rows m of the matched measurement (0: empty)
    double nis, logdet;          // yTilde^T S^-1 yTilde and log det S of the update (NaN when the update failed)
    int ric_samples, ric_squarings; // k_batch_riccati's / k_batch_discrete's: samples with dt > 0, the most squarings an exponential took (eqf_batch_last_riccati)
};
// The slots' buffers, the same for every kernel: slot s has two Sigma buffers and two landmark buffers (which = 0 / 1; the host names the current one) and one
// scratch area.
struct BatchBufs {
    int ld; // leading dimension of a Sigma buffer
    double *sig, *lm, *scr;
    size_t sig_stride, lm_stride, scr_stride; // doubles per buffer
    __host__ __device__ double* sig_of(int slot, int which) const { return sig + (2 * (size_t)slot + which) * sig_stride; }
    __host__ __device__ double* lm_of(int slot, int which) const { return lm + (2 * (size_t)slot + which) * lm_stride; }
    __host__ __device__ double* scr_of(int slot) const { return scr + (size_t)slot * scr_stride; }
};
struct BatchArgs {
    BatchBufs buf;
    const BatchIn* in;
    const ObsStep* steps;
    BatchOut* out;
};
// scratch layout of a slot: [0, ld * BATCH_NMAX) G = F Sigma, later T / W (m16 <= BATCH_MAXM columns) and, behind them, L (BATCH_MAXM^2); then the statistics rows
constexpr size_t batch_scr_doubles(int ld) { return (size_t)ld * BATCH_NMAX + 16 * BATCH_L; }

__device__ __forceinline__ int bt_tri(int i, int j) { return i * (i + 1) / 2 + j; } // packed lower triangle, i >= j

// LDS: one region reused by the phases (propagation: A / B rows; update: S, C, yTilde, z, Gamma)
constexpr int BATCH_SM_PROP = 441 + 252 + 66 + BATCH_L * 45 + BATCH_L * 9;
constexpr int BATCH_SM_UPD = BATCH_SPACK + BATCH_L * 6 + BATCH_MAXM + BATCH_MAXM + BATCH_NMAX + 3;
constexpr int BATCH_SM = BATCH_SM_PROP > BATCH_SM_UPD ? BATCH_SM_PROP : BATCH_SM_UPD;
static_assert(BATCH_SM_PROP + 20 <= BATCH_SM, "the slot's Qd / Pd sit behind the propagation rows");

// Sum of one wave's 64 values in a fixed order (the butterfly's pairing depends on the lane numbers alone); every lane gets it.
__device__ __forceinline__ double batch_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o, 64);
    return v;
}
// the lanes of one wave see each other's LDS stores behind this
__device__ __forceinline__ void batch_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// tile t of a lower triangle of tiles counted row by row: its row bi and column bj <= bi
__device__ __forceinline__ void batch_tri_tile(int t, int& bi, int& bj) {
    bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= t)
        ++bi;
    bj = t - bi * (bi + 1) / 2;
}
// addNewLandmarks' entry i of a landmark buffer: origin point p with its chart constants, Q = identity, a = 1
__device__ __forceinline__ void batch_new_landmark(double* planes, int i, double px, double py, double pz) {
    const int L = BATCH_L;
    planes[i] = px;
    planes[L + i] = py;
    planes[2 * L + i] = pz;
    store_chart_constants(planes + (size_t)CC_OFF * L, L, i, px, py, pz, nullptr);
    planes[BATCH_QQ * L + i] = 1.0;
    planes[(BATCH_QQ + 1) * L + i] = 0.0;
    planes[(BATCH_QQ + 2) * L + i] = 0.0;
    planes[(BATCH_QQ + 3) * L + i] = 0.0;
    planes[BATCH_QA * L + i] = 1.0;
}
// dst (n x n) = src gathered through gidx (LDS); a row or column with gidx < 0 is a new landmark's: zero cross terms, init_var on the diagonal
// (init_var by reference: k_batch_augment's stays in its packet entry until an element needs it, as before the two loops became this one)
__device__ __forceinline__ void batch_gather_sigma(double* dst, const double* src, const int* gidx, int n, int ld, const double& init_var) {
    for (int t = threadIdx.x; t < n * n; t += BATCH_T) {
        const int r = t % n, c = t / n;
        const int gr = gidx[r], gc = gidx[c];
        dst[r + (size_t)c * ld] = (gr >= 0 && gc >= 0) ? src[gr + (size_t)gc * ld] : (r == c ? init_var : 0.0);
    }
}
// what a frame reports however it ends (one thread); did, outliers, depth and gamma are written where they are decided
__device__ __forceinline__ void batch_finish(BatchOut* out, int status, int N, int cur, unsigned long long invalid, int dof, double nis, double logdet) {
    out->status = status;
    out->N = N;
    out->cur = cur;
    out->invalid = invalid;
    out->dof = dof;
    out->nis = nis;
    out->logdet = logdet;
}
// landmark i's camera-frame point estimate p = Q^-1 q0 from a landmark buffer (eqf_batch_state_estimate's expression)
__device__ __forceinline__ V3 batch_point_estimate(const double* lm, int i) {
    const int L = BATCH_L;
    return (1.0 / lm[BATCH_QA * L + i]) * q_rot(q_inv(ldq(lm + BATCH_QQ * L, L, i)), ld3(lm, L, i));
}

// Both kernels have one body, eqf_batch_frame_body.inc: k_batch_frame all of it, k_batch_frame_tail phases 2 - 5 (eqf_batch_step_accurate, below).
__global__ void __launch_bounds__(BATCH_T, 2) k_batch_frame(const BatchArgs ba) {
#define EQF_BATCH_FRAME_TAIL 0
#include "eqf_batch_frame_body.inc"
#undef EQF_BATCH_FRAME_TAIL
}
__global__ void __launch_bounds__(BATCH_T, 2) k_batch_frame_tail(const BatchArgs ba) {
#define EQF_BATCH_FRAME_TAIL 1
#include "eqf_batch_frame_body.inc"
#undef EQF_BATCH_FRAME_TAIL
}

// ===================================================================================================
// The Normal chart (eqf_batch_set_slot_chart, include/eqf_batch.h; coordinateSuite/normal.cpp). A Normal slot's Sigma is expressed in Normal coordinates; its
// Riccati step is the Euclidean step between two congruences with the block-diagonal change of coordinates M (eqf_math.hpp, normal_M; eqf_kernels.hpp,
// NormalM / normal_row), as riccati_open / riccati_close do on the context path:
//   Sigma' = M [ F_e (M^-1 Sigma M^-T) F_e^T + noise_e ] M^T + dt P.
// M depends on xi0 alone - the sensor block on its velocity and camera offset, which the host supplies in the slot's BatchNormalIn as normal_congruence does,
// a landmark's 3 x 3 block on its origin point q0 - and so is constant over a frame's propagation. Phases 2 - 5 of the frame need nothing new: measure_one,
// outlier_stats_body, lift_load / lift_landmark and store_chart_constants carry the Normal chart through in.ss.chart, as they do for a context.
struct BatchNormalIn {
    NormalM inv; // dir -1: M^-1
    NormalM fwd; // dir +1: M; k_batch_normal adds fwd.dtP on the diagonal (addP), the per-sample kernels add their noise in Euclidean coordinates (addP 0)
};
// Row i of T = M (nm.dir > 0) or M^-1, in normal_row's form (indices and coefficients, at most 7): a landmark row from the slot's table sM (LDS: T's 3 x 3 block of landmark l, row-major, at 9 l)
__device__ __forceinline__ int batch_normal_row(const NormalM& nm, const double* sM, int i, int (&idx)[7], double (&co)[7]) {
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        idx[k] = 0;
        co[k] = 0.0;
    }
    if (i < 21) { // normal_row's sensor rows, with every index of idx / co a constant (registers, no private memory)
        const double sg = nm.dir > 0 ? 1.0 : -1.0;
        idx[0] = i;
        co[0] = 1.0;
        if (i < 12)
            return 1;
        if (i < 15) { // [12:15, 6:9] = -skew(v0) (inverse: +skew(v0))
            const V3 r = row(skew(V3{nm.v0[0], nm.v0[1], nm.v0[2]}), i - 12);
            idx[1] = 6, idx[2] = 7, idx[3] = 8;
            co[1] = -sg * r.x, co[2] = -sg * r.y, co[3] = -sg * r.z;
            return 4;
        }
        const double* ad = nm.Ad + 6 * (i - 15); // [15:21, 6:12] = Ad(T0^-1) (inverse: -Ad(T0^-1))
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            idx[1 + c] = 6 + c;
            co[1 + c] = sg * ad[c];
        }
        return 7;
    }
    const int l = (i - 21) / 3, r = (i - 21) % 3;
    idx[0] = 21 + 3 * l, idx[1] = idx[0] + 1, idx[2] = idx[0] + 2;
    co[0] = sM[9 * l + 3 * r], co[1] = sM[9 * l + 3 * r + 1], co[2] = sM[9 * l + 3 * r + 2];
    return 3;
}
// The landmarks' blocks of M (sMf) and M^-1 (sMi) into LDS: landmark i's origin point is entry (map ? map[i] : i) of the planes
__device__ __forceinline__ void batch_normal_tables(const double* planes, const int* map, int Ns, double* sMf, double* sMi) {
    for (int i = threadIdx.x; i < Ns; i += BATCH_T) {
        const V3 p0 = ld3(planes, BATCH_L, map ? map[i] : i);
        const M3 Mf = normal_M(p0), Mi = normal_Minv(p0);
        const double f[9] = {Mf.a00, Mf.a01, Mf.a02, Mf.a10, Mf.a11, Mf.a12, Mf.a20, Mf.a21, Mf.a22};
        const double v[9] = {Mi.a00, Mi.a01, Mi.a02, Mi.a10, Mi.a11, Mi.a12, Mi.a20, Mi.a21, Mi.a22};
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            sMf[9 * i + e] = f[e];
            sMi[9 * i + e] = v[e];
        }
    }
}
// dst (n1 x n1: lower half, mirrored, so that Sigma stays exactly symmetric) = T src[g, g] T^T, plus nm.dtP on the diagonal when nm.addP; T and sM as in
// batch_normal_row, g = gidx (LDS). dst and src are different buffers. k_congruence_normal's sums, inside the slot's workgroup.
__device__ __forceinline__ void batch_normal_congruence(const NormalM& nm, const double* sM, int n1, int ld, const double* src, const int* gidx, double* dst) {
    for (int t = threadIdx.x; t < n1 * n1; t += BATCH_T) {
        const int i = t % n1, j = t / n1;
        if (i < j)
            continue;
        int ii[7], jj[7];
        double ci[7], cj[7];
        const int ni = batch_normal_row(nm, sM, i, ii, ci), nj = batch_normal_row(nm, sM, j, jj, cj);
        double acc = 0.0;
#pragma unroll
        for (int b = 0; b < 7; ++b) {
            if (b < nj) {
                const double* col = src + (size_t)gidx[jj[b]] * ld;
                double s = 0.0;
#pragma unroll
                for (int a = 0; a < 7; ++a)
                    if (a < ni)
                        s = fma(ci[a], col[gidx[ii[a]]], s);
                acc = fma(cj[b], s, acc);
            }
        }
        if (nm.addP && i == j)
            acc += nm.dtP[i < 21 ? i / 3 : 7];
        dst[i + (size_t)j * ld] = acc;
        dst[j + (size_t)i * ld] = acc;
    }
}
// The process noise of a Normal slot in Euclidean coordinates, M^-1 P M^-T (block diagonal like M), for the per-sample kernels: the 21 x 21 sensor block
// (row-major) at pe, the landmarks' 3 x 3 blocks behind it (9 per landmark, at 441 + 9 l). nm = the slot's M^-1, sMi its landmark table, Pd the eight variances.
constexpr int BATCH_NORMAL_PE = 441 + 9 * BATCH_L;
static_assert(BATCH_NORMAL_PE <= 16 * BATCH_L, "M^-1 P M^-T fits into the statistics rows of the slot's scratch area");
__device__ __forceinline__ void batch_normal_noise(const NormalM& nm, const double* sMi, int Ns, const double* Pd, double* pe) {
    for (int t = threadIdx.x; t < 441; t += BATCH_T) {
        const int r = t / 21, c = t % 21;
        int ii[7], jj[7];
        double ci[7], cj[7];
        const int ni = batch_normal_row(nm, sMi, r, ii, ci), nj = batch_normal_row(nm, sMi, c, jj, cj);
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int b = 0; b < 7; ++b)
                if (a < ni && b < nj && ii[a] == jj[b])
                    acc += ci[a] * cj[b] * Pd[ii[a] / 3];
        pe[t] = acc;
    }
    for (int t = threadIdx.x; t < 9 * Ns; t += BATCH_T) {
        const int l = t / 9, a = (t % 9) / 3, b = t % 3;
        const double* m = sMi + 9 * l;
        pe[441 + t] = Pd[7] * (m[3 * a] * m[3 * b] + m[3 * a + 1] * m[3 * b + 1] + m[3 * a + 2] * m[3 * b + 2]);
    }
}
// entry (r, c), r >= c, of that noise
__device__ __forceinline__ double batch_normal_noise_at(const double* pe, int r, int c) {
    if (r < 21)
        return pe[r * 21 + c];
    if (c < 21 || (r - 21) / 3 != (c - 21) / 3)
        return 0.0;
    return pe[441 + 9 * ((r - 21) / 3) + 3 * ((r - 21) % 3) + (c - 21) % 3];
}

// eqf_batch_step of the Normal slots: what phases 0 and 1 of k_batch_frame do for the other charts, followed by k_batch_frame_tail on the same stream, as
// k_batch_riccati / k_batch_discrete are. A kernel of its own and not another shape of the frame body: k_batch_frame keeps its text (eqf_batch_frame_body.inc).
//   0  as k_batch_frame's phase 0, with the rows assemble_landmark gives for the Euclidean chart, kept as dt A_e (the entries of F_e - I, as the reference's
//      I + dt A has them: a Sigma with entries near the largest double does not overflow in a sum that dt would have scaled down afterwards); the landmarks'
//      blocks of M and M^-1 into LDS, behind the rows
//      (the region the update's S needs anyway: BATCH_SM doubles, k_batch_frame's footprint);
//   a  Sigma_e = M^-1 Sigma[g, g] M^-T, gathered through the surviving rows, into the other Sigma buffer;
//   b  G = F_e Sigma_e into the scratch area;
//   c  G F_e^T + dt B_e Q B_e^T (no P) into the current Sigma buffer, whose contents step a has finished with - phase 3 of the tail overwrites it in any case;
//   d  Sigma' = M ( . ) M^T + dt P into the other Sigma buffer: where k_batch_frame_tail expects the propagated Sigma.
static_assert(BATCH_SM_PROP + 20 + 18 * BATCH_L <= BATCH_SM, "the landmarks' blocks of M and M^-1 sit behind the propagation rows and the slot's Qd / Pd");
__global__ void __launch_bounds__(BATCH_T, 2) k_batch_normal(const BatchArgs ba, const BatchNormalIn* nrm) {
    __shared__ double sm[BATCH_SM];
    __shared__ int s_gidx[BATCH_NMAX];
    __shared__ int s_surv[BATCH_L];
    const BatchIn& in = ba.in[blockIdx.x];
    const BatchNormalIn& nb = nrm[blockIdx.x];
    const int tid = threadIdx.x;
    const int L = BATCH_L, ld = ba.buf.ld;
    const int slot = in.slot, cur = in.cur, nxt = cur ^ 1;
    double* S0 = ba.buf.sig_of(slot, cur);
    double* S1 = ba.buf.sig_of(slot, nxt);
    const double* L0 = ba.buf.lm_of(slot, cur);
    double* L1 = ba.buf.lm_of(slot, nxt);
    double* G = ba.buf.scr_of(slot);
    const int Ns = in.Ns, n1 = 21 + 3 * Ns;
    const double dt = in.dt;
    double* Ass = sm;
    double* Bs = sm + 441;
    double* lm66 = sm + 693;
    double* Al = sm + 759;
    double* Bl = Al + BATCH_L * 45;
    double* Qd = sm + BATCH_SM_PROP;
    double* sMf = Qd + 20;
    double* sMi = sMf + 9 * BATCH_L;
    if (tid < 12)
        Qd[tid] = in.ss.Qd[tid];
    for (int t = tid; t < 441; t += BATCH_T)
        Ass[t] = dt * sensor_Ass_entry(in.ck, t); // dt A_e: F_e = I + dt A_e entry by entry, as the reference forms it
    for (int t = tid; t < 252; t += BATCH_T)
        Bs[t] = sensor_Bs_entry(in.ck, t);
    for (int t = tid; t < 66; t += BATCH_T)
        lm66[t] = in.ck.lm[t];
    for (int t = tid; t < Ns; t += BATCH_T)
        s_surv[t] = in.surv[t];
    __syncthreads();
    for (int r = tid; r < n1; r += BATCH_T)
        s_gidx[r] = r < 21 ? r : 21 + 3 * s_surv[(r - 21) / 3] + (r - 21) % 3;
    batch_normal_tables(L0, s_surv, Ns, sMf, sMi);
    {
        // k_batch_frame's split: waves 0 / 1 / 2 the three column parts of a landmark's rows of A_e and B_e, wave 3 its planes and the observer steps
        const int wave = tid >> 6, i = tid & 63;
        if (i < Ns) {
            const int o = s_surv[i];
            const V3 p0 = ld3(L0, L, o);
            Qt q = ldq(L0 + BATCH_QQ * L, L, o);
            double a = L0[BATCH_QA * L + o];
            if (wave < 3) {
                double al[45], bl[9];
                if (wave == 0) {
                    assemble_landmark<0>(lm66, EQVIO_COORD_EUCLIDEAN, p0, q, a, M3{}, M3{}, al, bl);
                    for (int r = 0; r < 3; ++r)
                        for (int c = 0; c < 6; ++c)
                            Al[i * 45 + r * 15 + c] = dt * al[r * 15 + c];
                    for (int e = 0; e < 9; ++e)
                        Bl[i * 9 + e] = bl[e];
                } else if (wave == 1) {
                    assemble_landmark<1>(lm66, EQVIO_COORD_EUCLIDEAN, p0, q, a, M3{}, M3{}, al, bl);
                    for (int r = 0; r < 3; ++r)
                        for (int c = 6; c < 12; ++c)
                            Al[i * 45 + r * 15 + c] = dt * al[r * 15 + c];
                } else {
                    assemble_landmark<2>(lm66, EQVIO_COORD_EUCLIDEAN, p0, q, a, M3{}, M3{}, al, bl);
                    for (int r = 0; r < 3; ++r)
                        for (int c = 12; c < 15; ++c)
                            Al[i * 45 + r * 15 + c] = dt * al[r * 15 + c];
                }
            } else {
                for (int pl = 0; pl < BATCH_QQ; ++pl)
                    L1[pl * L + i] = L0[pl * L + o];
                if (in.k > 0)
                    observer_chain(ba.steps + in.obs_off, in.k, p0, q, a);
                L1[BATCH_QQ * L + i] = q.w;
                L1[(BATCH_QQ + 1) * L + i] = q.x;
                L1[(BATCH_QQ + 2) * L + i] = q.y;
                L1[(BATCH_QQ + 3) * L + i] = q.z;
                L1[BATCH_QA * L + i] = a;
            }
        }
    }
    __syncthreads();
    // ---- a: into Euclidean coordinates
    batch_normal_congruence(nb.inv, sMi, n1, ld, S0, s_gidx, S1);
    __syncthreads();
    for (int r = tid; r < n1; r += BATCH_T)
        s_gidx[r] = r;
    // ---- b, c: k_batch_frame's phase 1 on Sigma_e, without P
    auto f_row = [&](int r, auto v) -> double {
        double acc = 0.0;
        if (r < 21) {
            for (int k = 0; k < 21; ++k)
                acc += Ass[r * 21 + k] * v(k);
        } else {
            const int i = (r - 21) / 3, a = (r - 21) % 3;
            const double* row = Al + i * 45 + a * 15;
            for (int e = 0; e < 12; ++e)
                acc += row[e] * v(al_col(e));
            for (int b = 0; b < 3; ++b)
                acc += row[12 + b] * v(21 + 3 * i + b);
        }
        return v(r) + acc;
    };
    auto b_entry = [&](int r, int e) -> double {
        if (r < 21)
            return Bs[r * 12 + e];
        const int i = (r - 21) / 3, a = (r - 21) % 3;
        return e < 3 ? Bl[i * 9 + a * 3 + e] : 0.0;
    };
    for (int t = tid; t < n1 * n1; t += BATCH_T) {
        const int r = t % n1, c = t / n1;
        const double* col = S1 + (size_t)c * ld;
        G[r + (size_t)c * ld] = f_row(r, [&](int k) { return col[k]; });
    }
    __syncthreads();
    for (int t = tid; t < n1 * n1; t += BATCH_T) {
        const int r = t % n1, c = t / n1;
        if (r < c)
            continue;
        double v = f_row(c, [&](int k) { return G[r + (size_t)k * ld]; });
        double nz = 0.0;
        for (int e = 0; e < 12; ++e)
            nz += b_entry(r, e) * Qd[e] * b_entry(c, e);
        v += dt * nz;
        S0[r + (size_t)c * ld] = v;
        S0[c + (size_t)r * ld] = v;
    }
    __syncthreads();
    // ---- d: back into Normal coordinates, plus dt P
    batch_normal_congruence(nb.fwd, sMf, n1, ld, S0, s_gidx, S1);
}

// ===================================================================================================
// eqf_batch_step_accurate (include/eqf_batch.h): integrateUpToTime with fastRiccati == false (src/VIOFilter.cpp:160-178) - per IMU sample one
// integrateRiccatiStateAccurate (VIO_eqf.cpp:74-91) at the X the samples before it have produced, then that sample's observer step - as a kernel of its own in
// front of k_batch_frame_tail, on the same stream within the same round trip. It ends where phases 0 and 1 of k_batch_frame end: Sigma of the surviving
// landmarks (n1 x n1) in the slot's other Sigma buffer, their planes in the other landmark buffer.
//
// Per sample with dt > 0, Sigma <- Phi Sigma Phi^T + Phi_B (Q / dt) Phi_B^T + dt P with [Phi Phi_B] the top n rows of exp(dt [[A, B], [0, 0]]), by the
// structured scheme of k_expm_sensor / k_expm_landmarks (eqf_kernels.hpp), restated inside the slot's workgroup: the scaling 2^-s from the infinity norm of
// dt [A B], a Taylor series of degree EXPM_K of the scaled generator - the sensor part E (21 x 33) by the whole workgroup, then [Y_i | F_i] (3 x 33, 3 x 3) a
// wave per landmark -, then s squarings [[E, 0], [Y, F]]^2 = [[E^2, 0], [Y E + F Y, F^2]] with every landmark's Y, F and E in LDS, in lockstep. Phi's rows have
// the shape of the rows of F = I + dt A in k_batch_frame's phase 1, except that a landmark row carries all 21 sensor columns: G = Phi Sigma goes to the
// scratch area, Sigma' = G Phi^T + noise (lower half, mirrored) to the other Sigma buffer, which is also the next sample's source - the first sample gathers
// from the current buffer through the surviving rows. Without a sample of dt > 0 the gathered Sigma is copied, bit for bit.
// The LDS footprint (78 KB: E, the scaled generator, two Taylor temporaries, 64 x 108 doubles of Y / F) is why this is no instantiation of the frame body.
struct RicStep {
    double dt;
    CommonK ck; // sensor-level terms of A and B at the X this sample starts from
};
struct RicArgs {
    BatchBufs buf;
    const BatchIn* in;
    const ObsStep* steps;
    const RicStep* rsteps;
    BatchOut* out;
};
constexpr int RIC_EN = 21 * 33;                        // E, the scaled generator, a Taylor temporary
constexpr int RIC_SLOT = 3 * 33 + 9;                   // a landmark's Y and F; before its Taylor series, its rows of A (45) and B (9)
constexpr int RIC_SM = 4 * RIC_EN + 66 + BATCH_L * RIC_SLOT;
static_assert(4 * (3 * 33) <= RIC_EN, "the waves' staging rows fit into the sensor series' temporary");

// The kernel's body is eqf_batch_riccati_body.inc, included once per kernel like the frame's. k_batch_riccati_normal (the Normal slots): the same samples in
// Euclidean coordinates between the two congruences. Before the first sample Sigma_e = M^-1 Sigma[g, g] M^-T goes to the other buffer in the gather's place; every
// sample works with the rows assemble_landmark gives for the Euclidean chart and adds dt M^-1 P M^-T (batch_normal_noise, kept in the statistics rows of the
// scratch area, which nothing reads before k_batch_frame_tail writes them) where the other charts add dt P; behind the last sample Sigma' = M Sigma_e M^T goes
// through the scratch area back to the other buffer. The landmark tables of M and M^-1 use the kernel's LDS while no sample does. Without a sample of dt > 0
// there is no congruence either: the gathered Sigma, bit for bit.
__global__ void __launch_bounds__(BATCH_T, 2) k_batch_riccati(const RicArgs ra) {
#define EQF_BATCH_NORMAL 0
#include "eqf_batch_riccati_body.inc"
#undef EQF_BATCH_NORMAL
}
__global__ void __launch_bounds__(BATCH_T, 2) k_batch_riccati_normal(const RicArgs ra, const BatchNormalIn* nrm) {
#define EQF_BATCH_NORMAL 1
#include "eqf_batch_riccati_body.inc"
#undef EQF_BATCH_NORMAL
}

// ===================================================================================================
// eqf_batch_step_discrete (include/eqf_batch.h): integrateUpToTime with fastRiccati == false and useDiscreteStateMatrix == true (src/VIOFilter.cpp:165-170) - per
// IMU sample one integrateRiccatiStateDiscrete (VIO_eqf.cpp:93-103) at the X the samples before it have produced, then that sample's observer step. The sibling of
// k_batch_riccati: launched in its place in front of k_batch_frame_tail, it ends where that kernel ends and moves Sigma the same way (the first sample gathers
// from the current buffer through the surviving rows, every later one reads the other buffer; without a sample of dt > 0 the gathered Sigma is copied).
//
// Per sample with dt > 0, Sigma <- A_d Sigma A_d^T + dt (B Q B^T + P). A_d = stateMatrixADiscrete (EqFMatrices.cpp:24-41) is the central difference, h = cbrt(eps),
// of a0Discrete over the 21 sensor coordinates and the 3 coordinates of every landmark, and has the arrow shape of the accurate mode's Phi: a dense 21 x 21 sensor
// block, per landmark a 3 x 21 strip and a 3 x 3 block. All of it is formed here:
//   sensor part   lanes 0 .. 41 of wave 0 evaluate one perturbation each (coordinate lane / 2, +h for even lanes, -h for odd ones) by the chain of
//                 eqf_integrate_riccati_discrete's discrete_A (eqf_hip.hip), with the helpers that function calls: sensorChart^-1, sensor_action,
//                 lift_discrete_sensor, the group products, two se3_log. Each leaves its 21-vector and the camera-frame pose change cpc of its lift in LDS; lane 42
//                 leaves the nominal cpc. The pairs are then differenced into the sensor block.
//   landmark rows a lane per landmark, by k_discrete_A's device functions (a0_discrete_landmark, lift_q, chart_fwd / chart_bwd), from the 43 cpc and the landmark's
//                 current Q, which wave 3 carries through the observer steps as in k_batch_riccati. The 24 central differences of a landmark (21 sensor coordinates,
//                 its own 3) are split over the four waves, six each.
//   noise         B's sensor rows from sensor_Bs_entry, the landmarks' 3 x 3 from assemble_landmark<0>, as phase 1 of the fast frame forms dt (B Q B^T + P).
// The packet carries per sample dt and CommonK (for B) as RicStep does, the sample's 13 IMU doubles, and the sensor parts of xi0 and of the X the sample starts
// from: 1.6 KB, not the 6 KB of A_d pieces a host-side chain would send - and no 42 lift-and-log chains per sample and slot on the host's one thread.
// G = A_d Sigma goes to the scratch area and Sigma' = G A_d^T + noise (lower half, mirrored) to the other buffer on the VALU, as step (5) of k_batch_riccati does.
struct DiscStep {
    double dt;
    CommonK ck;       // sensor-level terms of B at the X this sample starts from
    double imu[13];   // the sample
    GroupSensor X;    // sensor part of X at the sample's start
    SensorState xi0;  // the slot's origin (the same in every sample of a frame: it rides here so that the frame packet BatchIn stays what the other kernels read)
};
struct DiscArgs {
    BatchBufs buf;
    const BatchIn* in;
    const ObsStep* steps;
    const DiscStep* dsteps;
    BatchOut* out;
};
// Measurement switch, 0 in every build that ships: -DEQF_DISC_MEASURE_SKIP=1 builds k_batch_discrete without the two passes over Sigma (G = A_d Sigma and
// Sigma' = G A_d^T + noise), so that a kernel trace of that build shows what forming A_d and B costs on its own. For attributing the kernel's time only
// (profiles/r21_batch_discrete_kernel_stats.txt): the build's results mean nothing.
#ifndef EQF_DISC_MEASURE_SKIP
#define EQF_DISC_MEASURE_SKIP 0
#endif
constexpr int DISC_ROW = 24;                 // a landmark row of A_d: 21 sensor columns, its own 3
constexpr int DISC_SLOT = 3 * DISC_ROW + 9;  // a landmark's rows of A_d and its 3 x 3 of B
constexpr int DISC_NPERT = 42;               // perturbed evaluations of the sensor chain
constexpr int DISC_SM = 441 + 252 + 66 + DISC_NPERT * 21 + BATCH_L * DISC_SLOT;

// One evaluation of a0Discrete's sensor part (EqFMatrices.cpp:24-41) by one lane of k_batch_discrete: lane 42 the nominal one - it leaves cpc[0], the camera-frame
// pose change of liftVelocityDiscrete(xi_hat) -, lane 2 j + s < 42 the one with sensor coordinate j moved by +h (s = 0) or -h (s = 1), which leaves its cpc and its
// 21-vector epsilon_1. The chain is eqf_integrate_riccati_discrete's discrete_A (eqf_hip.hip), term for term. A function of its own (noinline): its 46-double
// states are live only here, not across the kernel. The order keeps few of them live at once: Lambda_hat^-1, then xi_e and its lift, then the products.
// (VARIANT: one copy per kernel that calls it - the kernel's EQF_BATCH_NORMAL -, so that each kernel is compiled with a callee of its own, as k_batch_discrete
// was when it was the only caller.)
template <int VARIANT> __device__ __attribute__((noinline)) void disc_sensor_eval(const DiscStep& ds, int lane, double h, double* sCol, Pose* cpc) {
    const double dt = ds.dt;
    const SensorState xhat = sensor_action(ds.X, ds.xi0);
    const GroupSensor Lh = lift_discrete_sensor(xhat, ds.imu, dt);
    if (lane == DISC_NPERT) {
        cpc[0] = pose_mul(pose_mul(pose_inv(xhat.cam), pose_inv(Lh.A)), xhat.cam);
        return;
    }
    const GroupSensor Lh_inv = group_inv(Lh);
    const int j = lane >> 1;
    const double hh = (lane & 1) ? -h : h;
    // block b of the perturbation e = +-h e_j (named scalars: no array indexed at run time)
    const auto eb = [&](int b) { return v3(j == 3 * b ? hh : 0.0, j == 3 * b + 1 ? hh : 0.0, j == 3 * b + 2 ? hh : 0.0); };
    // xi_e = sensorChart_std.inv(e, xi0) (VIOState.cpp:114-121)
    SensorState se;
    se.bgyr = ds.xi0.bgyr + eb(0);
    se.bacc = ds.xi0.bacc + eb(1);
    se.pose = pose_mul(ds.xi0.pose, se3_exp(eb(2), eb(3)));
    se.vel = ds.xi0.vel + eb(4);
    se.cam = pose_mul(ds.xi0.cam, se3_exp(eb(5), eb(6)));
    GroupSensor T;
    {
        const SensorState xs = sensor_action(ds.X, se);
        const GroupSensor Lp = lift_discrete_sensor(xs, ds.imu, dt);
        cpc[1 + lane] = pose_mul(pose_mul(pose_inv(xs.cam), pose_inv(Lp.A)), xs.cam);
        T = group_mul(Lp, Lh_inv);
    }
    const GroupSensor Gp = group_mul(group_mul(ds.X, T), group_inv(ds.X));
    const SensorState s1 = sensor_action(Gp, se);
    V3 om, tr, omc, trc;
    se3_log(pose_mul(pose_inv(ds.xi0.pose), s1.pose), om, tr);
    se3_log(pose_mul(pose_inv(ds.xi0.cam), s1.cam), omc, trc);
    double* col = sCol + lane * 21;
    const V3 parts[7] = {s1.bgyr - ds.xi0.bgyr, s1.bacc - ds.xi0.bacc, om, tr, s1.vel - ds.xi0.vel, omc, trc};
    for (int b = 0; b < 7; ++b) {
        col[3 * b] = parts[b].x;
        col[3 * b + 1] = parts[b].y;
        col[3 * b + 2] = parts[b].z;
    }
}

// The kernel's body is eqf_batch_discrete_body.inc, included once per kernel. k_batch_discrete_normal (the Normal slots): as k_batch_riccati_normal - A_d under
// the Normal chart is M A_d,e M^-1, as on the context path (the reference differentiates in Normal coordinates; the two agree to the differencing's own noise),
// so A_d,e and B_e are formed for the Euclidean chart and the samples run between the two congruences, with dt M^-1 P M^-T in dt P's place.
__global__ void __launch_bounds__(BATCH_T, 2) k_batch_discrete(const DiscArgs da) {
#define EQF_BATCH_NORMAL 0
#include "eqf_batch_discrete_body.inc"
#undef EQF_BATCH_NORMAL
}
__global__ void __launch_bounds__(BATCH_T, 2) k_batch_discrete_normal(const DiscArgs da, const BatchNormalIn* nrm) {
#define EQF_BATCH_NORMAL 1
#include "eqf_batch_discrete_body.inc"
#undef EQF_BATCH_NORMAL
}

// ===================================================================================================
// eqf_batch_nees and eqf_batch_augment (include/eqf_batch.h): one workgroup per entry, each touching its own slot only.
// The scratch area holds nothing live between launches: k_batch_frame writes every scratch word before it reads it in the same launch (G in phase 1, the
// statistics rows in phase 2, T / W and L in phase 4, the lift estimates over the statistics rows), so k_batch_nees may use it freely. k_batch_nees writes
// nothing else; k_batch_augment writes the slot's other buffer pair, which the host then names current.

// computeNEES (VIO_eqf.cpp:153-170): eps = stateChart(stateError); NEES = eps^T Sigma^-1 eps / n. The host gives the 21 sensor entries and the true point of
// every state landmark in state order; the landmark entries (pe = a R p, point_chart against q0) are computed here.
struct NeesIn {
    int slot, cur, N;
    int chart; // the slot's chart
    double eps[21];
    double p[3 * BATCH_L];
};
struct NeesOut {
    double sumsq; // eps^T Sigma^-1 eps
    int lu;       // 1: a pivot was <= 0 and the partial-pivot elimination gave the value
};
struct NeesArgs {
    BatchBufs buf;
    const NeesIn* in;
    NeesOut* out;
};
constexpr int NEES_PW = 16;  // panel width
constexpr int NEES_PLD = 228; // LDS panel column stride: rows k0 .. np (<= 215) and the zero rows of the last 16-row tile (< 224)
constexpr int NEES_NP = BATCH_NMAX + 1;

// sum over the workgroup; every thread gets it (s_red: BATCH_T / 64 doubles)
__device__ __forceinline__ double nees_block_sum(double v, double* s_red) {
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0)
        s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < BATCH_T / 64; ++w)
        t += s_red[w];
    __syncthreads();
    return t;
}

// Z = [Sigma ; eps^T] in the slot's scratch area (np + 1 rows, leading dimension ld >= 216 > np + 1, np columns: ld * 214 <= batch_scr_doubles(ld)), Sigma padded
// to the even dimension np with a unit diagonal entry as the context path's k_build_nees does. lower: only r >= c (the Cholesky reads no more).
__device__ __forceinline__ void nees_build_z(int n, int np, int ld, const double* S, const double* eps, double* Z, bool lower) {
    for (int t = threadIdx.x; t < (np + 1) * np; t += BATCH_T) {
        const int r = t % (np + 1), c = t / (np + 1);
        if (lower && r < c)
            continue;
        Z[r + (size_t)c * ld] = r == np ? eps[c] : (r < n && c < n ? S[r + (size_t)c * ld] : (r == c ? 1.0 : 0.0));
    }
}

// ---- the consistency record (eqf_batch_consistency, include/eqf_batch.h): what k_batch_consistency adds to the NEES of an entry
// Rows of eps / Sigma of block k (EQF_BLOCK_*): first row and size
__device__ __forceinline__ int cons_block_row(int k) { return k == 0 ? 0 : k == 1 ? 6 : k == 2 ? 9 : k == 3 ? 6 : k == 4 ? 12 : k == 5 ? 15 : 0; }
__device__ __forceinline__ int cons_block_dim(int k) { return k == 0 || k == 3 || k == 5 ? 6 : k == 6 ? 21 : 3; }
// LDS layout of the block forms, in the panel region P before the factorisation uses it (doubles): the sensor block of Sigma (21 x 21, M[i][j] at 21 i + j), the
// wave's working copy [M | x] of the 21-row block (row stride 22) with its solution behind it, one workspace per small block and one per landmark
constexpr int CONS_S21 = 0, CONS_W21 = 448, CONS_Y21 = CONS_W21 + 21 * 22, CONS_SMALL = 944, CONS_SMALL_W = 6 * 7 + 12, CONS_LM = CONS_SMALL + 6 * CONS_SMALL_W,
              CONS_LM_W = 3 * 4 + 6, CONS_END = CONS_LM + BATCH_L * CONS_LM_W;
static_assert(CONS_Y21 + 21 <= CONS_SMALL && 441 <= CONS_W21, "the block forms' LDS regions are disjoint");

// Measurement switch, 0 in every build that ships: -DEQF_CONS_MEASURE_SKIP=1 builds k_batch_consistency without the block forms (block[] and lm_quad stay
// unwritten), =2 without the stores of eps and of the diagonal of Sigma. For attributing the kernel's time only (profiles/r13_batch_consistency_breakdown.txt).
#ifndef EQF_CONS_MEASURE_SKIP
#define EQF_CONS_MEASURE_SKIP 0
#endif

// x^T M^-1 x by the elimination rule of VIOWriter.cpp's quadInv (the reference's .inverse() route): Gaussian elimination with partial pivoting on [M | x], the
// pivot the first row of largest magnitude, back substitution, then x^T y. One lane; w: K rows of [M | x] (row stride K + 1, destroyed), then K doubles that
// hold x and K that receive y. A zero pivot gives a non-finite value, which is returned as it is.
__device__ __forceinline__ double cons_quad_inv_lane(double* w, int K) {
    const int st = K + 1;
    double* x0 = w + K * st;
    double* y = x0 + K;
    for (int i = 0; i < K; ++i)
        x0[i] = w[i * st + K];
    for (int c = 0; c < K; ++c) {
        int p = c;
        for (int r = c + 1; r < K; ++r)
            if (fabs(w[r * st + c]) > fabs(w[p * st + c]))
                p = r;
        if (p != c)
            for (int j = 0; j <= K; ++j) {
                const double t = w[p * st + j];
                w[p * st + j] = w[c * st + j];
                w[c * st + j] = t;
            }
        for (int r = c + 1; r < K; ++r) {
            const double f = w[r * st + c] / w[c * st + c];
            for (int j = c; j <= K; ++j)
                w[r * st + j] -= f * w[c * st + j];
        }
    }
    for (int i = K - 1; i >= 0; --i) {
        double s = w[i * st + K];
        for (int j = i + 1; j < K; ++j)
            s -= w[i * st + j] * y[j];
        y[i] = s / w[i * st + i];
    }
    double q = 0.0;
    for (int i = 0; i < K; ++i)
        q += x0[i] * y[i];
    return q;
}

// The same rule for the 21-row sensor block by one wave: lane r owns row r of [M | x] (w, row stride 22, destroyed; x: the 21 sensor entries of eps; y: 21
// doubles). Per column: the pivot search across the wave (largest |a[r][c]|, the first such row), the row swap by lanes 0 .. 21, the elimination one lane per
// row; lane 0 then does the back substitution and x^T y in quadInv's order. Every lane returns the value.
__device__ __forceinline__ double cons_quad_inv_wave21(double* w, const double* x, double* y, int lane) {
    constexpr int K = 21, st = K + 1;
    for (int c = 0; c < K; ++c) {
        double v = (lane >= c && lane < K) ? fabs(w[lane * st + c]) : -1.0;
        int p = lane;
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(v, o, 64);
            const int op = __shfl_xor(p, o, 64);
            if (ov > v || (ov == v && op < p)) {
                v = ov;
                p = op;
            }
        }
        p = __shfl(p, 0, 64);
        p = (p >= c && p < K) ? p : c; // a column of NaN leaves no order: any row of the range, the same in every lane
        if (p != c && lane <= K) {
            const double t = w[p * st + lane];
            w[p * st + lane] = w[c * st + lane];
            w[c * st + lane] = t;
        }
        batch_wave_sync();
        if (lane > c && lane < K) {
            const double f = w[lane * st + c] / w[c * st + c];
            for (int j = c; j <= K; ++j)
                w[lane * st + j] -= f * w[c * st + j];
        }
        batch_wave_sync();
    }
    double q = 0.0;
    if (lane == 0) {
        for (int i = K - 1; i >= 0; --i) {
            double s = w[i * st + K];
            for (int j = i + 1; j < K; ++j)
                s -= w[i * st + j] * y[j];
            y[i] = s / w[i * st + i];
        }
        for (int i = 0; i < K; ++i)
            q += x[i] * y[i];
    }
    return __shfl(q, 0, 64);
}

// Blocked right-looking Cholesky of Z = [Sigma ; eps^T] with the eps row carried along as an extra row: after the factorisation that row holds z = L^-1 eps,
// and |z|^2 = eps^T Sigma^-1 eps. Per 16-column panel: rows k0 .. np of the panel into LDS, the panel factored on the VALU (one lane per row), the eps row's
// entries summed, and the trailing lower triangle (the eps row included) updated by Z -= L21 L21^T in 16 x 16 tiles on the matrix cores (mfma16_nt, one wave
// per tile, operands from LDS). A pivot <= 0 (or not finite) sends the slot to partial-pivot Gaussian elimination on [Sigma | eps], in the same workgroup: what
// k_ge_step / k_ge_back do over np launches in the context path, so a number comes back whenever the reference's Sigma.inverse() gives one.
//
// REC (k_batch_consistency): the same front half and the same factorisation, and between them the rest of the entry's consistency record - the seven block
// forms and the landmarks' 3 x 3 forms by quadInv's rule, the landmarks' point errors, eps and the diagonal of Sigma - written to rec with plain stores. The
// block forms work in the panel region before the first panel is loaded, so the LDS footprint is k_batch_nees's. eps^T Sigma^-1 eps and the fallback flag then go
// to rec->nees / rec->lu instead of na.out. Nothing of the arithmetic that leads to them depends on REC.
template <bool REC> __device__ __forceinline__ void batch_nees_body(const NeesArgs& na, eqf_batch_consistency_record* rec) {
    static_assert(CONS_END <= NEES_PLD * NEES_PW, "the block forms fit into the panel region");
    __shared__ double P[NEES_PLD * NEES_PW]; // the panel; x of the back substitution in the fallback
    __shared__ double s_eps[NEES_NP + 1];
    __shared__ double s_red[BATCH_T];
    __shared__ int s_idx[BATCH_T];
    __shared__ int s_perm[NEES_NP];
    const NeesIn& in = na.in[blockIdx.x];
    const int tid = threadIdx.x, L = BATCH_L, ld = na.buf.ld;
    const int N = in.N, n = 21 + 3 * N, np = n + (n & 1);
    const double* S = na.buf.sig_of(in.slot, in.cur);
    const double* lm = na.buf.lm_of(in.slot, in.cur);
    double* Z = na.buf.scr_of(in.slot);

    for (int r = tid; r < np; r += BATCH_T)
        if (r < 21 || r >= n)
            s_eps[r] = r < 21 ? in.eps[r] : 0.0;
    if (tid < N) {
        const int i = tid;
        const V3 pe = lm[BATCH_QA * L + i] * q_rot(ldq(lm + BATCH_QQ * L, L, i), V3{in.p[3 * i], in.p[3 * i + 1], in.p[3 * i + 2]}); // (Q_i^-1)^-1 p = a R p
        const V3 e = chart_fwd(in.chart, pe, ld3(lm, L, i)); // pointChart of the slot's chart (normal_chart under Normal)
        s_eps[21 + 3 * i] = e.x;
        s_eps[22 + 3 * i] = e.y;
        s_eps[23 + 3 * i] = e.z;
        if constexpr (REC) // |p_hat - p_true|
            rec->lm_err[i] = norm(batch_point_estimate(lm, i) - V3{in.p[3 * i], in.p[3 * i + 1], in.p[3 * i + 2]});
    }
    __syncthreads();
    if constexpr (REC) {
        for (int t = tid; t < 441; t += BATCH_T)
            P[CONS_S21 + t] = S[t / 21 + (size_t)(t % 21) * ld];
        __syncthreads();
        const int wave = tid >> 6, lane = tid & 63;
        if constexpr (EQF_CONS_MEASURE_SKIP & 1) {
        } else if (wave == 0) { // the 21-row block
            double* w = P + CONS_W21;
            for (int t = lane; t < 21 * 22; t += 64)
                w[t] = t % 22 < 21 ? P[CONS_S21 + 21 * (t / 22) + t % 22] : s_eps[t / 22];
            batch_wave_sync();
            const double q = cons_quad_inv_wave21(w, s_eps, P + CONS_Y21, lane);
            if (lane == 0)
                rec->block[EQF_BLOCK_SENSOR] = q;
        } else if (wave == 1) { // the six small blocks, one lane each
            if (lane < EQF_BLOCK_SENSOR) {
                const int r0 = cons_block_row(lane), K = cons_block_dim(lane);
                double* w = P + CONS_SMALL + lane * CONS_SMALL_W;
                for (int i = 0; i < K; ++i) {
                    for (int j = 0; j < K; ++j)
                        w[i * (K + 1) + j] = P[CONS_S21 + 21 * (r0 + i) + r0 + j];
                    w[i * (K + 1) + K] = s_eps[r0 + i];
                }
                rec->block[lane] = cons_quad_inv_lane(w, K);
            }
        } else if (wave == 2) { // the landmarks' 3 x 3 marginals, straight from Sigma
            if (lane < N) {
                const int r0 = 21 + 3 * lane;
                double* w = P + CONS_LM + lane * CONS_LM_W;
                for (int i = 0; i < 3; ++i) {
                    for (int j = 0; j < 3; ++j)
                        w[i * 4 + j] = S[(r0 + i) + (size_t)(r0 + j) * ld];
                    w[i * 4 + 3] = s_eps[r0 + i];
                }
                rec->lm_quad[lane] = cons_quad_inv_lane(w, 3);
            }
        }
        if constexpr (!(EQF_CONS_MEASURE_SKIP & 2))
            for (int r = tid; r < BATCH_NMAX; r += BATCH_T) {
                rec->eps[r] = r < n ? s_eps[r] : 0.0;
                rec->sigma_diag[r] = r < n ? S[r + (size_t)r * ld] : 0.0;
            }
        for (int i = N + tid; i < BATCH_L; i += BATCH_T) {
            rec->lm_quad[i] = 0.0;
            rec->lm_err[i] = 0.0;
        }
        if (tid == 0)
            rec->N = N;
    }
    nees_build_z(n, np, ld, S, s_eps, Z, true);
    __syncthreads();

    double acc = 0.0; // |z|^2, kept by thread 0
    bool fail = false;
    for (int k0 = 0; k0 < np && !fail; k0 += NEES_PW) {
        const int w = min(NEES_PW, np - k0), R = np + 1 - k0; // panel columns, rows (the last one is the eps row)
        for (int t = tid; t < NEES_PLD * NEES_PW; t += BATCH_T) {
            const int r = t % NEES_PLD, c = t / NEES_PLD;
            P[t] = (r < R && c < w && r >= c) ? Z[k0 + r + (size_t)(k0 + c) * ld] : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < w; ++j) {
            const double d = P[j + j * NEES_PLD]; // the same value in every lane: the exit is uniform
            if (!(d > 0.0) || !(d - d == 0.0)) {
                fail = true;
                break;
            }
            const double ljj = sqrt(d);
            for (int r = j + 1 + tid; r < R; r += BATCH_T)
                P[r + j * NEES_PLD] /= ljj;
            __syncthreads();
            for (int r = j + 1 + tid; r < R; r += BATCH_T) {
                const double lrj = P[r + j * NEES_PLD];
                for (int c = j + 1; c < w && c <= r; ++c)
                    P[r + c * NEES_PLD] -= lrj * P[c + j * NEES_PLD];
            }
            if (tid == 0)
                P[j + j * NEES_PLD] = ljj;
            __syncthreads();
        }
        if (fail)
            break;
        if (tid == 0)
            for (int c = 0; c < w; ++c)
                acc += P[(R - 1) + c * NEES_PLD] * P[(R - 1) + c * NEES_PLD];
        const int t0 = k0 + NEES_PW; // first trailing row and column
        if (t0 < np) {               // then w == 16: the product's K is the whole panel
            const int ntr = (np + 1 - t0 + 15) / 16, ntc = (np - t0 + 15) / 16, tri = ntc * (ntc + 1) / 2;
            const int ntiles = tri + (ntr > ntc ? ntc : 0);
            const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
            for (int t = wave; t < ntiles; t += BATCH_T / 64) {
                int bi, bj;
                if (t < tri) {
                    batch_tri_tile(t, bi, bj);
                } else {
                    bi = ntc;
                    bj = t - tri;
                }
                const d4 a = mfma16_nt(P + NEES_PW + 16 * bi, NEES_PLD, P + NEES_PW + 16 * bj, NEES_PLD);
                const int r = t0 + 16 * bi + lr;
                for (int q = 0; q < 4; ++q) {
                    const int c = t0 + 16 * bj + lk + 4 * q;
                    if (r <= np && c < np && r >= c)
                        Z[r + (size_t)c * ld] -= a[q];
                }
            }
        }
        __syncthreads();
    }
    if (!fail) {
        if (tid == 0) {
            if constexpr (REC) {
                rec->nees = acc;
                rec->lu = 0;
            } else {
                na.out[blockIdx.x].sumsq = acc;
                na.out[blockIdx.x].lu = 0;
            }
        }
        return;
    }

    // fallback: [Sigma | eps] read as rows M[i][j] = Z[j + i ld] (Sigma is symmetric; j = np is the right-hand side). Rows are never moved: s_perm maps
    // logical to physical rows. The pivot is the first row of largest |M[i][k]| (k_ge_step's rule).
    __syncthreads();
    nees_build_z(n, np, ld, S, s_eps, Z, false);
    for (int i = tid; i < np; i += BATCH_T)
        s_perm[i] = i;
    __syncthreads();
    for (int k = 0; k < np; ++k) {
        double best = -1.0;
        int bi = k;
        for (int i = k + tid; i < np; i += BATCH_T) {
            const double v = fabs(Z[k + (size_t)s_perm[i] * ld]);
            if (v > best) {
                best = v;
                bi = i;
            }
        }
        s_red[tid] = best;
        s_idx[tid] = bi;
        __syncthreads();
        for (int st = BATCH_T / 2; st > 0; st >>= 1) {
            if (tid < st) {
                const double o = s_red[tid + st];
                const int oi = s_idx[tid + st];
                if (o > s_red[tid] || (o == s_red[tid] && oi < s_idx[tid])) {
                    s_red[tid] = o;
                    s_idx[tid] = oi;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const int p = s_idx[0], t = s_perm[k];
            s_perm[k] = s_perm[p];
            s_perm[p] = t;
        }
        __syncthreads();
        const double* prow = Z + (size_t)s_perm[k] * ld;
        const double piv = prow[k];
        const int w = np - k; // columns k + 1 .. np
        for (int t = tid; t < (np - k - 1) * w; t += BATCH_T) {
            double* row = Z + (size_t)s_perm[k + 1 + t / w] * ld;
            const int j = k + 1 + t % w;
            const double l = row[k] / piv;
            row[j] -= l * prow[j];
        }
        __syncthreads();
    }
    // back substitution U x = b (x in P), then eps . x
    double* x = P;
    for (int k = np - 1; k >= 0; --k) {
        const double* row = Z + (size_t)s_perm[k] * ld;
        double s = 0.0;
        for (int j = k + 1 + tid; j < np; j += BATCH_T)
            s += row[j] * x[j];
        s = nees_block_sum(s, s_red);
        if (tid == 0)
            x[k] = (row[np] - s) / row[k];
        __syncthreads();
    }
    double s = 0.0;
    for (int j = tid; j < n; j += BATCH_T)
        s += s_eps[j] * x[j];
    s = nees_block_sum(s, s_red);
    if (tid == 0) {
        if constexpr (REC) {
            rec->nees = s;
            rec->lu = 1;
        } else {
            na.out[blockIdx.x].sumsq = s;
            na.out[blockIdx.x].lu = 1;
        }
    }
}
__global__ void __launch_bounds__(BATCH_T, 2) k_batch_nees(const NeesArgs na) { batch_nees_body<false>(na, nullptr); }
// eqf_batch_consistency: entry e's record at rec[e]; the host fills in the ids and divides the NEES by n
__global__ void __launch_bounds__(BATCH_T, 2) k_batch_consistency(const NeesArgs na, eqf_batch_consistency_record* rec) {
    batch_nees_body<true>(na, rec + blockIdx.x);
}

// augmentLandmarkStates (VIOFilter.cpp:112-132): removeOldLandmarks' compaction and addNewLandmarks (VIO_eqf.cpp:225-245), the two halves of k_batch_frame's
// phase 3 (kept landmarks by index; new ones with q0 = the provided point, its chart constants, Q = identity; Sigma with zero cross terms and
// initialPointVariance I), written into the slot's other buffer pair.
struct AugIn {
    int slot, cur, Nk, nnew; // landmarks kept, appended
    int keep[BATCH_L];       // state index of kept landmark i
    double p[3 * BATCH_L];   // provided point of the r-th appended landmark
    double init_var;         // the slot's initialPointVariance
};
struct AugArgs {
    BatchBufs buf;
    const AugIn* in;
};
__global__ void __launch_bounds__(BATCH_T) k_batch_augment(const AugArgs aa) {
    __shared__ int s_gidx[BATCH_NMAX];
    const AugIn& in = aa.in[blockIdx.x];
    const int tid = threadIdx.x, L = BATCH_L, ld = aa.buf.ld;
    const int nk = in.Nk, N2 = nk + in.nnew, n2 = 21 + 3 * N2, cur = in.cur, nxt = cur ^ 1;
    const double* S0 = aa.buf.sig_of(in.slot, cur);
    double* S1 = aa.buf.sig_of(in.slot, nxt);
    const double* L0 = aa.buf.lm_of(in.slot, cur);
    double* L1 = aa.buf.lm_of(in.slot, nxt);
    for (int r = tid; r < n2; r += BATCH_T)
        s_gidx[r] = r < 21 ? r : ((r - 21) / 3 < nk ? 21 + 3 * in.keep[(r - 21) / 3] + (r - 21) % 3 : -1);
    __syncthreads();
    batch_gather_sigma(S1, S0, s_gidx, n2, ld, in.init_var);
    if (tid < N2) {
        const int i = tid;
        if (i < nk) {
            for (int pl = 0; pl < BATCH_PLANES; ++pl)
                L1[pl * L + i] = L0[pl * L + in.keep[i]];
        } else {
            const int r = i - nk;
            batch_new_landmark(L1, i, in.p[3 * r], in.p[3 * r + 1], in.p[3 * r + 2]);
        }
    }
}

// eqf_batch_copy_slots (include/eqf_batch.h): entry e copies the live part of slot src's CURRENT buffer pair - the n x n of Sigma, n = 21 + 3 N, and the N live
// entries of the 35 landmark planes - into slot dst's OTHER pair, which the host then names current. No launch of the batch reads a slot's other pair before it
// has written it, so a copy never writes what this launch (or any entry of it) reads: a slot may be source and destination at once, and any mapping - fan-out,
// swap, cycle - goes in one launch. Nothing outside the live part is copied, because nothing outside it is ever read: k_batch_frame gathers Sigma through
// s_gidx and the planes through surv / s_keep (live indices only), k_batch_nees builds Z from r, c < n, k_batch_augment gathers through keep; the rows n .. ld and
// the plane entries N .. 64 are whatever the buffer held.
// Grid: x = entry, y = chunk of BATCH_COPY_COLS columns of Sigma (the last y also copies the planes); a block whose chunk starts at or behind column n has
// nothing to do. 16-byte loads and stores: ld is even and every buffer 16-byte aligned, so a column starts on a 16-byte boundary and its rows go in pairs; an odd
// n (or N) leaves one 8-byte element per column (plane). Blocks share nothing.
struct CopyIn {
    int src, scur; // source slot and its current pair
    int dst, dnxt; // destination slot and its other pair
    int N;         // the source's landmarks
};
struct CopyArgs {
    BatchBufs buf;
    const CopyIn* in;
};
constexpr int BATCH_COPY_COLS = 16;
constexpr int BATCH_COPY_CHUNKS = (BATCH_NMAX + BATCH_COPY_COLS - 1) / BATCH_COPY_COLS; // grid y
// the 16-byte accesses: every plane and every buffer of planes starts at an even number of doubles (eqf_batch_copy_slots checks ld and the Sigma stride)
static_assert(BATCH_L % 2 == 0 && (BATCH_PLANES * BATCH_L) % 2 == 0, "k_batch_copy moves pairs of doubles");
__global__ void __launch_bounds__(BATCH_T) k_batch_copy(const CopyArgs ca) {
    const CopyIn in = ca.in[blockIdx.x];
    const int tid = threadIdx.x, L = BATCH_L, ld = ca.buf.ld;
    const int N = in.N, n = 21 + 3 * N;
    const int c0 = blockIdx.y * BATCH_COPY_COLS, cols = min(BATCH_COPY_COLS, n - c0);
    if (cols > 0) {
        const double* S = ca.buf.sig_of(in.src, in.scur) + (size_t)c0 * ld;
        double* D = ca.buf.sig_of(in.dst, in.dnxt) + (size_t)c0 * ld;
        const int half = n >> 1; // >= 10
        for (int t = tid; t < cols * half; t += BATCH_T) {
            const size_t o = (size_t)(t / half) * ld + 2 * (t % half);
            *reinterpret_cast<double2*>(D + o) = *reinterpret_cast<const double2*>(S + o);
        }
        if ((n & 1) && tid < cols)
            D[(size_t)tid * ld + n - 1] = S[(size_t)tid * ld + n - 1];
    }
    if (blockIdx.y == gridDim.y - 1) {
        const double* S = ca.buf.lm_of(in.src, in.scur);
        double* D = ca.buf.lm_of(in.dst, in.dnxt);
        const int half = N >> 1; // 0 for N <= 1: the loop does not run
        for (int t = tid; t < BATCH_PLANES * half; t += BATCH_T) {
            const int o = (t / half) * L + 2 * (t % half);
            *reinterpret_cast<double2*>(D + o) = *reinterpret_cast<const double2*>(S + o);
        }
        if ((N & 1) && tid < BATCH_PLANES)
            D[tid * L + N - 1] = S[tid * L + N - 1];
    }
}

// eqf_batch_load_ctx / eqf_batch_store_ctx (include/eqf_batch.h): k_batch_copy's copy with a context (eqf_hip.h) on one side. The context keeps the same
// landmark planes in two arrays - q0 with its chart constants (30 planes), Qq and Qa (5 planes) - of plane stride Ncap, and Sigma with its own leading
// dimension; the slot's side is a BATCH_L-strided landmark buffer and a Sigma buffer of leading dimension buf.ld.
// TO_CTX false (load): entry e copies the context's current buffers into slot in[e].slot's pair in[e].which - the slot's OTHER pair, which the host then names
// current, so what the slot held (more rows, more landmarks, a stale pair) is never read again: k_batch_copy's argument. TO_CTX true (store): the one entry
// (ga.one; no packet) copies the slot's CURRENT pair into the context's current buffers, which eqf_set_state / eqf_set_sigma write in place as well.
// Grid and the Sigma chunks are k_batch_copy's: x = entry, y = chunk of BATCH_COPY_COLS columns, 16-byte accesses (both leading dimensions are even and every
// Sigma buffer starts on 16 bytes: the host checks). The last y also moves the landmarks, a lane per landmark: q0, Qq and Qa are copied; the 27 chart constants
// are formed from q0 by store_chart_constants, the one function every kernel that creates a landmark calls (k_scatter_landmarks of eqf_set_state and
// eqf_batch_set_state among them), so the destination's planes are those of the route through the host, bit for bit, whatever plane stride they were made at.
struct BridgeCtx {
    double* sig;   // the context's current Sigma buffer
    double* st;    // q0 (3 planes) and the chart constants behind them (CC_OFF), plane stride Ncap
    double *qq, *qa; // Qq (4 planes of stride Ncap), Qa
    int ld, Ncap;
};
struct BridgeIn {
    int slot, which; // the slot and the pair of its buffers the copy reads (store) or writes (load)
};
struct BridgeArgs {
    BatchBufs buf;
    BridgeCtx cx;
    const BridgeIn* in; // load: one entry per block x
    BridgeIn one;       // store: the entry itself
    int N;              // landmarks of the source
};
template <bool TO_CTX> __global__ void __launch_bounds__(BATCH_T) k_batch_bridge(const BridgeArgs ga) {
    const BridgeIn in = TO_CTX ? ga.one : ga.in[blockIdx.x];
    const int tid = threadIdx.x, L = BATCH_L, Ncap = ga.cx.Ncap;
    const int N = ga.N, n = 21 + 3 * N;
    const int c0 = blockIdx.y * BATCH_COPY_COLS, cols = min(BATCH_COPY_COLS, n - c0);
    const int lds = TO_CTX ? ga.buf.ld : ga.cx.ld, ldd = TO_CTX ? ga.cx.ld : ga.buf.ld;
    if (cols > 0) {
        const double* S = (TO_CTX ? ga.buf.sig_of(in.slot, in.which) : ga.cx.sig) + (size_t)c0 * lds;
        double* D = (TO_CTX ? ga.cx.sig : ga.buf.sig_of(in.slot, in.which)) + (size_t)c0 * ldd;
        const int half = n >> 1; // >= 10
        for (int t = tid; t < cols * half; t += BATCH_T) {
            const int c = t / half, r = 2 * (t % half);
            *reinterpret_cast<double2*>(D + (size_t)c * ldd + r) = *reinterpret_cast<const double2*>(S + (size_t)c * lds + r);
        }
        if ((n & 1) && tid < cols)
            D[(size_t)tid * ldd + n - 1] = S[(size_t)tid * lds + n - 1];
    }
    if (blockIdx.y == gridDim.y - 1 && tid < N) {
        const int i = tid;
        double* lm = ga.buf.lm_of(in.slot, in.which);
        if (TO_CTX) {
            const double px = lm[i], py = lm[L + i], pz = lm[2 * L + i];
            ga.cx.st[i] = px;
            ga.cx.st[Ncap + i] = py;
            ga.cx.st[2 * (size_t)Ncap + i] = pz;
            store_chart_constants(ga.cx.st + (size_t)CC_OFF * Ncap, Ncap, i, px, py, pz, nullptr);
            for (int c = 0; c < 4; ++c)
                ga.cx.qq[(size_t)c * Ncap + i] = lm[(BATCH_QQ + c) * L + i];
            ga.cx.qa[i] = lm[BATCH_QA * L + i];
        } else {
            const double px = ga.cx.st[i], py = ga.cx.st[Ncap + i], pz = ga.cx.st[2 * (size_t)Ncap + i];
            lm[i] = px;
            lm[L + i] = py;
            lm[2 * L + i] = pz;
            store_chart_constants(lm + (size_t)CC_OFF * L, L, i, px, py, pz, nullptr);
            for (int c = 0; c < 4; ++c)
                lm[(BATCH_QQ + c) * L + i] = ga.cx.qq[(size_t)c * Ncap + i];
            lm[BATCH_QA * L + i] = ga.cx.qa[i];
        }
    }
}

// eqf_batch_estimates (include/eqf_batch.h): entry e's workgroup reads its slot's CURRENT landmark planes and Sigma buffer and writes, into rec[e], the
// landmarks' camera-frame points p = Q^-1 q0 (eqf_batch_state_estimate's expression, the one k_batch_consistency uses for lm_err), their world-frame points
// pc * p with pc = pose * cameraOffset given by the host, and the 21 x 21 sensor block of Sigma, column-major - plain copies, so that block is Sigma's bit
// for bit. Entries of p / p_world beyond N are written as 0. N, the ids and the sensor estimate are the host's and are filled in there. The kernel writes
// nothing but the record: no LDS, no scratch area, no reduction - a record's bytes do not depend on the launch it is part of.
struct EstIn {
    int slot, cur, N, pad;
    Pose pc; // pose * cameraOffset of the slot's sensor estimate
};
struct EstArgs {
    BatchBufs buf;
    const EstIn* in;
    eqf_batch_estimate_record* rec;
};
__global__ void __launch_bounds__(BATCH_T) k_batch_estimate(const EstArgs ea) {
    const EstIn& in = ea.in[blockIdx.x];
    eqf_batch_estimate_record* rec = ea.rec + blockIdx.x;
    const int tid = threadIdx.x, ld = ea.buf.ld, N = in.N;
    const double* S = ea.buf.sig_of(in.slot, in.cur);
    const double* lm = ea.buf.lm_of(in.slot, in.cur);
    for (int i = tid; i < BATCH_L; i += BATCH_T) {
        V3 ph{0.0, 0.0, 0.0}, pw{0.0, 0.0, 0.0};
        if (i < N) {
            ph = batch_point_estimate(lm, i);
            pw = pose_act(in.pc, ph);
        }
        rec->p[3 * i] = ph.x, rec->p[3 * i + 1] = ph.y, rec->p[3 * i + 2] = ph.z;
        rec->p_world[3 * i] = pw.x, rec->p_world[3 * i + 1] = pw.y, rec->p_world[3 * i + 2] = pw.z;
    }
    for (int t = tid; t < 441; t += BATCH_T)
        rec->sigma_sensor[t] = S[t % 21 + (size_t)(t / 21) * ld];
}

// eqf_batch_predictions (include/eqf_batch.h): entry e's workgroup, a lane per landmark, reads its slot's CURRENT landmark planes and Sigma buffer and writes,
// into rec[e], landmark i's predicted camera-frame point p = T p_hat_i (p_hat = Q^-1 q0, eqf_batch_state_estimate's expression; T the product of the
// cameraPoseChangeInv of the host's predictState steps, the identity for none), its pixel cam.projectPoint(p), and getOutputCovById's C0_i Sigma_ii C0_i^T at the
// current estimate (k_output_cov's expressions: measure_one without the equivariant output, whose block does not depend on the pixel). A point with depth <= 0
// gets whatever cam_project gives. Entries beyond N are written as 0. N, the ids and the predicted sensor state are the host's and are filled in there. The
// kernel writes nothing but the record: no LDS, no scratch area, no reduction - a record's bytes do not depend on the launch it is part of.
struct PredIn {
    int slot, cur, N, chart;
    Cam cam;
    Pose T;
};
struct PredArgs {
    BatchBufs buf;
    const PredIn* in;
    eqf_batch_prediction_record* rec;
};
constexpr int BATCH_PRED_T = BATCH_L; // one wave: a lane per landmark
__global__ void __launch_bounds__(BATCH_PRED_T) k_batch_predict(const PredArgs pa) {
    const PredIn& in = pa.in[blockIdx.x];
    eqf_batch_prediction_record* rec = pa.rec + blockIdx.x;
    const int i = threadIdx.x, L = BATCH_L, ld = pa.buf.ld;
    V3 p{0.0, 0.0, 0.0};
    double yu = 0.0, yv = 0.0, v[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < in.N) {
        const double* Sig = pa.buf.sig_of(in.slot, in.cur);
        const double* lm = pa.buf.lm_of(in.slot, in.cur);
        p = pose_act(in.T, batch_point_estimate(lm, i));
        cam_project(in.cam, p, yu, yv);
        const MeasOut o = measure_one(in.chart, in.cam, ld3(lm, L, i), ldq(lm + BATCH_QQ * L, L, i), lm[BATCH_QA * L + i], 0.0, 0.0, false,
                                      in.chart == EQVIO_COORD_INVDEPTH ? ld_cc(lm, L, i, CC_R0) : M3{});
        const int l = 21 + 3 * i;
        double S[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                S[r][c] = Sig[l + r + (size_t)(l + c) * ld];
        double CS[2][3];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                CS[r][c] = o.c[r * 3 + 0] * S[0][c] + o.c[r * 3 + 1] * S[1][c] + o.c[r * 3 + 2] * S[2][c];
        v[0] = CS[0][0] * o.c[0] + CS[0][1] * o.c[1] + CS[0][2] * o.c[2];
        v[1] = CS[0][0] * o.c[3] + CS[0][1] * o.c[4] + CS[0][2] * o.c[5];
        v[2] = CS[1][0] * o.c[0] + CS[1][1] * o.c[1] + CS[1][2] * o.c[2];
        v[3] = CS[1][0] * o.c[3] + CS[1][1] * o.c[4] + CS[1][2] * o.c[5];
    }
    rec->p[3 * i] = p.x, rec->p[3 * i + 1] = p.y, rec->p[3 * i + 2] = p.z;
    rec->y[2 * i] = yu, rec->y[2 * i + 1] = yv;
    rec->out_cov[4 * i] = v[0], rec->out_cov[4 * i + 1] = v[1], rec->out_cov[4 * i + 2] = v[2], rec->out_cov[4 * i + 3] = v[3];
}

// ===================================================================================================
// eqf_batch_convert_chart (include/eqf_batch.h): entry e's workgroup re-expresses its slot's Sigma in another chart, Sigma' = T Sigma T^T with T = M_to M_from^-1.
// The charts' changes of coordinates against the Euclidean one are constant and block diagonal (coordinateDifferential_invdepth_euclid / _normal_euclid,
// VIOState.cpp:355-401): M_euclid = I, M_invdepth = blockdiag(I_21, conv_euc2ind(q0_i)), M_normal = the M of k_batch_normal (NormalM's sensor block, normal_M(q0_i)).
// So T's sensor block is the identity unless one side is Normal (sdir +1: M's, to Normal; -1: M^-1's, from Normal; 0: the identity), and landmark i's 3 x 3 block
// is one of conv_euc2ind, conv_ind2euc, normal_M, normal_Minv at q0_i or, between InvDepth and Normal, the product of two of them through Euclidean.
// The kernel reads the slot's CURRENT Sigma and landmark buffers and writes the OTHER ones, which the host then names current (k_batch_augment's and
// k_batch_copy's rule: no launch reads a slot's other pair before it has written it). q0, Qq and Qa are copied; the chart constants are formed from q0 by
// store_chart_constants, the one function every kernel that creates a landmark calls. A workgroup touches its own slot only and sums in a fixed order, so a
// slot's result has the same bytes whatever launch it is part of. The helpers below are this kernel's own: no other kernel's text changes.
struct RechartIn {
    int slot, cur, N;
    int from, to; // charts
    int sdir;     // the sensor block of T: +1 M (to Normal), -1 M^-1 (from Normal), 0 the identity
    double v0[3];  // xi0's velocity (NormalM::v0)
    double Ad[36]; // Ad(T0^-1) of xi0's camera offset, row-major (NormalM::Ad)
};
struct RechartArgs {
    BatchBufs buf;
    const RechartIn* in;
};
// a chart's 3 x 3 block against Euclidean at q0: M (inv false) or M^-1
__device__ __forceinline__ M3 rechart_chart_block(int chart, V3 q0, bool inv) {
    if (chart == EQVIO_COORD_INVDEPTH)
        return inv ? conv_ind2euc(q0) : conv_euc2ind(q0);
    return inv ? normal_Minv(q0) : normal_M(q0); // Normal: the Euclidean chart never gets here
}
// Landmark block of T = M_to M_from^-1 at q0, row-major into t[9]. One side Euclidean: the other side's block as it is; else the product through Euclidean.
__device__ __forceinline__ void rechart_landmark_block(int from, int to, V3 q0, double* t) {
    M3 T;
    if (from == EQVIO_COORD_EUCLIDEAN)
        T = rechart_chart_block(to, q0, false);
    else if (to == EQVIO_COORD_EUCLIDEAN)
        T = rechart_chart_block(from, q0, true);
    else
        T = rechart_chart_block(to, q0, false) * rechart_chart_block(from, q0, true);
    t[0] = T.a00, t[1] = T.a01, t[2] = T.a02, t[3] = T.a10, t[4] = T.a11, t[5] = T.a12, t[6] = T.a20, t[7] = T.a21, t[8] = T.a22;
}
// Row i of T in batch_normal_row's form (indices and coefficients, at most 7): the sensor rows from the entry, a landmark row from the table sT (LDS, 9 per landmark)
__device__ __forceinline__ int rechart_row(const RechartIn& in, const double* sT, int i, int (&idx)[7], double (&co)[7]) {
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        idx[k] = 0;
        co[k] = 0.0;
    }
    if (i < 21) {
        idx[0] = i;
        co[0] = 1.0;
        if (i < 12 || in.sdir == 0)
            return 1;
        const double sg = in.sdir > 0 ? 1.0 : -1.0;
        if (i < 15) { // [12:15, 6:9] = -skew(v0) (inverse: +skew(v0))
            const V3 r = row(skew(V3{in.v0[0], in.v0[1], in.v0[2]}), i - 12);
            idx[1] = 6, idx[2] = 7, idx[3] = 8;
            co[1] = -sg * r.x, co[2] = -sg * r.y, co[3] = -sg * r.z;
            return 4;
        }
        const double* ad = in.Ad + 6 * (i - 15); // [15:21, 6:12] = Ad(T0^-1) (inverse: -Ad(T0^-1))
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            idx[1 + c] = 6 + c;
            co[1 + c] = sg * ad[c];
        }
        return 7;
    }
    const int l = (i - 21) / 3, r = (i - 21) % 3;
    idx[0] = 21 + 3 * l, idx[1] = idx[0] + 1, idx[2] = idx[0] + 2;
    co[0] = sT[9 * l + 3 * r], co[1] = sT[9 * l + 3 * r + 1], co[2] = sT[9 * l + 3 * r + 2];
    return 3;
}
__global__ void __launch_bounds__(BATCH_T) k_batch_rechart(const RechartArgs ra) {
    __shared__ double sT[9 * BATCH_L];
    const RechartIn& in = ra.in[blockIdx.x];
    const int tid = threadIdx.x, L = BATCH_L, ld = ra.buf.ld;
    const int N = in.N, n = 21 + 3 * N;
    const double* S0 = ra.buf.sig_of(in.slot, in.cur);
    double* S1 = ra.buf.sig_of(in.slot, in.cur ^ 1);
    const double* L0 = ra.buf.lm_of(in.slot, in.cur);
    double* L1 = ra.buf.lm_of(in.slot, in.cur ^ 1);
    // the landmarks: their block of T into the table, their planes into the other buffer (a lane per landmark)
    if (tid < N) {
        const int i = tid;
        const double px = L0[i], py = L0[L + i], pz = L0[2 * L + i];
        rechart_landmark_block(in.from, in.to, V3{px, py, pz}, sT + 9 * i);
        L1[i] = px;
        L1[L + i] = py;
        L1[2 * L + i] = pz;
        store_chart_constants(L1 + (size_t)CC_OFF * L, L, i, px, py, pz, nullptr);
        for (int c = 0; c < 4; ++c)
            L1[(BATCH_QQ + c) * L + i] = L0[(BATCH_QQ + c) * L + i];
        L1[BATCH_QA * L + i] = L0[BATCH_QA * L + i];
    }
    __syncthreads();
    // Sigma' = T Sigma T^T: entry (i, j), i >= j, is sum_b T[j, b] (sum_a T[i, a] Sigma[a, b]) - (T_i Sigma_ij) first, then (. T_j^T) - and is mirrored
    for (int t = tid; t < n * n; t += BATCH_T) {
        const int i = t % n, j = t / n;
        if (in.sdir == 0 && i < 21 && j < 21) { // T's sensor block is the identity: Sigma's is copied, both halves as they are
            S1[i + (size_t)j * ld] = S0[i + (size_t)j * ld];
            continue;
        }
        if (i < j)
            continue;
        int ii[7], jj[7];
        double ci[7], cj[7];
        const int ni = rechart_row(in, sT, i, ii, ci), nj = rechart_row(in, sT, j, jj, cj);
        double acc = 0.0;
#pragma unroll
        for (int b = 0; b < 7; ++b) {
            if (b < nj) {
                const double* col = S0 + (size_t)jj[b] * ld;
                double s = 0.0;
#pragma unroll
                for (int a = 0; a < 7; ++a)
                    if (a < ni)
                        s = fma(ci[a], col[ii[a]], s);
                acc = fma(cj[b], s, acc);
            }
        }
        S1[i + (size_t)j * ld] = acc;
        S1[j + (size_t)i * ld] = acc;
    }
}

} // namespace eqf
