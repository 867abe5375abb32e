// eqf_fork.hpp - kernels of eqf_copy_ctx and eqf_convert_chart (include/eqf_hip.h): a context's whole filter into another context, and a context's Sigma
// into another chart, both on the device. gfx950 only. Included by eqf_hip.hip behind eqf_batch.hpp, whose rechart_landmark_block (the landmark block of
// T = M_to M_from^-1 at q0: conv_euc2ind, conv_ind2euc, normal_M, normal_Minv or a product of two) this file calls as it stands. No kernel or device function
// of another file is changed by it.
#pragma once
#include "eqf_batch.hpp"

namespace eqf {

// ---------------------------------------------------------------------------------------------------
// k_ctx_copy: Sigma (n x n, column-major) and the landmark planes from one context's layout into another's - both leading dimensions, both plane strides.
// grid (ceil(ceil(n / 2) / 256), ceil(n / CTX_COPY_COLS) + 1): block row y < the column chunks copies CTX_COPY_COLS columns of Sigma, 256 pairs of rows per block
// column; the last block row copies the planes, live landmarks only. vec_sigma / vec_planes (the host checks alignment): 16-byte accesses, an odd last row or
// landmark by one 8-byte access; otherwise every element by an 8-byte access. Pure data movement: the destination holds the source's bits.
constexpr int CTX_COPY_COLS = 4, CTX_COPY_T = 256;
struct CtxCopySide {
    double* sigma;    // the context's current Sigma buffer
    double* st;       // q0 (3 planes) and the chart constants behind them (CC_OFF + CC_PLANES planes in all), plane stride Ncap
    double* lm;       // Qq (4 planes of stride Ncap), then Qa
    int ld, Ncap;
};
struct CtxCopyArgs {
    CtxCopySide src, dst; // (src is only read)
    int N;
    int vec_sigma, vec_planes;
};
__device__ __forceinline__ void ctx_copy_run(double* __restrict__ D, const double* __restrict__ S, int count, int x, bool vec) {
    // elements [0, count) of one contiguous run; x = this thread's pair index within the run
    if (vec) {
        if (2 * x + 1 < count)
            *reinterpret_cast<double2*>(D + 2 * x) = *reinterpret_cast<const double2*>(S + 2 * x);
        else if (2 * x < count)
            D[2 * x] = S[2 * x];
    } else {
        if (2 * x < count)
            D[2 * x] = S[2 * x];
        if (2 * x + 1 < count)
            D[2 * x + 1] = S[2 * x + 1];
    }
}
__global__ void __launch_bounds__(CTX_COPY_T) k_ctx_copy(const CtxCopyArgs ca) {
    const int N = ca.N, n = 21 + 3 * N;
    const int x = blockIdx.x * CTX_COPY_T + threadIdx.x;
    const int chunks = (n + CTX_COPY_COLS - 1) / CTX_COPY_COLS;
    if ((int)blockIdx.y < chunks) {
        const int c0 = blockIdx.y * CTX_COPY_COLS;
#pragma unroll
        for (int k = 0; k < CTX_COPY_COLS; ++k)
            if (c0 + k < n)
                ctx_copy_run(ca.dst.sigma + (size_t)(c0 + k) * ca.dst.ld, ca.src.sigma + (size_t)(c0 + k) * ca.src.ld, n, x, ca.vec_sigma != 0);
        return;
    }
    if (2 * x >= N)
        return;
    for (int p = 0; p < CC_OFF + CC_PLANES; ++p)
        ctx_copy_run(ca.dst.st + (size_t)p * ca.dst.Ncap, ca.src.st + (size_t)p * ca.src.Ncap, N, x, ca.vec_planes != 0);
    for (int p = 0; p < 5; ++p)
        ctx_copy_run(ca.dst.lm + (size_t)p * ca.dst.Ncap, ca.src.lm + (size_t)p * ca.src.Ncap, N, x, ca.vec_planes != 0);
}

// ---------------------------------------------------------------------------------------------------
// k_ctx_rechart: Sigma' = T Sigma T^T with T = M_to M_from^-1 (k_batch_rechart's T), out of place, for a context of any size.
// Row groups are cut along landmark boundaries: group 0 = the 21 sensor rows, group g >= 1 = the landmarks [RC_G (g - 1), RC_G g). T is block diagonal - one
// 21 x 21 block (the identity unless a side is Normal), one 3 x 3 block per landmark - so tile (gi, gj) of Sigma' is a function of tile (gi, gj) of Sigma and of
// the blocks of T of the two groups alone. One workgroup per tile of the lower triangle (gi >= gj), blockIdx.x = gi (gi + 1) / 2 + gj:
//   1. the blocks of T of its row group and of its column group, formed once from q0 into LDS (a lane per landmark; two waves, one per group);
//   2. its tile of Sigma into LDS, consecutive lanes on consecutive rows of a column (runs of up to 48 doubles);
//   3. entry (i, j) = sum_b T[j, b] (sum_a T[i, a] Sigma[a, b]): (T_i Sigma_ij) first, then (. T_j^T), both by fma from 0 in ascending a and b over the row's
//      non-zeros - 3 for a landmark row, up to 7 for a sensor row (normal_row's lists) - into a second LDS tile; a diagonal tile computes i >= j and mirrors there;
//   4. the tile and, off the diagonal, its transpose written from LDS, consecutive lanes on consecutive rows: Sigma' is symmetric bit for bit.
// With sdir == 0 (neither side Normal) tile (0, 0) is copied as it is. An entry's value depends on nothing but Sigma, q0 and the sensor constants: not on the
// grid, the capacity or the leading dimension. No flag, no wait, no co-residency: a workgroup reads the old buffer and writes its own tile (and mirror) of the new one.
constexpr int RC_G = 16, RC_ROWS = 3 * RC_G, RC_LDT = RC_ROWS + 1, RC_T = 256; // (odd tile stride: the transposed read of step 4 walks distinct banks)
static_assert(RC_ROWS >= 21, "group 0 (the sensor rows) must fit a tile");
struct CtxRechartArgs {
    const double* S0; // current Sigma buffer
    double* S1;       // the other one
    const double* q0; // 3 planes of stride Ncap
    int N, Ncap, ld;
    int from, to; // charts
    int sdir;     // the sensor block of T: +1 M (to Normal), -1 M^-1 (from Normal), 0 the identity
    double v0[3];  // xi0's velocity (NormalM::v0)
    double Ad[36]; // Ad(T0^-1) of xi0's camera offset, row-major (NormalM::Ad)
};
__host__ __device__ __forceinline__ int rc_groups(int N) { return 1 + (N + RC_G - 1) / RC_G; }
__device__ __forceinline__ int rc_row0(int g) { return g == 0 ? 0 : 21 + RC_ROWS * (g - 1); }
__device__ __forceinline__ int rc_rows(int g, int N) { return g == 0 ? 21 : 3 * min(RC_G, N - RC_G * (g - 1)); }
// Row r (local to group g) of T, indices local to the group: a sensor row as rechart_row writes it, a landmark row from the group's table sT (9 per landmark)
__device__ __forceinline__ int rc_row(const CtxRechartArgs& ra, int g, const double* sT, int r, int (&idx)[7], double (&co)[7]) {
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        idx[k] = 0;
        co[k] = 0.0;
    }
    if (g == 0) {
        idx[0] = r;
        co[0] = 1.0;
        if (r < 12 || ra.sdir == 0)
            return 1;
        const double sg = ra.sdir > 0 ? 1.0 : -1.0;
        if (r < 15) { // [12:15, 6:9] = -skew(v0) (inverse: +skew(v0))
            const V3 k = row(skew(V3{ra.v0[0], ra.v0[1], ra.v0[2]}), r - 12);
            idx[1] = 6, idx[2] = 7, idx[3] = 8;
            co[1] = -sg * k.x, co[2] = -sg * k.y, co[3] = -sg * k.z;
            return 4;
        }
        const double* ad = ra.Ad + 6 * (r - 15); // [15:21, 6:12] = Ad(T0^-1) (inverse: -Ad(T0^-1))
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            idx[1 + c] = 6 + c;
            co[1 + c] = sg * ad[c];
        }
        return 7;
    }
    const int l = r / 3, k = r % 3;
    idx[0] = 3 * l, idx[1] = idx[0] + 1, idx[2] = idx[0] + 2;
    co[0] = sT[9 * l + 3 * k], co[1] = sT[9 * l + 3 * k + 1], co[2] = sT[9 * l + 3 * k + 2];
    return 3;
}
__global__ void __launch_bounds__(RC_T) k_ctx_rechart(const CtxRechartArgs ra) {
    __shared__ double sIn[RC_ROWS * RC_LDT], sOut[RC_ROWS * RC_LDT];
    __shared__ double sTi[9 * RC_G], sTj[9 * RC_G];
    const int tid = threadIdx.x, N = ra.N, ld = ra.ld;
    // tile (gi, gj) of the lower triangle from the block index
    const int b = blockIdx.x;
    int gi = (int)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while (gi * (gi + 1) / 2 > b)
        --gi;
    while ((gi + 1) * (gi + 2) / 2 <= b)
        ++gi;
    const int gj = b - gi * (gi + 1) / 2;
    if (gi >= rc_groups(N))
        return;
    const int Ri = rc_rows(gi, N), Rj = rc_rows(gj, N), i0 = rc_row0(gi), j0 = rc_row0(gj);
    const double* Sin = ra.S0 + i0 + (size_t)j0 * ld;
    if (gi == 0 && ra.sdir == 0) { // T's sensor block is the identity: Sigma's is copied, both halves as they are
        for (int t = tid; t < 21 * 21; t += RC_T)
            ra.S1[t % 21 + (size_t)(t / 21) * ld] = Sin[t % 21 + (size_t)(t / 21) * ld];
        return;
    }
    // 1. the groups' blocks of T (waves 0 and 1)
    if (gi > 0 && tid < Ri / 3) {
        const int l = RC_G * (gi - 1) + tid;
        rechart_landmark_block(ra.from, ra.to, ld3(ra.q0, ra.Ncap, l), sTi + 9 * tid);
    }
    if (gj > 0 && tid >= 64 && tid - 64 < Rj / 3) {
        const int l = RC_G * (gj - 1) + tid - 64;
        rechart_landmark_block(ra.from, ra.to, ld3(ra.q0, ra.Ncap, l), sTj + 9 * (tid - 64));
    }
    // 2. the tile of Sigma
    for (int t = tid; t < Ri * Rj; t += RC_T) {
        const int r = t % Ri, c = t / Ri;
        sIn[c * RC_LDT + r] = Sin[r + (size_t)c * ld];
    }
    __syncthreads();
    // 3. the entries
    const bool diag = gi == gj;
    for (int t = tid; t < Ri * Rj; t += RC_T) {
        const int r = t % Ri, c = t / Ri;
        if (diag && r < c)
            continue;
        int ii[7], jj[7];
        double ci[7], cj[7];
        const int ni = rc_row(ra, gi, sTi, r, ii, ci), nj = rc_row(ra, gj, sTj, c, jj, cj);
        double acc = 0.0;
#pragma unroll
        for (int bb = 0; bb < 7; ++bb) {
            if (bb < nj) {
                const double* col = sIn + jj[bb] * RC_LDT;
                double s = 0.0;
#pragma unroll
                for (int a = 0; a < 7; ++a)
                    if (a < ni)
                        s = fma(ci[a], col[ii[a]], s);
                acc = fma(cj[bb], s, acc);
            }
        }
        sOut[c * RC_LDT + r] = acc;
        if (diag)
            sOut[r * RC_LDT + c] = acc;
    }
    __syncthreads();
    // 4. the tile and its mirror image
    double* Sout = ra.S1 + i0 + (size_t)j0 * ld;
    for (int t = tid; t < Ri * Rj; t += RC_T) {
        const int r = t % Ri, c = t / Ri;
        Sout[r + (size_t)c * ld] = sOut[c * RC_LDT + r];
    }
    if (!diag) {
        double* Smir = ra.S1 + j0 + (size_t)i0 * ld;
        for (int t = tid; t < Ri * Rj; t += RC_T) {
            const int c = t % Rj, r = t / Rj; // consecutive lanes on consecutive rows of the mirror image (= columns of the tile)
            Smir[c + (size_t)r * ld] = sOut[c * RC_LDT + r];
        }
    }
}

} // namespace eqf
