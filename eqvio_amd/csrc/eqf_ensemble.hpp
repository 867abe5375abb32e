// eqf_ensemble.hpp - kernels of the particle ensemble (include/eqf_ensemble.h): P hypotheses of the true state against one context. gfx950 only.
// Included by eqf_hip.hip behind eqf_fork.hpp. It calls eqf_kernels.hpp's chart_fwd / chart_bwd, ld3 / ldq and eqf_math.hpp as they stand; no kernel or device
// function of another file is changed by it. No kernel here talks to another workgroup: no flags, no waits, no co-residency.
//
// Layouts. A particle's points: plane (c, i) = coordinate c of landmark i, particles contiguous: pts[(c * Ncap + i) * ldp + k] - a lane per (particle, landmark)
// reads and writes coalesced. Error coordinates: E[k + c * ldp], particle k, coordinate c ("particle-major": E^T of the header's n x P matrix), so that a row of
// E^T enters the factorisation's work matrix Z as a contiguous run and a lane per particle stores coalesced.
#pragma once
#include "eqf_kernels.hpp"

namespace eqf {

__device__ __forceinline__ size_t ens_at(int Ncap, int ldp, int c, int i, int k) { return ((size_t)c * Ncap + i) * ldp + k; }

// eps of landmark i (the filter's index) for every particle: stateChart(Q_i p_true ; q0_i), Q_i p = a R p (eqf_compute_nees' host loop, one lane per (particle, landmark)).
// match[i]: the landmark's place in the ensemble's id list. grid (ceil(P / 256), N).
__global__ void __launch_bounds__(256) k_ens_errors(int P, int NcapCtx, int chart, const double* __restrict__ q0, const double* __restrict__ Qq, const double* __restrict__ Qa,
                                                    const int* __restrict__ match, const double* __restrict__ pts, int NcapE, int ldp, double* __restrict__ E) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (k >= P)
        return;
    const int t = match[i];
    const V3 ptrue{pts[ens_at(NcapE, ldp, 0, t, k)], pts[ens_at(NcapE, ldp, 1, t, k)], pts[ens_at(NcapE, ldp, 2, t, k)]};
    const V3 pe = Qa[i] * q_rot(ldq(Qq, NcapCtx, i), ptrue);
    const V3 e = chart_fwd(chart, pe, ld3(q0, NcapCtx, i));
    E[k + (size_t)(21 + 3 * i) * ldp] = e.x;
    E[k + (size_t)(22 + 3 * i) * ldp] = e.y;
    E[k + (size_t)(23 + 3 * i) * ldp] = e.z;
}

// Z for the factorisation chain: rows [0, np) = Sigma padded to the even dimension np with a unit diagonal (k_build_nees' square), then `extra` rows:
// dup == 0: row np + k = eps_k^T (the chain leaves eps_k^T L^-T there); dup == 1: Sigma's padded rows once more (the chain leaves Sigma L^-T = L there).
// grid (ceil((np + extra) / 256), np).
__global__ void __launch_bounds__(256) k_ens_build_Z(int n, int np, int ld, int ldz, const double* __restrict__ Sig, const double* __restrict__ E, int ldp, int extra, int dup,
                                                     double* __restrict__ Z) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
    if (r >= np + extra)
        return;
    double v;
    if (r >= np && !dup)
        v = c < n ? E[(r - np) + (size_t)c * ldp] : 0.0;
    else {
        const int rr = r >= np ? r - np : r;
        v = (rr < n && c < n) ? Sig[rr + (size_t)c * ld] : ((rr == c) ? 1.0 : 0.0);
    }
    Z[r + (size_t)c * ldz] = v;
}

// |row np + k of W|^2 for every particle. A workgroup takes 32 particles; lane group g of its 8 sums the columns c = g (mod 8) in ascending order and the 8 partial
// sums are added in one fixed tree: a particle's value depends on its own row alone - the same bits wherever it stands and whatever P is. grid ceil(P / 32).
// (One lane per particle over all np columns was 167 us at n = 621, a quarter of the whole call.)
__global__ void __launch_bounds__(256) k_ens_rowsumsq(int P, int np, int ldz, const double* __restrict__ W, double* __restrict__ out) {
    __shared__ double sp[8][33];
    const int r = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int k = blockIdx.x * 32 + r, kc = min(k, P - 1);
    double s = 0.0;
    for (int c = g; c < np; c += 8) {
        const double v = W[np + kc + (size_t)c * ldz];
        s = __builtin_fma(v, v, s);
    }
    sp[g][r] = s;
    __syncthreads();
    if (g == 0 && k < P)
        out[k] = ((sp[0][r] + sp[1][r]) + (sp[2][r] + sp[3][r])) + ((sp[4][r] + sp[5][r]) + (sp[6][r] + sp[7][r]));
}

// E^T = (L Xi)^T with L = rows [np, np + n) of W, lower triangle only (what the chain left above the diagonal is rounding noise and is masked), Xi n x P column-major.
// One wave per 16 x 16 tile (16 coordinates x 16 particles), k ascending in steps of 4 up to the tile's last row. grid (ceil(n / 16), ceil(P / 64)), 4 waves.
__global__ void __launch_bounds__(256) k_ens_trmm(int n, int np, int P, int ldz, const double* __restrict__ W, const double* __restrict__ Xi, double* __restrict__ E, int ldp) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lr = lane & 15, lk = lane >> 4;
    const int i0 = blockIdx.x * 16, p0 = (blockIdx.y * 4 + wave) * 16;
    if (p0 >= P)
        return;
    const int row = i0 + lr, rowc = min(row, n - 1);
    const int pj = p0 + lr, pjc = min(pj, P - 1);
    const int kend = min(n, i0 + 16);
    d4 acc = {0, 0, 0, 0};
    for (int k0 = 0; k0 < kend; k0 += 4) {
        const int k = k0 + lk, kc = min(k, n - 1);
        const double lv = W[np + rowc + (size_t)kc * ldz], xv = Xi[kc + (size_t)pjc * n];
        const double a = (row < n && k < n && k <= row) ? lv : 0.0; // I operand: L[i0 + lr][k]
        const double b = (k < n && pj < P) ? xv : 0.0;              // J operand: Xi[k][p0 + lr]
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(b, a, acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int pp = p0 + lk + 4 * q;
        if (row < n && pp < P)
            E[pp + (size_t)row * ldp] = acc[q];
    }
}

// particle_k's point i = stateGroupAction(X, stateChart^-1(eps_k))_i = Q_i^-1 chart^-1(eps_k,i ; q0_i). grid (ceil(P / 256), N).
__global__ void __launch_bounds__(256) k_ens_sample_points(int P, int NcapCtx, int chart, const double* __restrict__ q0, const double* __restrict__ Qq,
                                                           const double* __restrict__ Qa, const double* __restrict__ E, int ldp, double* __restrict__ pts, int NcapE) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (k >= P)
        return;
    const V3 e{E[k + (size_t)(21 + 3 * i) * ldp], E[k + (size_t)(22 + 3 * i) * ldp], E[k + (size_t)(23 + 3 * i) * ldp]};
    const V3 q = chart_bwd(chart, e, ld3(q0, NcapCtx, i));
    const V3 p = (1.0 / Qa[i]) * q_rot(q_inv(ldq(Qq, NcapCtx, i)), q);
    pts[ens_at(NcapE, ldp, 0, i, k)] = p.x;
    pts[ens_at(NcapE, ldp, 1, i, k)] = p.y;
    pts[ens_at(NcapE, ldp, 2, i, k)] = p.z;
}

// integrateSystemFunction's landmark part: p <- cameraPoseChangeInv_k * p, the pose of particle k as 7 planes of stride ldp (quaternion w x y z, translation).
// grid (ceil(P / 256), N), in place.
__global__ void __launch_bounds__(256) k_ens_integrate(int P, const double* __restrict__ pose7, double* __restrict__ pts, int NcapE, int ldp) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (k >= P)
        return;
    const Pose T{Qt{pose7[k], pose7[ldp + k], pose7[2 * (size_t)ldp + k], pose7[3 * (size_t)ldp + k]},
                 V3{pose7[4 * (size_t)ldp + k], pose7[5 * (size_t)ldp + k], pose7[6 * (size_t)ldp + k]}};
    const V3 p{pts[ens_at(NcapE, ldp, 0, i, k)], pts[ens_at(NcapE, ldp, 1, i, k)], pts[ens_at(NcapE, ldp, 2, i, k)]};
    const V3 r = pose_act(T, p);
    pts[ens_at(NcapE, ldp, 0, i, k)] = r.x;
    pts[ens_at(NcapE, ldp, 1, i, k)] = r.y;
    pts[ens_at(NcapE, ldp, 2, i, k)] = r.z;
}

// out's particle k = in's particle src[k]. grid (ceil(Pnew / 256), 3 N).
__global__ void __launch_bounds__(256) k_ens_gather(int Pnew, const int* __restrict__ src, const double* __restrict__ in, double* __restrict__ out, int NcapE, int N, int ldp) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Pnew)
        return;
    const int c = blockIdx.y / N, i = blockIdx.y % N;
    out[ens_at(NcapE, ldp, c, i, k)] = in[ens_at(NcapE, ldp, c, i, src[k])];
}

// C = E E^T / P (n x n, leading dimension n): one wave per 16 x 16 tile of the lower triangle, particles in ascending order in steps of 4; the mirror image is
// written from the same register, and a diagonal tile writes only its lower half and its mirror. grid (ceil(n / 16), ceil(n / 16)), one wave.
__global__ void __launch_bounds__(64) k_ens_cov(int n, int P, const double* __restrict__ E, int ldp, double* __restrict__ Cout) {
    const int i0 = blockIdx.x * 16, j0 = blockIdx.y * 16;
    if (j0 > i0)
        return;
    const int lr = threadIdx.x & 15, lk = threadIdx.x >> 4;
    const int ri = min(i0 + lr, n - 1), rj = min(j0 + lr, n - 1);
    d4 acc = {0, 0, 0, 0};
    for (int p0 = 0; p0 < P; p0 += 4) {
        const int pp = p0 + lk, ppc = min(pp, P - 1);
        const double av = E[ppc + (size_t)ri * ldp], bv = E[ppc + (size_t)rj * ldp];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pp < P ? bv : 0.0, pp < P ? av : 0.0, acc, 0, 0, 0);
    }
    const int i = i0 + lr;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + lk + 4 * q;
        if (i < n && j < n && (i0 != j0 || i >= j)) {
            const double v = acc[q] / (double)P;
            Cout[i + (size_t)j * n] = v;
            Cout[j + (size_t)i * n] = v;
        }
    }
}

} // namespace eqf
