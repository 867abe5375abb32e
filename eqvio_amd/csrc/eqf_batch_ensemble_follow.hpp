// eqf_batch_ensemble_follow.hpp - kernels of eqf_bens_follow (eqvio_amd/csrc/eqf_batch_ensemble_follow.h): every listed cloud becomes a cloud over its slot's current
// landmarks - the kept point planes moved to their new places, the added landmarks drawn from the slot's belief conditional on what the particle already is.
// gfx950 only. Included at the end of eqf_hip.hip behind eqf_batch_ensemble_output_host.hpp. It reads eqf_batch_ensemble.hpp's BensBufs layouts and
// eqf_batch_ensemble_output.hpp's second place G (plane 23 + 64 c + i: coordinate c of point i) and calls chart_bwd / ld3 / ldq, philox4x64_10 /
// philox_normal_pair as they stand; k_bens_errors and k_bens_factor are launched unchanged in front of these kernels. No kernel or device function of another
// file is changed, and the packet of these kernels is its own (BensFollowIn): BensIn and BensOutIn keep their sizes.
// No kernel here talks to another workgroup: the pivot flag of an adding entry is written by k_bens_factor and read by the launches behind it.
#pragma once
#include "eqf_batch_ensemble_output.hpp"

namespace eqf {

// one entry of a call, prepared by the host. The entries that add come first in the packet: entry q < nadd has the pivot flag flag[q].
struct BensFollowIn {
    int slot, cur, N, P; // the slot, its current buffers and landmarks (the cloud's landmarks after the call), the cloud's particles
    int nK, chart;       // the kept landmarks: the first nK of the slot's order; the slot's chart
    unsigned long long seed, stream;
    int from[BATCH_L]; // i < nK: the cloud's old place of the slot's landmark i
};
struct BensFollowArgs {
    BatchBufs buf;
    BensBufs eb;
    double* G; // the second place of the move (null when no entry of the call moves a plane)
    const BensFollowIn* in;
    int nadd;
};

// ---- rows nk .. n - 1 of eps = L [z_K ; Xi_A] for 16 particles per wave, nk = 21 + 3 nK, z_K = L_KK^-1 eps_K with eps_K the rows k_bens_errors left in the
// slot's E. Three passes over the wave's LDS tile Ys (row r, particle p at Ys[16 r + p]):
//  1. k_bens_solve's blocked forward substitution over rows 0 .. nk - 1 (the tiles on the left on the MFMA, the 16 x 16 triangle on the VALU, the pivot row
//     handed over by a lane shuffle); rows from nk on are masked to zero, the diagonal there to one;
//  2. k_bens_sample_eps' fill: a lane per (row block of four, particle), counter (j, p0 + p, 0, 0) - of the block nk >> 2 only the rows from nk on are written;
//  3. k_bens_sample_eps' product over the 16-row tiles from the one that holds row nk, k ascending in steps of 4 up to the tile's last row; only rows nk .. n - 1
//     are written to E.
// A particle's rows depend on its own column of E, on L and on (seed, stream, its index) alone. Returns without writing where the entry's pivot flag is set.
// grid (ceil(Pmax / 16), adding entries), one wave.
__global__ void __launch_bounds__(64) k_bens_follow_eps(const BensFollowArgs a) {
    __shared__ double Ys[BENS_XR * 16];
    const BensFollowIn& in = a.in[blockIdx.y];
    const int P = in.P, p0 = blockIdx.x * 16;
    if (a.eb.flag[blockIdx.y] || p0 >= P)
        return;
    const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4, ldp = a.eb.ldp;
    const int n = 21 + 3 * in.N, nk = 21 + 3 * in.nK, nb = (n + 3) >> 2;
    const double* L = a.eb.L_of(in.slot);
    double* E = a.eb.E_of(in.slot);
    for (int i0 = 0; i0 < nk; i0 += 16) {
        const int row = i0 + lr, rowc = min(row, nk - 1);
        d4 acc = {0, 0, 0, 0};
        for (int k0 = 0; k0 < i0; k0 += 4) {
            const int k = k0 + lk; // < i0 <= nk - 1
            const double lv = L[rowc + (size_t)k * BENS_LDL];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ys[k * 16 + lr], row < nk ? lv : 0.0, acc, 0, 0, 0);
        }
        double t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int pp = p0 + lk + 4 * q, ppc = min(pp, P - 1);
            const double ev = E[ppc + (size_t)rowc * ldp];
            t[q] = ((row < nk && pp < P) ? ev : 0.0) - acc[q];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int rj = i0 + j, rjc = min(rj, nk - 1);
            const double dv = L[rjc + (size_t)rjc * BENS_LDL], ov = L[rowc + (size_t)rjc * BENS_LDL];
            const double ljj = rj < nk ? dv : 1.0;
            const double lrj = (row < nk && rj < nk && lr > j) ? ov : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double yj = __shfl(t[q], (lane & 48) | j, 64) / ljj;
                t[q] = lr == j ? yj : t[q] - lrj * yj;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            Ys[row * 16 + lk + 4 * q] = t[q]; // row <= 16 ceil(nk / 16) - 1 < BENS_XR
        __syncthreads();
    }
    const int jb = nk >> 2; // the first row block of normals that is used, partly where nk is no multiple of 4
    for (int t = lane; t < (nb - jb) * 16; t += 64) {
        const int j = jb + (t >> 4), p = t & 15;
        unsigned long long x[4];
        philox4x64_10(in.seed, in.stream, (unsigned long long)j, (unsigned long long)(p0 + p), 0ull, 0ull, x);
        double z[4];
        philox_normal_pair(x[0], x[1], z[0], z[1]);
        philox_normal_pair(x[2], x[3], z[2], z[3]);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (4 * j + c >= nk)
                Ys[(4 * j + c) * 16 + p] = z[c]; // < 4 nb <= 216 rows
    }
    __syncthreads();
    for (int i0 = nk & ~15; i0 < n; i0 += 16) {
        const int row = i0 + lr, rowc = min(row, n - 1), kend = min(n, i0 + 16);
        d4 acc = {0, 0, 0, 0};
        for (int k0 = 0; k0 < kend; k0 += 4) {
            const int k = k0 + lk, kc = min(k, n - 1); // k < 4 nb: inside the tile
            const double lv = L[rowc + (size_t)kc * BENS_LDL], xv = Ys[k * 16 + lr];
            const double av = (row < n && k <= row) ? lv : 0.0; // L[i0 + lr][k], lower triangle (k <= row < n)
            const double bv = k < n ? xv : 0.0;                 // [z_K ; Xi_A][k][p0 + lr]
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(bv, av, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int pp = p0 + lk + 4 * q;
            if (row >= nk && row < n && pp < P)
                E[pp + (size_t)row * ldp] = acc[q];
        }
    }
}

// ---- the point planes, a lane per (entry, landmark i of the slot's order, particle). The move cannot be in place (landmark i's new place may be the old
// place of another kept one), so it goes through the second place G and back, in two launches:
//  back == 0: a kept landmark whose place changes (i < nK, from[i] != i): its three planes from the cloud's place from[i] to G's place i;
//  back == 1: the same planes from G to the cloud's place i - the bytes they held; an added landmark (nK <= i < N): p = Q_i^-1 chart^-1(eps_i ; q0_i) from
//             the rows k_bens_follow_eps left in E, k_bens_sample_apply's landmark branch.
// The sensor planes are not touched. An adding entry whose pivot flag is set is skipped by both launches: its planes do not move.
// grid (ceil(Pmax / 256), Nmax, entries).
__global__ void __launch_bounds__(BATCH_T) k_bens_follow_place(const BensFollowArgs a, int back) {
    const BensFollowIn& in = a.in[blockIdx.z];
    const int k = blockIdx.x * BATCH_T + threadIdx.x, i = blockIdx.y, ldp = a.eb.ldp;
    if (k >= in.P || i >= in.N || ((int)blockIdx.z < a.nadd && a.eb.flag[blockIdx.z]))
        return;
    double* pts = a.eb.pts_of(in.slot);
    if (i < in.nK) {
        const int o = in.from[i];
        if (o == i)
            return;
        double* g = a.G + ((size_t)in.slot * BENS_GP + 23 + i) * ldp + k;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (back)
                pts[bens_pt(ldp, c, i, k)] = g[(size_t)c * BATCH_L * ldp];
            else
                g[(size_t)c * BATCH_L * ldp] = pts[bens_pt(ldp, c, o, k)];
        }
    } else if (back) {
        const int Lm = BATCH_L;
        const double* E = a.eb.E_of(in.slot);
        const double* lm = a.buf.lm_of(in.slot, in.cur);
        const V3 e{E[k + (size_t)(21 + 3 * i) * ldp], E[k + (size_t)(22 + 3 * i) * ldp], E[k + (size_t)(23 + 3 * i) * ldp]};
        const V3 q = chart_bwd(in.chart, e, ld3(lm, Lm, i));
        const V3 p = (1.0 / lm[BATCH_QA * Lm + i]) * q_rot(q_inv(ldq(lm + BATCH_QQ * Lm, Lm, i)), q);
        pts[bens_pt(ldp, 0, i, k)] = p.x;
        pts[bens_pt(ldp, 1, i, k)] = p.y;
        pts[bens_pt(ldp, 2, i, k)] = p.z;
    }
}

} // namespace eqf
