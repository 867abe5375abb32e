// eqf_batch_ensemble_output.hpp - kernels of the measurement side of the particle ensembles against batch slots (include/eqf_batch_ensemble_output.h): every
// listed cloud's log-likelihoods, normalised weights and running sums, weightedResample's choice with the uniforms generated in place, the gather of the chosen
// particles, and the particle covariance. gfx950 only. Included by eqf_hip.hip behind eqf_batch_ensemble_host.hpp. It reads eqf_batch_ensemble.hpp's BensBufs
// layouts (sens_of / pts_of / E_of, bens_pt), eqf_math.hpp's cam_project and eqf_ensemble_random.hpp's philox4x64_10 / philox_unit as they stand; no kernel or
// device function of another file is changed by it, and the packet of these kernels is its own (BensOutIn): BensIn keeps its size.
// k_bens_loglik, k_bens_weights and k_bens_pick restate k_ens_loglik, k_ens_weights (raw == 0) and k_ens_pick of eqf_ensemble_output.hpp with the same operations
// in the same order, an entry per blockIdx.y (blockIdx.x for the weights); those kernels themselves stay as they are.
// No kernel here talks to another workgroup.
//
// Layouts (BensOutBufs). Per entry q of a call: scal[4 q ..] = (max, sum, sum of squares, number of finite entries), ll[q ldp + k], w[q ldp + k],
// src[q ldp + k]. Per slot s: the running sums cum[s ldp + k] (what a later resample reads: the kept weights), and the gather's second place
// G[(215 s + plane) ldp + k], plane c < 23 a sensor plane, 23 + 64 c + i coordinate c of point i.
#pragma once
#include "eqf_batch_ensemble.hpp"

namespace eqf {

constexpr int BENS_GP = 23 + 3 * BATCH_L; // 215 planes of a cloud

struct BensOutBufs {
    double *scal, *ll, *w, *cum, *G;
    int* src;
    __host__ __device__ double* cum_of(int slot, int ldp) const { return cum + (size_t)slot * ldp; }
    __host__ __device__ double* G_of(int slot, int ldp) const { return G + (size_t)slot * BENS_GP * ldp; }
};
// one entry of a likelihood or resample call, prepared by the host
struct BensOutIn {
    int slot, P, N, M; // the slot, its cloud's particles and landmarks, the measured landmarks
    int P_new, pad;
    unsigned long long seed, stream;
    double meas_var;
    Cam cam;
    double y[2 * BATCH_L];
    int match[BATCH_L]; // the measured landmark j is the cloud's landmark match[j]
};
struct BensOutArgs {
    BensBufs eb;
    BensOutBufs ob;
    const BensOutIn* in;
};

// ---- ll[q ldp + k] of every particle of every entry: k_ens_loglik's body. A workgroup takes 32 particles, lane group g of its 8 sums the landmarks
// j = g (mod 8) in ascending order (u then v) and the 8 partial sums are added in one fixed tree. A workgroup wholly beyond its entry's P returns as one; inside
// the last one the particle index is clamped, so that every lane reaches the barrier. grid (ceil(Pmax / 32), entries).
__global__ void __launch_bounds__(256) k_bens_loglik(const BensOutArgs a) {
    __shared__ double sp[8][33];
    const BensOutIn& in = a.in[blockIdx.y];
    const int P = in.P, M = in.M, ldp = a.eb.ldp;
    if ((int)blockIdx.x * 32 >= P)
        return;
    const int r = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int k = blockIdx.x * 32 + r, kc = min(k, P - 1);
    const double* pts = a.eb.pts_of(in.slot);
    double s = 0.0;
    for (int j = g; j < M; j += 8) {
        const int t = in.match[j];
        const V3 p{pts[bens_pt(ldp, 0, t, kc)], pts[bens_pt(ldp, 1, t, kc)], pts[bens_pt(ldp, 2, t, kc)]};
        double u, v;
        cam_project(in.cam, p, u, v);
        const double eu = in.y[2 * j] - u, ev = in.y[2 * j + 1] - v;
        s = __builtin_fma(eu, eu, s);
        s = __builtin_fma(ev, ev, s);
    }
    sp[g][r] = s;
    __syncthreads();
    if (g == 0 && k < P) {
        const double tot = ((sp[0][r] + sp[1][r]) + (sp[2][r] + sp[3][r])) + ((sp[4][r] + sp[5][r]) + (sp[6][r] + sp[7][r]));
        const double v = 0.0 - 0.5 * tot / in.meas_var;
        a.ob.ll[(size_t)blockIdx.y * ldp + k] = isfinite(v) ? v : -INFINITY;
    }
}

// ---- the normalised weights, the running sums and the four scalars of every entry, ONE workgroup of 256 per entry: k_ens_weights' body at raw == 0, in the
// orders include/eqf_ensemble_output.h states (lane l owns the run [l R, (l + 1) R), R = ceil(P / 256)). The running sums go to the slot's own place (the kept
// weights), everything else to the entry's rows. If no entry is finite only scal is written. Every exit is uniform over the workgroup. grid (entries).
__global__ void __launch_bounds__(256) k_bens_weights(const BensOutArgs a) {
    __shared__ double sa[256], sb[256];
    __shared__ int sn[256];
    const BensOutIn& e = a.in[blockIdx.x];
    const int P = e.P, ldp = a.eb.ldp;
    const double* in = a.ob.ll + (size_t)blockIdx.x * ldp;
    double* w = a.ob.w + (size_t)blockIdx.x * ldp;
    double* cum = a.ob.cum_of(e.slot, ldp);
    double* scal = a.ob.scal + 4 * (size_t)blockIdx.x;
    const int l = threadIdx.x, R = (P + 255) / 256;
    const int lo = min(P, l * R), hi = min(P, lo + R);
    double m = -INFINITY;
    int nf = 0;
    for (int j = lo; j < hi; ++j) {
        const double v = in[j];
        if (isfinite(v)) {
            m = fmax(m, v);
            ++nf;
        }
    }
    sa[l] = m;
    sn[l] = nf;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (l < h) {
            sa[l] = fmax(sa[l], sa[l + h]);
            sn[l] += sn[l + h];
        }
        __syncthreads();
    }
    const double mx = sa[0];
    const int nfin = sn[0];
    __syncthreads();
    if (nfin == 0) {
        if (l == 0) {
            scal[0] = -INFINITY;
            scal[1] = 0.0;
            scal[2] = 0.0;
            scal[3] = 0.0;
        }
        return;
    }
    double t = 0.0;
    for (int j = lo; j < hi; ++j) {
        const double v = in[j];
        const double ej = isfinite(v) ? exp(v - mx) : 0.0;
        w[j] = ej;
        t += ej;
    }
    sa[l] = t;
    __syncthreads();
    if (l == 0) {
        double o = 0.0;
        for (int i = 0; i < 256; ++i) {
            sb[i] = o;
            o += sa[i];
        }
        sa[0] = o;
    }
    __syncthreads();
    const double sum = sa[0], off = sb[l];
    double run = 0.0, sq = 0.0;
    for (int j = lo; j < hi; ++j) {
        const double ej = w[j];
        run += ej;
        const double wj = ej / sum;
        cum[j] = (off + run) / sum;
        w[j] = wj;
        sq = __builtin_fma(wj, wj, sq);
    }
    __syncthreads();
    sa[l] = sq;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (l < h)
            sa[l] += sa[l + h];
        __syncthreads();
    }
    if (l == 0) {
        scal[0] = mx;
        scal[1] = sum;
        scal[2] = sa[0];
        scal[3] = (double)nfin;
    }
}

// ---- weightedResample's choice, a lane per new particle: u_k = U(word k & 3 of the block of counter (k >> 2, 0, 0, 1)) under the key (seed, stream) -
// k_ens_uniforms' value, computed by the lane that reads it (the four lanes of a block each compute it; the word is taken by selects, not by an index) - and
// k_ens_pick's binary search of the slot's running sums: the first j with c_j >= (u_k + k) / P_new, capped at P - 1. grid (ceil(Pnew_max / 256), entries).
__global__ void __launch_bounds__(256) k_bens_pick(const BensOutArgs a) {
    const BensOutIn& in = a.in[blockIdx.y];
    const int k = blockIdx.x * blockDim.x + threadIdx.x, P = in.P, Pnew = in.P_new, ldp = a.eb.ldp;
    if (k >= Pnew)
        return;
    unsigned long long x[4];
    philox4x64_10(in.seed, in.stream, (unsigned long long)(k >> 2), 0ull, 0ull, 1ull, x);
    const int wd = k & 3;
    const unsigned long long xw = wd == 0 ? x[0] : (wd == 1 ? x[1] : (wd == 2 ? x[2] : x[3]));
    const double* cum = a.ob.cum_of(in.slot, ldp);
    const double thr = (philox_unit(xw) + (double)k) / (double)Pnew;
    int lo = 0, hi = P - 1; // the answer lies in [lo, hi]; hi = P - 1 is the cap
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] >= thr)
            hi = mid;
        else
            lo = mid + 1;
    }
    a.ob.src[(size_t)blockIdx.y * ldp + k] = lo;
}

// ---- the gather, in two launches because it cannot be in place (a lane may read a source another lane has already overwritten): back == 0 copies plane
// blockIdx.y of particle src[k] of the cloud to particle k of the slot's second place G, back == 1 copies G's plane to the cloud. blockIdx.y < 23: a sensor
// plane; 23 + 3 i + c: coordinate c of the cloud's point i (i < N). grid (ceil(Pnew_max / 256), 23 + 3 Nmax, entries).
__global__ void __launch_bounds__(256) k_bens_gather(const BensOutArgs a, int back) {
    const BensOutIn& in = a.in[blockIdx.z];
    const int k = blockIdx.x * blockDim.x + threadIdx.x, ldp = a.eb.ldp;
    const int t = (int)blockIdx.y - 23, i = t / 3, c = t - 3 * i;
    if (k >= in.P_new || (t >= 0 && i >= in.N))
        return;
    double* cl = t < 0 ? a.eb.sens_of(in.slot) + (size_t)blockIdx.y * ldp : a.eb.pts_of(in.slot) + bens_pt(ldp, c, i, 0);
    double* g = a.ob.G_of(in.slot, ldp) + (size_t)(t < 0 ? (int)blockIdx.y : 23 + BATCH_L * c + i) * ldp;
    if (back)
        cl[k] = g[k];
    else
        g[k] = cl[a.ob.src[(size_t)blockIdx.z * ldp + k]];
}

// ---- estimateParticleCovariance: C = E E^T / P of every entry (n x n, leading dimension n, at cov + entry * 213 * 213) from the errors k_bens_errors left
// in the slot's E: k_ens_cov's body. One wave per 16 x 16 tile of the lower triangle, particles in ascending order in steps of 4 (the last step masked), the
// mirror image written from the same register; a diagonal tile writes only its lower half and its mirror. grid (tiles of the largest n, entries), one wave.
__global__ void __launch_bounds__(64) k_bens_cov(const BensArgs a, double* __restrict__ cov) {
    const BensIn& in = a.in[blockIdx.y];
    const int n = 21 + 3 * in.N, P = in.P, ldp = a.eb.ldp, nt = (n + 15) / 16;
    if ((int)blockIdx.x >= nt * (nt + 1) / 2)
        return;
    int bi, bj;
    batch_tri_tile(blockIdx.x, bi, bj);
    const int i0 = 16 * bi, j0 = 16 * bj;
    const double* E = a.eb.E_of(in.slot);
    double* Cout = cov + (size_t)blockIdx.y * BATCH_NMAX * BATCH_NMAX;
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
