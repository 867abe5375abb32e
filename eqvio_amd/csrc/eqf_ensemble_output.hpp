// eqf_ensemble_output.hpp - kernels of the ensemble's measurement side (include/eqf_ensemble_output.h): every particle's measurement, its log-likelihood, the
// normalised weights with their running sums, and weightedResample's index choice. gfx950 only. Included by eqf_hip.hip behind eqf_ensemble.hpp, whose plane
// layout pts[(c * Ncap + i) * ldp + k] (ens_at) it reads; cam_project is eqf_math.hpp's, the camera passed by value. No kernel or device function of another file
// is changed by it, and no kernel here talks to another workgroup.
#pragma once
#include "eqf_ensemble.hpp"

namespace eqf {

// meas[(2 j + c) * ldp + k] = projectPoint(point match[j] of particle k)[c]: a lane per (particle, measured landmark), loads and stores contiguous in k.
// grid (ceil(P / 256), M).
__global__ void __launch_bounds__(256) k_ens_measure(int P, Cam cam, const int* __restrict__ match, const double* __restrict__ pts, int NcapE, int ldp, double* __restrict__ meas) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (k >= P)
        return;
    const int t = match[j];
    const V3 p{pts[ens_at(NcapE, ldp, 0, t, k)], pts[ens_at(NcapE, ldp, 1, t, k)], pts[ens_at(NcapE, ldp, 2, t, k)]};
    double u, v;
    cam_project(cam, p, u, v);
    meas[(size_t)(2 * j) * ldp + k] = u;
    meas[(size_t)(2 * j + 1) * ldp + k] = v;
}

// ll[k] = -1/2 (sum_j |y_j - projectPoint(p_{k, match[j]})|^2) / var, -infinity where that is not finite. k_ens_rowsumsq's pattern: a workgroup takes 32 particles,
// lane group g of its 8 sums the landmarks j = g (mod 8) in ascending order (u then v) and the 8 partial sums are added in one fixed tree, so a particle's value
// depends on its own points alone - the same bits wherever it stands and whatever P is - without one lane walking M divisions alone. M = 0 gives +0.0.
// grid ceil(P / 32).
__global__ void __launch_bounds__(256) k_ens_loglik(int P, int M, Cam cam, const int* __restrict__ match, const double* __restrict__ y, double var, const double* __restrict__ pts,
                                                    int NcapE, int ldp, double* __restrict__ ll) {
    __shared__ double sp[8][33];
    const int r = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int k = blockIdx.x * 32 + r, kc = min(k, P - 1);
    double s = 0.0;
    for (int j = g; j < M; j += 8) {
        const int t = match[j];
        const V3 p{pts[ens_at(NcapE, ldp, 0, t, kc)], pts[ens_at(NcapE, ldp, 1, t, kc)], pts[ens_at(NcapE, ldp, 2, t, kc)]};
        double u, v;
        cam_project(cam, p, u, v);
        const double eu = y[2 * j] - u, ev = y[2 * j + 1] - v;
        s = __builtin_fma(eu, eu, s);
        s = __builtin_fma(ev, ev, s);
    }
    sp[g][r] = s;
    __syncthreads();
    if (g == 0 && k < P) {
        const double tot = ((sp[0][r] + sp[1][r]) + (sp[2][r] + sp[3][r])) + ((sp[4][r] + sp[5][r]) + (sp[6][r] + sp[7][r]));
        const double v = 0.0 - 0.5 * tot / var;
        ll[k] = isfinite(v) ? v : -INFINITY;
    }
}

// The normalised weights w[P], their running sums cum[P] and scal = (max, sum, sum of squares, number of finite entries), by ONE workgroup of 256 in the orders
// the header states. raw == 0: in = log-likelihoods, e_j = exp(in_j - max) (0 where in_j is not finite); raw == 1: in = the caller's weights (checked on the host:
// finite, >= 0, not all zero), e_j = in_j and max is reported as 0. Lane l owns the contiguous run [l R, (l + 1) R), R = ceil(P / 256). If no entry is finite only
// scal is written. in and w may be the same array (a lane reads and writes its own run only). grid 1.
__global__ void __launch_bounds__(256) k_ens_weights(int P, int raw, const double* in, double* w, double* __restrict__ cum, double* __restrict__ scal) {
    __shared__ double sa[256], sb[256];
    __shared__ int sn[256];
    const int l = threadIdx.x, R = (P + 255) / 256;
    const int lo = min(P, l * R), hi = min(P, lo + R);
    // the maximum (order-free) and the number of finite entries
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
    const double mx = raw ? 0.0 : sa[0];
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
    // e_j into w, the run totals t_l
    double t = 0.0;
    for (int j = lo; j < hi; ++j) {
        const double v = in[j];
        const double ej = raw ? v : (isfinite(v) ? exp(v - mx) : 0.0);
        w[j] = ej;
        t += ej;
    }
    sa[l] = t;
    __syncthreads();
    // o_l = t_0 + ... + t_(l-1) in ascending l, sum = o_255 + t_255: one lane, 256 additions
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
    // running sums, normalised weights, squares
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

// weightedResample's choice: src[k] = the first j with cum[j] >= (u[k] + k) / Pnew, or P - 1 if there is none - a binary search of the non-decreasing running
// sums, a lane per new particle. grid ceil(Pnew / 256).
__global__ void __launch_bounds__(256) k_ens_pick(int P, int Pnew, const double* __restrict__ cum, const double* __restrict__ u, int* __restrict__ src) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Pnew)
        return;
    const double thr = (u[k] + (double)k) / (double)Pnew;
    int lo = 0, hi = P - 1; // the answer lies in [lo, hi]; hi = P - 1 is the cap
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] >= thr)
            hi = mid;
        else
            lo = mid + 1;
    }
    src[k] = lo;
}

} // namespace eqf
