// The ensemble's measurement side, host side (include/eqf_ensemble_output.h; kernels in eqf_ensemble_output.hpp). Included by eqf_hip.hip behind
// eqf_ensemble_host.hpp, whose struct, ens_alloc and synchronous style it shares; make_cam, camera_ok, blocks, spin_stream, HIPCHK are eqf_hip.hip's.
// No call here takes a context: the kernels run on the ensemble's own stream.
//
// Device data of these calls (allocated with the ensemble): d_lw = [max, sum, sum of squares, finite count | loglik[P] | weights[P]] so that one copy brings all
// results back, d_cum the running sums, d_yu the measurement (2 M doubles) or the uniforms (P_new doubles), d_idx the matched landmark places or the chosen
// indices, d_E (the error scratch, rebuilt by every call that uses it) the 2 M planes of eqf_ensemble_measure.
#pragma once
#include "eqf_ensemble_output.h"

namespace {
// the ensemble's place of every measured id; EQF_E_BAD_ARG for an id it does not hold or a repeated one
int ens_match_ids(const eqf_ensemble* e, const int* ids, int M, std::vector<int>& match) {
    std::vector<std::pair<int, int>> mine(e->N);
    for (int t = 0; t < e->N; ++t)
        mine[t] = {e->ids[t], t};
    std::sort(mine.begin(), mine.end());
    match.resize(M);
    std::vector<char> seen(e->N, 0);
    for (int j = 0; j < M; ++j) {
        const auto it = std::lower_bound(mine.begin(), mine.end(), std::make_pair(ids[j], -1));
        if (it == mine.end() || it->first != ids[j] || seen[it->second])
            return EQF_E_BAD_ARG;
        seen[it->second] = 1;
        match[j] = it->second;
    }
    return 0;
}
// what measure and likelihood check before anything else
int ens_output_front(const eqf_ensemble* e, const eqvio_camera* cam, const int* ids, int M, std::vector<int>& match) {
    if (!e || !cam || !camera_ok(cam) || M < 0 || (M > 0 && !ids) || e->P < 1)
        return EQF_E_BAD_ARG;
    return ens_match_ids(e, ids, M, match);
}
} // namespace

int eqf_ensemble_measure(eqf_ensemble* e, const eqvio_camera* cam, const int* ids, int M, double* y_out) {
    std::vector<int> match;
    EQFCHK(ens_output_front(e, cam, ids, M, match));
    if (M > 0 && !y_out)
        return EQF_E_BAD_ARG;
    if (M == 0)
        return 0;
    const int P = e->P;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpy(e->d_idx, match.data(), sizeof(int) * M, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_ens_measure, dim3(blocks(P, 256), M), dim3(256), 0, e->stream, P, make_cam(cam), e->d_idx, e->d_pts[e->cur], e->Nalloc(), e->ldp, e->d_E);
    HIPCHK(hipGetLastError());
    ++e->launches;
    EQFCHK(spin_stream(e->stream));
    e->h.resize(2 * (size_t)M * P);
    HIPCHK(hipMemcpy2D(e->h.data(), sizeof(double) * P, e->d_E, sizeof(double) * e->ldp, sizeof(double) * P, 2 * (size_t)M, hipMemcpyDeviceToHost));
    for (int k = 0; k < P; ++k)
        for (int r = 0; r < 2 * M; ++r)
            y_out[2 * (size_t)M * k + r] = e->h[(size_t)r * P + k];
    return 0;
}

int eqf_ensemble_likelihood(eqf_ensemble* e, const eqvio_camera* cam, const int* ids, const double* y, int M, double meas_var, double* loglik, double* weights,
                            double* logsumexp, double* ess) {
    std::vector<int> match;
    EQFCHK(ens_output_front(e, cam, ids, M, match));
    if ((M > 0 && !y) || !(meas_var > 0.0) || !std::isfinite(meas_var))
        return EQF_E_BAD_ARG;
    const int P = e->P;
    HIPCHK(hipSetDevice(e->device));
    e->w_valid = false; // from here on the kept weights are being replaced
    if (M > 0) {
        HIPCHK(hipMemcpy(e->d_idx, match.data(), sizeof(int) * M, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(e->d_yu, y, sizeof(double) * 2 * M, hipMemcpyHostToDevice));
    }
    double *d_ll = e->d_lw + 4, *d_w = e->d_lw + 4 + P;
    hipLaunchKernelGGL(k_ens_loglik, dim3(blocks(P, 32)), dim3(256), 0, e->stream, P, M, make_cam(cam), e->d_idx, e->d_yu, meas_var, e->d_pts[e->cur], e->Nalloc(), e->ldp, d_ll);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_ens_weights, dim3(1), dim3(256), 0, e->stream, P, 0, d_ll, d_w, e->d_cum, e->d_lw);
    HIPCHK(hipGetLastError());
    e->launches += 2;
    EQFCHK(spin_stream(e->stream));
    e->h.resize(4 + 2 * (size_t)P);
    HIPCHK(hipMemcpy(e->h.data(), e->d_lw, sizeof(double) * (4 + 2 * (size_t)P), hipMemcpyDeviceToHost));
    const double mx = e->h[0], sum = e->h[1], sq = e->h[2];
    if (e->h[3] == 0.0)
        return EQF_E_NONFINITE; // nothing kept
    if (loglik)
        std::copy(e->h.begin() + 4, e->h.begin() + 4 + P, loglik);
    if (weights)
        std::copy(e->h.begin() + 4 + P, e->h.begin() + 4 + 2 * (size_t)P, weights);
    if (logsumexp)
        *logsumexp = mx + std::log(sum);
    if (ess)
        *ess = 1.0 / sq;
    e->w_valid = true;
    return 0;
}

namespace {
// the weights eqf_ensemble_resample_weighted picks by: the caller's (finite, >= 0, not all zero) or the kept ones
int ens_weights_ok(const eqf_ensemble* e, const double* weights) {
    if (weights) {
        double s = 0.0;
        for (int j = 0; j < e->P; ++j) {
            if (!(weights[j] >= 0.0) || !std::isfinite(weights[j]))
                return EQF_E_BAD_ARG;
            s += weights[j];
        }
        if (!(s > 0.0) || !std::isfinite(s))
            return EQF_E_BAD_ARG;
    } else if (!e->w_valid)
        return EQF_E_BAD_ARG;
    return 0;
}
// eqf_ensemble_resample_weighted behind its copy of u: d_yu holds the P_new uniforms (uploaded, or generated there by eqf_ensemble_resample_weighted_seeded)
int ens_resample_from_u(eqf_ensemble* e, int P_new, const double* weights, int* src_out) {
    const int P = e->P, N = e->N;
    if (weights) {
        double* d_w = e->d_lw + 4 + P;
        HIPCHK(hipMemcpy(d_w, weights, sizeof(double) * P, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_ens_weights, dim3(1), dim3(256), 0, e->stream, P, 1, d_w, d_w, e->d_cum, e->d_lw);
        HIPCHK(hipGetLastError());
        ++e->launches;
    }
    hipLaunchKernelGGL(k_ens_pick, dim3(blocks(P_new, 256)), dim3(256), 0, e->stream, P, P_new, e->d_cum, e->d_yu, e->d_idx);
    HIPCHK(hipGetLastError());
    ++e->launches;
    if (N > 0) {
        hipLaunchKernelGGL(k_ens_gather, dim3(blocks(P_new, 256), 3 * N), dim3(256), 0, e->stream, P_new, e->d_idx, e->d_pts[e->cur], e->d_pts[1 - e->cur], e->Nalloc(), N, e->ldp);
        HIPCHK(hipGetLastError());
        ++e->launches;
    }
    EQFCHK(spin_stream(e->stream));
    std::vector<int> src(P_new);
    HIPCHK(hipMemcpy(src.data(), e->d_idx, sizeof(int) * P_new, hipMemcpyDeviceToHost));
    if (N > 0)
        e->cur = 1 - e->cur;
    std::vector<double> sens(23 * (size_t)P_new);
    for (int k = 0; k < P_new; ++k)
        std::copy(e->sensor.begin() + 23 * (size_t)src[k], e->sensor.begin() + 23 * (size_t)src[k] + 23, sens.begin() + 23 * (size_t)k);
    e->sensor.swap(sens);
    e->P = P_new;
    if (src_out)
        std::copy(src.begin(), src.end(), src_out);
    return 0;
}
} // namespace

int eqf_ensemble_resample_weighted(eqf_ensemble* e, int P_new, const double* weights, const double* u, int* src_out) {
    if (!e || !u || P_new < 1 || e->P < 1)
        return EQF_E_BAD_ARG;
    if (P_new > e->Pcap)
        return EQF_E_CAPACITY;
    for (int k = 0; k < P_new; ++k)
        if (!(u[k] >= 0.0 && u[k] < 1.0))
            return EQF_E_BAD_ARG;
    EQFCHK(ens_weights_ok(e, weights));
    HIPCHK(hipSetDevice(e->device));
    e->w_valid = false;
    HIPCHK(hipMemcpy(e->d_yu, u, sizeof(double) * P_new, hipMemcpyHostToDevice));
    return ens_resample_from_u(e, P_new, weights, src_out);
}
