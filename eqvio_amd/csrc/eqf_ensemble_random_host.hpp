// The ensemble's seeded draws, host side (include/eqf_ensemble_random.h; kernels in eqf_ensemble_random.hpp). Included by eqf_hip.hip behind
// eqf_ensemble_output_host.hpp: every seeded call is the unseeded call's own body (ens_sample_from_xi, ens_resample_from_u, eqf_ensemble_integrate) behind a
// generator launch that fills the device array the caller's numbers used to be copied into.
//
// Device data: sample_seeded writes d_xi, resample_weighted_seeded d_yu (where the unseeded calls' copies land); normals, and through it integrate_seeded, use d_E,
// the error scratch that every call rebuilds before it reads it (ldp * npcap >= rows * P doubles); uniforms uses d_yu (>= Pcap doubles).
#pragma once
#include "eqf_ensemble_random.h"

namespace {
void ens_launch_normals(eqf_ensemble* e, hipStream_t st, unsigned long long seed, unsigned long long stream, int rows, int P, double* d_out) {
    const long long lanes = (long long)((rows + 3) / 4) * P;
    hipLaunchKernelGGL(k_ens_normals, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, rows, P, seed, stream, d_out);
    ++e->launches;
}
void ens_launch_uniforms(eqf_ensemble* e, unsigned long long seed, unsigned long long stream, int count, double* d_out) {
    hipLaunchKernelGGL(k_ens_uniforms, dim3(blocks(blocks(count, 4), 64)), dim3(64), 0, e->stream, count, seed, stream, d_out);
    ++e->launches;
}
} // namespace

int eqf_ensemble_normals(eqf_ensemble* e, unsigned long long seed, unsigned long long stream, int rows, int P, double* out) {
    if (!e || !out || rows < 1 || P < 1)
        return EQF_E_BAD_ARG;
    if (rows > e->npcap || P > e->Pcap)
        return EQF_E_CAPACITY;
    HIPCHK(hipSetDevice(e->device));
    ens_launch_normals(e, e->stream, seed, stream, rows, P, e->d_E);
    HIPCHK(hipGetLastError());
    EQFCHK(spin_stream(e->stream));
    HIPCHK(hipMemcpy(out, e->d_E, sizeof(double) * (size_t)rows * P, hipMemcpyDeviceToHost));
    return 0;
}

int eqf_ensemble_uniforms(eqf_ensemble* e, unsigned long long seed, unsigned long long stream, int count, double* out) {
    if (!e || !out || count < 1)
        return EQF_E_BAD_ARG;
    if (count > e->Pcap)
        return EQF_E_CAPACITY;
    HIPCHK(hipSetDevice(e->device));
    ens_launch_uniforms(e, seed, stream, count, e->d_yu);
    HIPCHK(hipGetLastError());
    EQFCHK(spin_stream(e->stream));
    HIPCHK(hipMemcpy(out, e->d_yu, sizeof(double) * count, hipMemcpyDeviceToHost));
    return 0;
}

int eqf_ensemble_sample_seeded(eqf_ensemble* e, eqf_ctx* c, int P, unsigned long long seed, unsigned long long stream) {
    EQFCHK(ens_check_ctx(e, c));
    if (P < 1)
        return EQF_E_BAD_ARG;
    if (P > e->Pcap || c->N > e->Ncap)
        return EQF_E_CAPACITY;
    EQFCHK(enter(c));
    EQFCHK(join_observer(c));
    const EnsCountersKept keep(c);
    ens_launch_normals(e, c->stream, seed, stream, c->n(), P, e->d_xi); // n <= 21 + 3 Ncap rows: d_xi's room
    HIPCHK(hipGetLastError());
    return ens_sample_from_xi(e, c, P);
}

int eqf_ensemble_resample_weighted_seeded(eqf_ensemble* e, int P_new, const double* weights, unsigned long long seed, unsigned long long stream, int* src_out) {
    if (!e || P_new < 1 || e->P < 1)
        return EQF_E_BAD_ARG;
    if (P_new > e->Pcap)
        return EQF_E_CAPACITY;
    EQFCHK(ens_weights_ok(e, weights));
    HIPCHK(hipSetDevice(e->device));
    e->w_valid = false;
    ens_launch_uniforms(e, seed, stream, P_new, e->d_yu);
    HIPCHK(hipGetLastError());
    return ens_resample_from_u(e, P_new, weights, src_out);
}

int eqf_ensemble_integrate_seeded(eqf_ensemble* e, const double* imu13, double dt, const double* sigma6, unsigned long long seed, unsigned long long stream) {
    if (!e || !imu13 || !sigma6)
        return EQF_E_BAD_ARG;
    const int P = e->P;
    if (P == 0)
        return 0;
    std::vector<double> off(6 * (size_t)P);
    EQFCHK(eqf_ensemble_normals(e, seed, stream, 6, P, off.data()));
    for (int k = 0; k < P; ++k)
        for (int c = 0; c < 6; ++c)
            off[c + 6 * (size_t)k] = sigma6[c] * off[c + 6 * (size_t)k];
    return eqf_ensemble_integrate(e, imu13, dt, off.data());
}
