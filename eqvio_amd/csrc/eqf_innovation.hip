// EQF_OPT_INNOVATION_STATS: the kernel behind the update tail (eqf_innovation.hpp says what it computes and why it is a translation unit of its own).
#include "eqf_innovation.hpp"

namespace eqf {

__global__ void __launch_bounds__(INNOV_T) k_innovation_stats(const InnovArgs a) {
    if (a.spec && *a.spec == a.spec_seq)
        return; // cancelled speculative tail: the slot keeps its old number
    __shared__ double s_nis[INNOV_T / 64], s_log[INNOV_T / 64];
    __shared__ int s_dof[INNOV_T / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool stalled = a.stall_seq > 0 && __hip_atomic_load(a.flags + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.stall_seq;
    double nis = 0.0, slog = 0.0;
    int dof = 0;
    if (!stalled) {
        const double* zrow = a.W + (a.rows - 1);
        for (int j = tid; j < a.m; j += INNOV_T) {
            bool live = true;
            if (a.removed) {
                const int i = a.lmidx[j >> 1];
                live = i < 0 || i >= a.nlm || a.removed[i] == 0;
            }
            if (live) {
                const double z = zrow[(size_t)j * a.ldz];
                const double d = a.tiles[(size_t)1024 * (j >> 5) + 33 * (j & 31)];
                nis = fma(z, z, nis);
                slog += log(d);
                ++dof;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        nis += __shfl_xor(nis, o, 64);
        slog += __shfl_xor(slog, o, 64);
        dof += __shfl_xor(dof, o, 64);
    }
    if (lane == 0)
        s_nis[wave] = nis, s_log[wave] = slog, s_dof[wave] = dof;
    __syncthreads();
    if (tid == 0) {
        a.out->nis = (s_nis[0] + s_nis[1]) + (s_nis[2] + s_nis[3]);
        a.out->logdet = -2.0 * ((s_log[0] + s_log[1]) + (s_log[2] + s_log[3]));
        a.out->dof = (s_dof[0] + s_dof[1]) + (s_dof[2] + s_dof[3]);
        __threadfence_system();
        __hip_atomic_store(&a.out->seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

void launch_innovation_kernel(const InnovArgs& a, hipStream_t stream) { hipLaunchKernelGGL(k_innovation_stats, dim3(1), dim3(INNOV_T), 0, stream, a); }

} // namespace eqf
