// eqf_ensemble_random.hpp - the ensemble's random draws on the device (include/eqf_ensemble_random.h): Philox4x64-10, a counter-based generator, and the two
// kernels that turn its words into standard normals and uniforms. gfx950 only. Included by eqf_hip.hip behind eqf_ensemble_output.hpp. A value depends on
// (seed, stream, row, particle) alone: every lane computes its own counter's block and nothing else - no state, no LDS, no word passed between lanes, no kernel
// that talks to another workgroup. No kernel or device function of another file is changed by it.
#pragma once
#include "eqf_ensemble_output.hpp"

namespace eqf {

// Philox4x64-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; numpy's np.random.Philox): the block of counter (c0, c1, c2, c3) under the
// key (k0, k1). A round is c <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is bumped after each round.
__device__ __forceinline__ void philox4x64_10(unsigned long long k0, unsigned long long k1, unsigned long long c0, unsigned long long c1, unsigned long long c2, unsigned long long c3,
                                              unsigned long long x[4]) {
    constexpr unsigned long long M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull, W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long hi0 = __umul64hi(M0, c0), lo0 = M0 * c0, hi1 = __umul64hi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    x[0] = c0;
    x[1] = c1;
    x[2] = c2;
    x[3] = c3;
}

// U(x) = (2 (x >> 12) + 1) 2^-53: the odd multiples of 2^-53 - exact in fp64 (2 (x >> 12) + 1 < 2^53), strictly inside (0, 1), U(x) + U(~x) = 1
__device__ __forceinline__ double philox_unit(unsigned long long x) { return (double)(2ull * (x >> 12) + 1ull) * 0x1p-53; }

// Box-Muller of the word pair (a, b): r = sqrt(-2 log U(a)), (r cospi(2 U(b)), r sinpi(2 U(b))). 2 U is exact, so sincospi gets an exact argument.
__device__ __forceinline__ void philox_normal_pair(unsigned long long a, unsigned long long b, double& z0, double& z1) {
    const double r = sqrt(-2.0 * log(philox_unit(a)));
    double s, c;
    sincospi(2.0 * philox_unit(b), &s, &c);
    z0 = r * c;
    z1 = r * s;
}

// xi[r + rows * k], rows x P column-major, standard normals: a lane per (row block j, particle k), the row block the fast index, so that a wave writes a contiguous
// run of one column. Rows 4 j .. 4 j + 3 of particle k are the block of counter (j, k, 0, 0) under the key (seed, stream): words (x0, x1) give rows 4 j and 4 j + 1,
// words (x2, x3) rows 4 j + 2 and 4 j + 3. Rows beyond `rows` in the last block are not stored. grid ceil(ceil(rows / 4) P / 256).
__global__ void __launch_bounds__(256) k_ens_normals(int rows, int P, unsigned long long seed, unsigned long long stream, double* __restrict__ xi) {
    const int nb = (rows + 3) >> 2;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)nb * P)
        return;
    const int k = (int)(t / nb), j = (int)(t - (long long)k * nb);
    unsigned long long x[4];
    philox4x64_10(seed, stream, (unsigned long long)j, (unsigned long long)k, 0ull, 0ull, x);
    double z0, z1, z2, z3;
    philox_normal_pair(x[0], x[1], z0, z1);
    philox_normal_pair(x[2], x[3], z2, z3);
    const int r = 4 * j;
    double* col = xi + (size_t)rows * k + r;
    col[0] = z0; // r < rows: j < nb
    if (r + 1 < rows)
        col[1] = z1;
    if (r + 2 < rows)
        col[2] = z2;
    if (r + 3 < rows)
        col[3] = z3;
}

// u[i] = U(word i & 3 of the block of counter (i >> 2, 0, 0, 1)) under the key (seed, stream): a lane per four draws, one wave per workgroup (the largest
// request, a capacity of particles, is a few hundred lanes). grid ceil(ceil(count / 4) / 64).
__global__ void __launch_bounds__(64) k_ens_uniforms(int count, unsigned long long seed, unsigned long long stream, double* __restrict__ u) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, i = 4 * t;
    if (t >= ((count + 3) >> 2))
        return;
    unsigned long long x[4];
    philox4x64_10(seed, stream, (unsigned long long)t, 0ull, 0ull, 1ull, x);
    u[i] = philox_unit(x[0]);
    if (i + 1 < count)
        u[i + 1] = philox_unit(x[1]);
    if (i + 2 < count)
        u[i + 2] = philox_unit(x[2]);
    if (i + 3 < count)
        u[i + 3] = philox_unit(x[3]);
}

} // namespace eqf
