// eqf_batch_ensemble.hpp - kernels of the particle ensembles against batch slots (include/eqf_batch_ensemble.h): one cloud per slot of a filter batch, every
// listed cloud sampled, moved or judged by the same launch. gfx950 only. Included by eqf_hip.hip behind eqf_ensemble_random.hpp. It calls eqf_math.hpp,
// eqf_kernels.hpp's sensor_action / group_inv / chart_fwd / chart_bwd / ld3 / ldq, eqf_batch.hpp's BatchBufs and plane constants and eqf_ensemble_random.hpp's
// philox4x64_10 / philox_normal_pair as they stand; no kernel or device function of another file is changed by it.
// No kernel here talks to another workgroup: the pivot flag of an entry is written by k_bens_factor and read by the launches behind it.
//
// Layouts, per slot s (BensBufs): sensor planes sens[(23 s + c) ldp + k] (coordinate c of eqvio_types.h's 23, particle k), point planes
// pts[((3 s + c) 64 + i) ldp + k], error coordinates E[(214 s + r) ldp + k] ("particle-major": a lane per particle reads and writes coalesced), the factor
// L[(s 214 + c) 216 + r] column-major, lower triangle (the upper one is zero). The slot's Sigma and landmark planes are read in place from the batch.
#pragma once
#include "eqf_batch.hpp"
#include "eqf_ensemble_random.hpp"

namespace eqf {

constexpr int BENS_NP = BATCH_NMAX + 1; // 214: the largest padded dimension
constexpr int BENS_LDL = 216;           // leading dimension of L
constexpr int BENS_PW = 16;             // panel width of the factorisation, tile of the solve and the product
constexpr int BENS_PLD = 228;           // LDS panel column stride: rows k0 .. np (<= 214) and the zero rows of the last 16-row tile (< 224 + 4)
constexpr int BENS_XR = 224;            // rows of a wave's LDS tile (14 tiles of 16 >= 214; 4 ceil(213 / 4) = 216 rows of normals)

struct BensBufs {
    int ldp; // particles' leading dimension
    double *sens, *pts, *E, *L, *out;
    int* flag;
    __host__ __device__ double* sens_of(int slot) const { return sens + (size_t)slot * 23 * ldp; }
    __host__ __device__ double* pts_of(int slot) const { return pts + (size_t)slot * 3 * BATCH_L * ldp; }
    __host__ __device__ double* E_of(int slot) const { return E + (size_t)slot * BENS_NP * ldp; }
    __host__ __device__ double* L_of(int slot) const { return L + (size_t)slot * BENS_NP * BENS_LDL; }
};
// one entry of a call, prepared by the host
struct BensIn {
    int slot, cur, N, P; // the slot, its current buffers and landmarks; the particles the launch runs over
    int chart, noisy;    // the slot's chart; integrate: 1 with sigma6
    unsigned long long seed, stream;
    SensorState xi0;
    GroupSensor X;
    double imu[13], dt, sigma6[6];
    int match[BATCH_L]; // errors: the filter's landmark i is the cloud's landmark match[i]
};
struct BensArgs {
    BatchBufs buf;
    BensBufs eb;
    const BensIn* in;
};

__device__ __forceinline__ size_t bens_pt(int ldp, int c, int i, int k) { return ((size_t)c * BATCH_L + i) * ldp + k; }
__device__ __forceinline__ SensorState bens_load_sensor(const double* sp, int ldp, int k) {
    double s[23];
#pragma unroll
    for (int c = 0; c < 23; ++c)
        s[c] = sp[(size_t)c * ldp + k];
    SensorState r;
    r.bgyr = v3(s[0], s[1], s[2]);
    r.bacc = v3(s[3], s[4], s[5]);
    r.pose = Pose{Qt{s[6], s[7], s[8], s[9]}, v3(s[10], s[11], s[12])};
    r.vel = v3(s[13], s[14], s[15]);
    r.cam = Pose{Qt{s[16], s[17], s[18], s[19]}, v3(s[20], s[21], s[22])};
    return r;
}
__device__ __forceinline__ void bens_store_sensor(const SensorState& r, double* sp, int ldp, int k) {
    const double s[23] = {r.bgyr.x, r.bgyr.y,   r.bgyr.z,   r.bacc.x,   r.bacc.y, r.bacc.z, r.pose.R.w, r.pose.R.x, r.pose.R.y, r.pose.R.z, r.pose.x.x, r.pose.x.y,
                          r.pose.x.z, r.vel.x,  r.vel.y,    r.vel.z,    r.cam.R.w, r.cam.R.x, r.cam.R.y, r.cam.R.z,  r.cam.x.x,  r.cam.x.y,  r.cam.x.z};
#pragma unroll
    for (int c = 0; c < 23; ++c)
        sp[(size_t)c * ldp + k] = s[c];
}
// so3_Vinv without its cancellation: the (th / 2) cot(th / 2) form of the coefficient (eqf_ensemble_host.hpp's ens_Vinv, restated for the device; so3_Vinv
// itself stays as it is)
__device__ __forceinline__ M3 bens_Vinv(V3 om) {
    const double th = norm(om);
    if (th < 1e-4)
        return so3_Vinv(om);
    const double half = 0.5 * th;
    const double Cc = (1.0 - half * cos(half) / sin(half)) / (th * th);
    const M3 Om = skew(om);
    return m3_identity() - 0.5 * Om + Cc * (Om * Om);
}
__device__ __forceinline__ void bens_se3_log(const Pose& P, V3& om, V3& v) {
    om = so3_log(P.R);
    v = bens_Vinv(om) * P.x;
}

// ---- the factor: one workgroup per entry. L L^T = Sigma padded to the even dimension np with a unit diagonal entry, 16-column panels in LDS (k_batch_nees'
// right-looking scheme: scalar panel, trailing update in 16 x 16 MFMA tiles), L left in the ensemble's own storage, flag[entry] = 1 when a pivot was <= 0 or
// not finite (L then holds the panels before it). grid (entries).
__global__ void __launch_bounds__(BATCH_T) k_bens_factor(const BensArgs a) {
    __shared__ double Pn[BENS_PLD * BENS_PW];
    const BensIn& in = a.in[blockIdx.x];
    const int tid = threadIdx.x, ld = a.buf.ld, ldl = BENS_LDL;
    const int n = 21 + 3 * in.N, np = n + (n & 1);
    const double* S = a.buf.sig_of(in.slot, in.cur);
    double* Z = a.eb.L_of(in.slot);
    for (int t = tid; t < np * np; t += BATCH_T) {
        const int r = t % np, c = t / np;
        Z[r + (size_t)c * ldl] = r < c ? 0.0 : (r < n && c < n ? S[r + (size_t)c * ld] : (r == c ? 1.0 : 0.0));
    }
    __syncthreads();
    bool fail = false;
    for (int k0 = 0; k0 < np && !fail; k0 += BENS_PW) {
        const int w = min(BENS_PW, np - k0), R = np - k0; // panel columns and rows
        for (int t = tid; t < BENS_PLD * BENS_PW; t += BATCH_T) {
            const int r = t % BENS_PLD, c = t / BENS_PLD;
            Pn[t] = (r < R && c < w && r >= c) ? Z[k0 + r + (size_t)(k0 + c) * ldl] : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < w; ++j) {
            const double d = Pn[j + j * BENS_PLD]; // the same value in every lane: the exit is uniform
            if (!(d > 0.0) || !(d - d == 0.0)) {
                fail = true;
                break;
            }
            const double ljj = sqrt(d);
            for (int r = j + 1 + tid; r < R; r += BATCH_T)
                Pn[r + j * BENS_PLD] /= ljj;
            __syncthreads();
            for (int r = j + 1 + tid; r < R; r += BATCH_T) {
                const double lrj = Pn[r + j * BENS_PLD];
                for (int c = j + 1; c < w && c <= r; ++c)
                    Pn[r + c * BENS_PLD] -= lrj * Pn[c + j * BENS_PLD];
            }
            if (tid == 0)
                Pn[j + j * BENS_PLD] = ljj;
            __syncthreads();
        }
        if (fail)
            break;
        for (int t = tid; t < R * w; t += BATCH_T) {
            const int r = t % R, c = t / R;
            if (r >= c)
                Z[k0 + r + (size_t)(k0 + c) * ldl] = Pn[r + c * BENS_PLD];
        }
        const int t0 = k0 + BENS_PW; // first trailing row and column
        if (t0 < np) {               // then w == 16: the product's K is the whole panel
            const int nt = (np - t0 + 15) / 16, ntiles = nt * (nt + 1) / 2;
            const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
            for (int t = wave; t < ntiles; t += BATCH_T / 64) {
                int bi, bj;
                batch_tri_tile(t, bi, bj);
                const d4 acc = mfma16_nt(Pn + BENS_PW + 16 * bi, BENS_PLD, Pn + BENS_PW + 16 * bj, BENS_PLD);
                const int r = t0 + 16 * bi + lr;
                for (int q = 0; q < 4; ++q) {
                    const int c = t0 + 16 * bj + lk + 4 * q;
                    if (r < np && c < np && r >= c)
                        Z[r + (size_t)c * ldl] -= acc[q];
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0)
        a.eb.flag[blockIdx.x] = fail ? 1 : 0;
}

// ---- eps = L Xi with Xi = normals(seed, stream, n, P) generated here: one wave per 16 particles. The wave first fills its 16 columns of Xi in LDS (a lane
// per (row block, particle): k_ens_normals' counter map, every value computed once), then runs over the 16-row tiles of L, k ascending in steps of 4 up to the
// tile's last row. E particle-major. grid (ceil(Pmax / 16), entries), one wave.
__global__ void __launch_bounds__(64) k_bens_sample_eps(const BensArgs a) {
    __shared__ double Xs[BENS_XR * 16];
    const BensIn& in = a.in[blockIdx.y];
    const int P = in.P, p0 = blockIdx.x * 16;
    if (a.eb.flag[blockIdx.y] || p0 >= P)
        return;
    const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4, ldp = a.eb.ldp;
    const int n = 21 + 3 * in.N, nb = (n + 3) >> 2;
    const double* L = a.eb.L_of(in.slot);
    double* E = a.eb.E_of(in.slot);
    for (int t = lane; t < nb * 16; t += 64) {
        const int j = t >> 4, p = t & 15;
        unsigned long long x[4];
        philox4x64_10(in.seed, in.stream, (unsigned long long)j, (unsigned long long)(p0 + p), 0ull, 0ull, x);
        double z0, z1, z2, z3;
        philox_normal_pair(x[0], x[1], z0, z1);
        philox_normal_pair(x[2], x[3], z2, z3);
        Xs[(4 * j) * 16 + p] = z0;
        Xs[(4 * j + 1) * 16 + p] = z1;
        Xs[(4 * j + 2) * 16 + p] = z2;
        Xs[(4 * j + 3) * 16 + p] = z3;
    }
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 16) {
        const int row = i0 + lr, rowc = min(row, n - 1), kend = min(n, i0 + 16);
        d4 acc = {0, 0, 0, 0};
        for (int k0 = 0; k0 < kend; k0 += 4) {
            const int k = k0 + lk, kc = min(k, n - 1); // k < 4 nb: inside the tile of normals
            const double lv = L[rowc + (size_t)kc * BENS_LDL], xv = Xs[k * 16 + lr];
            const double av = (row < n && k <= row) ? lv : 0.0; // L[i0 + lr][k], lower triangle (k <= row < n)
            const double bv = k < n ? xv : 0.0;                 // Xi[k][p0 + lr]
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(bv, av, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int pp = p0 + lk + 4 * q;
            if (row < n && pp < P)
                E[pp + (size_t)row * ldp] = acc[q];
        }
    }
}

// ---- particle k of entry e from its eps: stateGroupAction(X, stateChart^-1(eps_k ; xi0)). blockIdx.y == 0: the sensor part, a lane per particle
// (sensorChart_std.inv / sensorChart_normal.inv, VIOState.cpp:114-121, 138-151, then sensorStateGroupAction); blockIdx.y == 1 + i: landmark i, a lane per
// particle, p = Q_i^-1 chart^-1(eps_k,i ; q0_i). grid (ceil(Pmax / 256), 1 + Nmax, entries).
__global__ void __launch_bounds__(BATCH_T) k_bens_sample_apply(const BensArgs a) {
    const BensIn& in = a.in[blockIdx.z];
    const int k = blockIdx.x * BATCH_T + threadIdx.x, ldp = a.eb.ldp;
    if (a.eb.flag[blockIdx.z] || k >= in.P || (int)blockIdx.y > in.N)
        return;
    const double* E = a.eb.E_of(in.slot);
    if (blockIdx.y == 0) {
        double e[21];
#pragma unroll
        for (int r = 0; r < 21; ++r)
            e[r] = E[k + (size_t)r * ldp];
        const SensorState& xi0 = in.xi0;
        SensorState s;
        s.bgyr = xi0.bgyr + v3(e[0], e[1], e[2]);
        s.bacc = xi0.bacc + v3(e[3], e[4], e[5]);
        const V3 om = v3(e[6], e[7], e[8]);
        const Pose B = se3_exp(v3(e[15], e[16], e[17]), v3(e[18], e[19], e[20]));
        if (in.chart == EQVIO_COORD_NORMAL) {
            const M3 V = so3_V(om);
            const Pose A{so3_exp(om), V * v3(e[9], e[10], e[11])};
            const V3 vA = V * v3(e[12], e[13], e[14]);
            s.pose = pose_mul(xi0.pose, A);
            s.vel = q_rot(q_inv(s.pose.R), q_rot(xi0.pose.R, xi0.vel) + q_rot(xi0.pose.R, vA));
            s.cam = pose_mul(pose_mul(pose_inv(A), xi0.cam), B);
        } else {
            s.pose = pose_mul(xi0.pose, se3_exp(om, v3(e[9], e[10], e[11])));
            s.vel = xi0.vel + v3(e[12], e[13], e[14]);
            s.cam = pose_mul(xi0.cam, B);
        }
        bens_store_sensor(sensor_action(in.X, s), a.eb.sens_of(in.slot), ldp, k);
    } else {
        const int i = blockIdx.y - 1, Lm = BATCH_L;
        const double* lm = a.buf.lm_of(in.slot, in.cur);
        const V3 e{E[k + (size_t)(21 + 3 * i) * ldp], E[k + (size_t)(22 + 3 * i) * ldp], E[k + (size_t)(23 + 3 * i) * ldp]};
        const V3 q = chart_bwd(in.chart, e, ld3(lm, Lm, i));
        const V3 p = (1.0 / lm[BATCH_QA * Lm + i]) * q_rot(q_inv(ldq(lm + BATCH_QQ * Lm, Lm, i)), q);
        double* pts = a.eb.pts_of(in.slot);
        pts[bens_pt(ldp, 0, i, k)] = p.x;
        pts[bens_pt(ldp, 1, i, k)] = p.y;
        pts[bens_pt(ldp, 2, i, k)] = p.z;
    }
}

// ---- computeNEES's eps of every particle of every entry into E. blockIdx.y == 0: the sensor rows, a lane per particle (nees_sensor_error term by term with the
// cancellation-free logarithm, as eqf_ensemble_host.hpp's ens_sensor_error), the padding row n of an odd dimension zeroed; blockIdx.y == 1 + i: the filter's
// landmark i, stateChart(Q_i p_true ; q0_i) with p_true the cloud's landmark match[i]. grid (ceil(Pmax / 256), 1 + Nmax, entries).
__global__ void __launch_bounds__(BATCH_T) k_bens_errors(const BensArgs a) {
    const BensIn& in = a.in[blockIdx.z];
    const int k = blockIdx.x * BATCH_T + threadIdx.x, ldp = a.eb.ldp;
    if (k >= in.P || (int)blockIdx.y > in.N)
        return;
    double* E = a.eb.E_of(in.slot);
    if (blockIdx.y == 0) {
        const SensorState& xi0 = in.xi0;
        const SensorState se = sensor_action(group_inv(in.X), bens_load_sensor(a.eb.sens_of(in.slot), ldp, k));
        V3 dv = se.vel - xi0.vel;
        V3 om, tr, omc, trc;
        const Pose Arel = pose_mul(pose_inv(xi0.pose), se.pose);
        bens_se3_log(Arel, om, tr);
        if (in.chart == EQVIO_COORD_NORMAL) {
            const V3 vA = q_rot(q_inv(xi0.pose.R), q_rot(se.pose.R, se.vel) - q_rot(xi0.pose.R, xi0.vel));
            dv = bens_Vinv(om) * vA;
            bens_se3_log(pose_mul(pose_mul(pose_inv(xi0.cam), Arel), se.cam), omc, trc);
        } else
            bens_se3_log(pose_mul(pose_inv(xi0.cam), se.cam), omc, trc);
        const V3 parts[7] = {se.bgyr - xi0.bgyr, se.bacc - xi0.bacc, om, tr, dv, omc, trc};
#pragma unroll
        for (int b = 0; b < 7; ++b) {
            E[k + (size_t)(3 * b) * ldp] = parts[b].x;
            E[k + (size_t)(3 * b + 1) * ldp] = parts[b].y;
            E[k + (size_t)(3 * b + 2) * ldp] = parts[b].z;
        }
        const int n = 21 + 3 * in.N;
        if (n & 1)
            E[k + (size_t)n * ldp] = 0.0;
    } else {
        const int i = blockIdx.y - 1, t = in.match[i], Lm = BATCH_L;
        const double* lm = a.buf.lm_of(in.slot, in.cur);
        const double* pts = a.eb.pts_of(in.slot);
        const V3 ptrue{pts[bens_pt(ldp, 0, t, k)], pts[bens_pt(ldp, 1, t, k)], pts[bens_pt(ldp, 2, t, k)]};
        const V3 pe = lm[BATCH_QA * Lm + i] * q_rot(ldq(lm + BATCH_QQ * Lm, Lm, i), ptrue);
        const V3 e = chart_fwd(in.chart, pe, ld3(lm, Lm, i));
        E[k + (size_t)(21 + 3 * i) * ldp] = e.x;
        E[k + (size_t)(22 + 3 * i) * ldp] = e.y;
        E[k + (size_t)(23 + 3 * i) * ldp] = e.z;
    }
}

// ---- nees: Y = L^-1 E for 16 particles per wave by a blocked forward substitution, and |y_k|^2 / n in the same launch. For the 16-row tile i0 the products
// with the tiles on its left run on the MFMA (L from HBM / L2, Y from the wave's LDS tile), its 16 x 16 triangle on the VALU: 16 steps, the pivot row's value
// handed to the lanes of the same particles by a lane shuffle. A lane keeps (row i0 + lr, particles lk + 4 q): it sums its rows' squares in ascending order,
// and the 16 lanes of a particle are added in one fixed butterfly - a particle's value depends on its own column and on L alone. Rows from np on are zero.
// Returns without writing where the entry's pivot flag is set. grid (ceil(Pmax / 16), entries), one wave.
__global__ void __launch_bounds__(64) k_bens_solve(const BensArgs a) {
    __shared__ double Ys[BENS_XR * 16];
    const BensIn& in = a.in[blockIdx.y];
    const int P = in.P, p0 = blockIdx.x * 16;
    if (a.eb.flag[blockIdx.y] || p0 >= P)
        return;
    const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4, ldp = a.eb.ldp;
    const int n = 21 + 3 * in.N, np = n + (n & 1);
    const double* L = a.eb.L_of(in.slot);
    const double* E = a.eb.E_of(in.slot);
    double ss[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i0 = 0; i0 < np; i0 += 16) {
        const int row = i0 + lr, rowc = min(row, np - 1);
        d4 acc = {0, 0, 0, 0};
        for (int k0 = 0; k0 < i0; k0 += 4) {
            const int k = k0 + lk; // < i0 <= np - 1
            const double lv = L[rowc + (size_t)k * BENS_LDL];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ys[k * 16 + lr], row < np ? lv : 0.0, acc, 0, 0, 0);
        }
        double t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int pp = p0 + lk + 4 * q, ppc = min(pp, P - 1);
            const double ev = E[ppc + (size_t)rowc * ldp];
            t[q] = ((row < np && pp < P) ? ev : 0.0) - acc[q];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int rj = i0 + j, rjc = min(rj, np - 1);
            const double dv = L[rjc + (size_t)rjc * BENS_LDL], ov = L[rowc + (size_t)rjc * BENS_LDL];
            const double ljj = rj < np ? dv : 1.0;
            const double lrj = (row < np && rj < np && lr > j) ? ov : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double yj = __shfl(t[q], (lane & 48) | j, 64) / ljj;
                t[q] = lr == j ? yj : t[q] - lrj * yj;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            Ys[row * 16 + lk + 4 * q] = t[q];
            ss[q] = __builtin_fma(t[q], t[q], ss[q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double v = ss[q];
        for (int o = 8; o > 0; o >>= 1)
            v += __shfl_xor(v, o, 64);
        const int pp = p0 + lk + 4 * q;
        if (lr == 0 && pp < P)
            a.eb.out[(size_t)blockIdx.y * ldp + pp] = v / (double)n;
    }
}

// ---- integrateSystemFunction, sensor part (VIOState.cpp:28-50, 65), a lane per (entry, particle): the new sensor state in place, and the pose the landmarks
// move by (cameraPoseChangeInv, :53) as rows 0 .. 6 of the slot's E (quaternion w x y z, translation) for k_bens_integrate_points. With sigma6 the sample is
// disturbed by the particle's own six normals of (seed, stream): rows 0 .. 3 the block of counter (0, k, 0, 0), rows 4, 5 of (1, k, 0, 0).
// grid (ceil(Pmax / 256), entries).
__global__ void __launch_bounds__(BATCH_T) k_bens_integrate_sensor(const BensArgs a) {
    const BensIn& in = a.in[blockIdx.y];
    const int k = blockIdx.x * BATCH_T + threadIdx.x, ldp = a.eb.ldp;
    if (k >= in.P)
        return;
    double* sp = a.eb.sens_of(in.slot);
    const SensorState s = bens_load_sensor(sp, ldp, k);
    const double* imu = in.imu;
    const double dt = in.dt;
    V3 gyr = v3(imu[1], imu[2], imu[3]), acc = v3(imu[4], imu[5], imu[6]);
    if (in.noisy) {
        unsigned long long x[4];
        double z[8];
        philox4x64_10(in.seed, in.stream, 0ull, (unsigned long long)k, 0ull, 0ull, x);
        philox_normal_pair(x[0], x[1], z[0], z[1]);
        philox_normal_pair(x[2], x[3], z[2], z[3]);
        philox4x64_10(in.seed, in.stream, 1ull, (unsigned long long)k, 0ull, 0ull, x);
        philox_normal_pair(x[0], x[1], z[4], z[5]);
        gyr = gyr + v3(in.sigma6[0] * z[0], in.sigma6[1] * z[1], in.sigma6[2] * z[2]);
        acc = acc + v3(in.sigma6[3] * z[3], in.sigma6[4] * z[4], in.sigma6[5] * z[5]);
    }
    gyr = gyr - s.bgyr;
    acc = acc - s.bacc;
    SensorState r;
    r.bgyr = s.bgyr + dt * v3(imu[7], imu[8], imu[9]);
    r.bacc = s.bacc + dt * v3(imu[10], imu[11], imu[12]);
    const V3 ivd = q_rot(s.pose.R, acc) + v3(0, 0, -kGravity); // inertialVelocityDiff
    const V3 wv = q_rot(s.pose.R, s.vel);
    Pose pc;
    pc.R = so3_exp(dt * gyr);
    pc.x = q_rot(q_inv(s.pose.R), dt * wv + (0.5 * dt * dt) * ivd);
    r.pose = pose_mul(s.pose, pc);
    r.vel = q_rot(q_inv(r.pose.R), wv + dt * ivd);
    r.cam = s.cam;
    bens_store_sensor(r, sp, ldp, k);
    const Pose T = pose_mul(pose_mul(pose_inv(s.cam), pose_inv(pc)), s.cam);
    double* E = a.eb.E_of(in.slot);
    const double t7[7] = {T.R.w, T.R.x, T.R.y, T.R.z, T.x.x, T.x.y, T.x.z};
#pragma unroll
    for (int c = 0; c < 7; ++c)
        E[k + (size_t)c * ldp] = t7[c];
}
// ... and its landmark part: p <- cameraPoseChangeInv_k * p, a lane per (entry, particle, landmark), in place. grid (ceil(Pmax / 256), Nmax, entries).
__global__ void __launch_bounds__(BATCH_T) k_bens_integrate_points(const BensArgs a) {
    const BensIn& in = a.in[blockIdx.z];
    const int k = blockIdx.x * BATCH_T + threadIdx.x, i = blockIdx.y, ldp = a.eb.ldp;
    if (k >= in.P || i >= in.N)
        return;
    const double* E = a.eb.E_of(in.slot);
    const Pose T{Qt{E[k], E[k + (size_t)ldp], E[k + 2 * (size_t)ldp], E[k + 3 * (size_t)ldp]}, V3{E[k + 4 * (size_t)ldp], E[k + 5 * (size_t)ldp], E[k + 6 * (size_t)ldp]}};
    double* pts = a.eb.pts_of(in.slot);
    const V3 p{pts[bens_pt(ldp, 0, i, k)], pts[bens_pt(ldp, 1, i, k)], pts[bens_pt(ldp, 2, i, k)]};
    const V3 r = pose_act(T, p);
    pts[bens_pt(ldp, 0, i, k)] = r.x;
    pts[bens_pt(ldp, 1, i, k)] = r.y;
    pts[bens_pt(ldp, 2, i, k)] = r.z;
}

} // namespace eqf
