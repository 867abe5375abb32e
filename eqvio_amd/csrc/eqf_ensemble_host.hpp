// Particle ensemble, host side (include/eqf_ensemble.h; kernels in eqf_ensemble.hpp). Included by eqf_hip.hip behind the filter batch, in the same translation
// unit: it uses that file's enter, join_observer, launch_chain, read_flags, sync_ctx, unpack_sensor / pack_sensor, sensor_action / group_inv, HIPCHK and pick_ld, and
// reads a context's Sigma and landmark planes in place. Nothing of the context path is changed by it.
//
// Every entry point is synchronous: it returns with the device idle for this ensemble, so the copies in front of a call's kernels are plain blocking copies
// (their number never depends on P) and the kernels of a call that takes a context run on that context's stream, behind whatever the context has queued.
#pragma once
#include "eqf_ensemble.h"

struct eqf_ensemble {
    int device = 0;
    hipStream_t stream = nullptr; // calls without a context (integrate, resample)
    int Pcap = 0, Ncap = 0, ldp = 0; // capacity; leading dimension of the particle-major arrays
    int npcap = 0, ldz = 0;          // columns and leading dimension of the factorisation's work matrices
    int P = 0, N = 0;
    std::vector<int> ids;
    std::vector<double> sensor;      // 23 x P, host resident like a context's sensor state
    double* d_pts[2] = {nullptr, nullptr}; // the points (eqf_ensemble.hpp's plane layout), double-buffered for the resampling gather
    int cur = 0;
    double *d_E = nullptr, *d_Z = nullptr, *d_W = nullptr, *d_xi = nullptr, *d_out = nullptr, *d_cov = nullptr, *d_pose = nullptr;
    int* d_idx = nullptr;
    // the measurement side (eqf_ensemble_output_host.hpp): results and kept weights, running sums, measurement / uniforms; the kept weights are valid
    double *d_lw = nullptr, *d_cum = nullptr, *d_yu = nullptr;
    bool w_valid = false;
    long launches = 0, factorisations = 0;
    std::vector<double> h; // host staging
    std::vector<void*> own;
    int Nalloc() const { return std::max(Ncap, 1); }
};

namespace {
template <class T> int ens_alloc(eqf_ensemble* e, T*& p, size_t count) {
    HIPCHK(hipMalloc(&p, sizeof(T) * std::max<size_t>(count, 1)));
    e->own.push_back(p);
    return 0;
}
// the context's counters (launch calls and their host time among them) are what they were when the call returns
struct EnsCountersKept {
    eqf_ctx* c;
    CtxCounters kept;
    explicit EnsCountersKept(eqf_ctx* ctx) : c(ctx), kept(*ctx) {}
    ~EnsCountersKept() { static_cast<CtxCounters&>(*c) = kept; }
};
// what every call that takes a context checks before anything else
int ens_check_ctx(const eqf_ensemble* e, const eqf_ctx* c) {
    if (!e || !c || e->device != c->device)
        return EQF_E_BAD_ARG;
    if (c->sig32)
        return EQF_E_UNSUPPORTED;
    return 0;
}
// the filter's landmark i is the ensemble's landmark match[i] (host data on both sides, current before the context is entered: eqf_remove_landmarks and
// eqf_add_landmarks update ids and N at once)
int ens_match(const eqf_ensemble* e, const eqf_ctx* c, std::vector<int>& match) {
    std::vector<std::pair<int, int>> mine(e->N);
    for (int t = 0; t < e->N; ++t)
        mine[t] = {e->ids[t], t};
    std::sort(mine.begin(), mine.end());
    match.resize(c->N);
    for (int i = 0; i < c->N; ++i) {
        const auto it = std::lower_bound(mine.begin(), mine.end(), std::make_pair(c->ids[i], -1));
        if (it == mine.end() || it->first != c->ids[i])
            return EQF_E_BAD_ARG; // the reference asserts that the true state holds every filter landmark
        match[i] = it->second;
    }
    return 0;
}
// sensorChart_std.inv / sensorChart_normal.inv (VIOState.cpp:114-121, 138-151)
SensorState ens_sensor_chart_inv(int chart, const double* e, const SensorState& xi0) {
    SensorState s;
    s.bgyr = xi0.bgyr + v3(e[0], e[1], e[2]);
    s.bacc = xi0.bacc + v3(e[3], e[4], e[5]);
    const V3 om = v3(e[6], e[7], e[8]);
    const Pose B = se3_exp(v3(e[15], e[16], e[17]), v3(e[18], e[19], e[20]));
    if (chart == EQVIO_COORD_NORMAL) {
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
    return s;
}
// so3_Vinv without its cancellation. eqf_math.hpp's coefficient (1 - (th / 2) sin th / (1 - cos th)) / th^2 subtracts twice: 1 - cos th keeps th^2 of its digits and the
// outer difference th^2 / 12 of those. Against 40-digit arithmetic the coefficient is off by 3.5e-8 relative at th = 0.01 and 1.9e-4 at th = 0.001 (the half-angle form
// below: 1e-11 and 1.9e-9), which reaches a translation coordinate of eps as th^2 / 12 of that - 3e-13 and 1.6e-11 - and showed as 1.2e-12 on NEES(sampled particle) =
// |xi|^2 / n at N = 0. (th / 2) cot(th / 2) has one subtraction of terms that are exact to rounding. Host code of this path only: so3_Vinv is a device function of
// every kernel and stays as it is.
M3 ens_Vinv(V3 om) {
    const double th = norm(om);
    if (th < 1e-4)
        return so3_Vinv(om);
    const double half = 0.5 * th;
    const double Cc = (1.0 - half * cos(half) / sin(half)) / (th * th);
    const M3 Om = skew(om);
    return m3_identity() - 0.5 * Om + Cc * (Om * Om);
}
void ens_se3_log(const Pose& P, V3& om, V3& v) {
    om = so3_log(P.R);
    v = ens_Vinv(om) * P.x;
}
// nees_sensor_error (eqf_hip.hip) term by term, with the logarithm above
void ens_sensor_error(const SensorState& xi0, const GroupSensor& X, int chart, const double* ts, double* eps) {
    const SensorState se = sensor_action(group_inv(X), unpack_sensor(ts));
    V3 dv = se.vel - xi0.vel;
    V3 om, tr, omc, trc;
    const Pose Arel = pose_mul(pose_inv(xi0.pose), se.pose);
    ens_se3_log(Arel, om, tr);
    if (chart == EQVIO_COORD_NORMAL) {
        const V3 vA = q_rot(q_inv(xi0.pose.R), q_rot(se.pose.R, se.vel) - q_rot(xi0.pose.R, xi0.vel));
        dv = ens_Vinv(om) * vA;
        ens_se3_log(pose_mul(pose_mul(pose_inv(xi0.cam), Arel), se.cam), omc, trc);
    } else
        ens_se3_log(pose_mul(pose_inv(xi0.cam), se.cam), omc, trc);
    const V3 parts[7] = {se.bgyr - xi0.bgyr, se.bacc - xi0.bacc, om, tr, dv, omc, trc};
    for (int b = 0; b < 7; ++b)
        pack_v3(parts[b], eps + 3 * b);
}
// E^T (particle-major, eqf_ensemble.hpp) for the ensemble against the entered context: the 21 sensor coordinates of every particle on the host (one 2-D copy),
// the landmark coordinates by one launch
int ens_form_errors(eqf_ensemble* e, eqf_ctx* c, const std::vector<int>& match) {
    const int P = e->P, N = c->N;
    e->h.resize((size_t)21 * P);
    double eps[21];
    for (int k = 0; k < P; ++k) {
        ens_sensor_error(c->xi0, c->X, c->chart, e->sensor.data() + 23 * (size_t)k, eps);
        for (int r = 0; r < 21; ++r)
            e->h[(size_t)r * P + k] = eps[r];
    }
    HIPCHK(hipMemcpy2D(e->d_E, sizeof(double) * e->ldp, e->h.data(), sizeof(double) * P, sizeof(double) * P, 21, hipMemcpyHostToDevice));
    if (N > 0) {
        HIPCHK(hipMemcpy(e->d_idx, match.data(), sizeof(int) * N, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_ens_errors, dim3(blocks(P, 256), N), dim3(256), 0, c->stream, P, c->Ncap, c->chart, c->q0(), c->Qq(), c->Qa(), e->d_idx, e->d_pts[e->cur], e->Nalloc(),
                           e->ldp, e->d_E);
        HIPCHK(hipGetLastError());
        ++e->launches;
    }
    return 0;
}
// Z = [Sigma padded ; extra rows] through the launch chain; EQF_E_NOT_SPD if a pivot was <= 0. The stream is idle on return.
int ens_factorise(eqf_ensemble* e, eqf_ctx* c, int extra, int dup) {
    const int n = c->n(), np = n + (n & 1); // even dimension for the chain's 2x2-pivot elimination, as eqf_compute_nees
    HIPCHK(hipMemsetAsync(c->d_flags, 0, sizeof(int) * 4, c->stream));
    hipLaunchKernelGGL(k_ens_build_Z, dim3(blocks(np + extra, 256), np), dim3(256), 0, c->stream, n, np, c->ld, e->ldz, (const double*)c->sigma(), e->d_E, e->ldp, extra, dup, e->d_Z);
    HIPCHK(hipGetLastError());
    EQFCHK(launch_chain(c, np + extra, np, e->ldz, e->d_Z, e->d_W));
    e->launches += 2 + blocks(np, 32);
    ++e->factorisations;
    EQFCHK(read_flags(c));
    return c->h_flags[0] ? EQF_E_NOT_SPD : 0;
}
// checks, matching, entry and E^T: the common front of errors, nees and covariance
int ens_errors_front(eqf_ensemble* e, eqf_ctx* c) {
    EQFCHK(ens_check_ctx(e, c));
    if (e->P < 1)
        return EQF_E_BAD_ARG;
    std::vector<int> match;
    EQFCHK(ens_match(e, c, match));
    EQFCHK(enter(c));
    EQFCHK(join_observer(c));
    return ens_form_errors(e, c, match);
}
} // namespace

int eqf_ensemble_create(eqf_ensemble** out, int device, int max_particles, int max_landmarks) {
    if (!out || max_particles < 1 || max_landmarks < 0 || device < 0)
        return EQF_E_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || device >= ndev)
        return EQF_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return EQF_E_NO_DEVICE;
    HIPCHK(hipSetDevice(device));
    eqf_ensemble* e = new eqf_ensemble();
    e->device = device;
    e->Pcap = max_particles;
    e->Ncap = max_landmarks;
    e->ldp = pick_ld(max_particles);
    const int ncap = 21 + 3 * max_landmarks;
    e->npcap = ncap + (ncap & 1);
    e->ldz = pick_ld(e->npcap + std::max(e->Pcap, e->npcap)); // nees: np + P rows; sample: 2 np rows
    int rc = (int)hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    const size_t planes = 3 * (size_t)e->Nalloc() * e->ldp;
    auto all = [&]() {
        EQFCHK(ens_alloc(e, e->d_pts[0], planes));
        EQFCHK(ens_alloc(e, e->d_pts[1], planes));
        EQFCHK(ens_alloc(e, e->d_E, (size_t)e->ldp * e->npcap));
        EQFCHK(ens_alloc(e, e->d_Z, (size_t)e->ldz * e->npcap));
        EQFCHK(ens_alloc(e, e->d_W, (size_t)e->ldz * e->npcap));
        EQFCHK(ens_alloc(e, e->d_xi, (size_t)ncap * e->Pcap));
        EQFCHK(ens_alloc(e, e->d_out, (size_t)e->Pcap));
        EQFCHK(ens_alloc(e, e->d_cov, (size_t)ncap * ncap));
        EQFCHK(ens_alloc(e, e->d_pose, 7 * (size_t)e->ldp));
        EQFCHK(ens_alloc(e, e->d_idx, (size_t)std::max(e->Pcap, e->Nalloc())));
        EQFCHK(ens_alloc(e, e->d_lw, 4 + 2 * (size_t)e->Pcap));
        EQFCHK(ens_alloc(e, e->d_cum, (size_t)e->Pcap));
        EQFCHK(ens_alloc(e, e->d_yu, (size_t)std::max(e->Pcap, 2 * e->Nalloc())));
        return 0;
    };
    if (!rc)
        rc = all();
    if (rc) {
        eqf_ensemble_destroy(e);
        return rc == (int)hipErrorOutOfMemory ? EQF_E_CAPACITY : rc;
    }
    *out = e;
    return 0;
}

void eqf_ensemble_destroy(eqf_ensemble* e) {
    if (!e)
        return;
    (void)hipSetDevice(e->device);
    for (void* p : e->own)
        (void)hipFree(p);
    if (e->stream)
        (void)hipStreamDestroy(e->stream);
    delete e;
}

int eqf_ensemble_size(const eqf_ensemble* e, int* P, int* N) {
    if (!e)
        return EQF_E_BAD_ARG;
    if (P)
        *P = e->P;
    if (N)
        *N = e->N;
    return 0;
}

int eqf_ensemble_stats(eqf_ensemble* e, long* launches, long* factorisations, int reset) {
    if (!e)
        return EQF_E_BAD_ARG;
    if (launches)
        *launches = e->launches;
    if (factorisations)
        *factorisations = e->factorisations;
    if (reset)
        e->launches = e->factorisations = 0;
    return 0;
}

int eqf_ensemble_set(eqf_ensemble* e, int P, int N, const int* ids, const double* sensor, const double* p) {
    if (!e || P < 0 || N < 0 || (P > 0 && !sensor) || (N > 0 && !ids) || (P > 0 && N > 0 && !p))
        return EQF_E_BAD_ARG;
    if (P > e->Pcap || N > e->Ncap)
        return EQF_E_CAPACITY;
    {
        std::vector<int> sorted(ids, ids + N);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return EQF_E_BAD_ARG;
    }
    HIPCHK(hipSetDevice(e->device));
    if (P > 0 && N > 0) {
        e->h.resize(3 * (size_t)N * P);
        for (int k = 0; k < P; ++k)
            for (int i = 0; i < N; ++i)
                for (int c = 0; c < 3; ++c)
                    e->h[((size_t)c * N + i) * P + k] = p[3 * ((size_t)N * k + i) + c];
        for (int c = 0; c < 3; ++c)
            HIPCHK(hipMemcpy2D(e->d_pts[e->cur] + (size_t)c * e->Nalloc() * e->ldp, sizeof(double) * e->ldp, e->h.data() + (size_t)c * N * P, sizeof(double) * P, sizeof(double) * P, N,
                               hipMemcpyHostToDevice));
    }
    e->P = P;
    e->N = N;
    e->w_valid = false;
    e->ids.assign(ids, ids + N);
    e->sensor.assign(sensor, sensor + 23 * (size_t)P);
    return 0;
}

int eqf_ensemble_get(eqf_ensemble* e, int* ids, double* sensor, double* p, int capP, int capN) {
    if (!e)
        return EQF_E_BAD_ARG;
    const int P = e->P, N = e->N;
    if (P > capP || N > capN)
        return EQF_E_CAPACITY;
    if (ids)
        std::copy(e->ids.begin(), e->ids.end(), ids);
    if (sensor)
        std::copy(e->sensor.begin(), e->sensor.end(), sensor);
    if (p && P > 0 && N > 0) {
        HIPCHK(hipSetDevice(e->device));
        e->h.resize(3 * (size_t)N * P);
        for (int c = 0; c < 3; ++c)
            HIPCHK(hipMemcpy2D(e->h.data() + (size_t)c * N * P, sizeof(double) * P, e->d_pts[e->cur] + (size_t)c * e->Nalloc() * e->ldp, sizeof(double) * e->ldp, sizeof(double) * P, N,
                               hipMemcpyDeviceToHost));
        for (int k = 0; k < P; ++k)
            for (int i = 0; i < N; ++i)
                for (int c = 0; c < 3; ++c)
                    p[3 * ((size_t)N * k + i) + c] = e->h[((size_t)c * N + i) * P + k];
    }
    return P;
}

namespace {
// eqf_ensemble_sample behind its copy of xi: d_xi holds the n x P standard normals (uploaded, or generated there by eqf_ensemble_sample_seeded); the context is
// entered and its counters are kept by the caller
int ens_sample_from_xi(eqf_ensemble* e, eqf_ctx* c, int P) {
    const int N = c->N, n = c->n(), np = n + (n & 1);
    // L: the chain on [Sigma ; Sigma] leaves Sigma L^-T = L in rows [np, 2 np) of W
    EQFCHK(ens_factorise(e, c, np, 1));
    hipLaunchKernelGGL(k_ens_trmm, dim3(blocks(n, 16), blocks(P, 64)), dim3(256), 0, c->stream, n, np, P, e->ldz, e->d_W, e->d_xi, e->d_E, e->ldp);
    HIPCHK(hipGetLastError());
    ++e->launches;
    EQFCHK(sync_ctx(c));
    // the sensor part of every particle on the host: sensorStateGroupAction(X, sensorChart^-1(eps[0, 21) ; xi0))
    e->h.resize((size_t)21 * P);
    HIPCHK(hipMemcpy2D(e->h.data(), sizeof(double) * P, e->d_E, sizeof(double) * e->ldp, sizeof(double) * P, 21, hipMemcpyDeviceToHost));
    std::vector<double> sens(23 * (size_t)P);
    double eps[21];
    for (int k = 0; k < P; ++k) {
        for (int r = 0; r < 21; ++r)
            eps[r] = e->h[(size_t)r * P + k];
        pack_sensor(sensor_action(c->X, ens_sensor_chart_inv(c->chart, eps, c->xi0)), sens.data() + 23 * (size_t)k);
    }
    if (N > 0) {
        hipLaunchKernelGGL(k_ens_sample_points, dim3(blocks(P, 256), N), dim3(256), 0, c->stream, P, c->Ncap, c->chart, c->q0(), c->Qq(), c->Qa(), e->d_E, e->ldp, e->d_pts[e->cur],
                           e->Nalloc());
        HIPCHK(hipGetLastError());
        ++e->launches;
        EQFCHK(sync_ctx(c));
    }
    e->P = P;
    e->N = N;
    e->w_valid = false;
    e->ids = c->ids;
    e->sensor.swap(sens);
    return 0;
}
} // namespace

int eqf_ensemble_sample(eqf_ensemble* e, eqf_ctx* c, int P, const double* xi) {
    EQFCHK(ens_check_ctx(e, c));
    if (!xi || P < 1)
        return EQF_E_BAD_ARG;
    if (P > e->Pcap || c->N > e->Ncap)
        return EQF_E_CAPACITY;
    EQFCHK(enter(c));
    EQFCHK(join_observer(c));
    const EnsCountersKept keep(c);
    HIPCHK(hipMemcpy(e->d_xi, xi, sizeof(double) * (size_t)c->n() * P, hipMemcpyHostToDevice));
    return ens_sample_from_xi(e, c, P);
}

int eqf_ensemble_integrate(eqf_ensemble* e, const double* imu13, double dt, const double* imu_offset) {
    if (!e || !imu13)
        return EQF_E_BAD_ARG;
    const int P = e->P, N = e->N;
    if (P == 0)
        return 0;
    // integrateSystemFunction, sensor part (VIOState.cpp:28-50, 65), and the pose the landmarks move by (:53)
    std::vector<double> sens(23 * (size_t)P);
    e->h.resize(7 * (size_t)P);
    for (int k = 0; k < P; ++k) {
        const SensorState s = unpack_sensor(e->sensor.data() + 23 * (size_t)k);
        V3 gyr = v3(imu13[1], imu13[2], imu13[3]), acc = v3(imu13[4], imu13[5], imu13[6]);
        if (imu_offset) {
            gyr = gyr + v3(imu_offset[6 * k], imu_offset[6 * k + 1], imu_offset[6 * k + 2]);
            acc = acc + v3(imu_offset[6 * k + 3], imu_offset[6 * k + 4], imu_offset[6 * k + 5]);
        }
        gyr = gyr - s.bgyr;
        acc = acc - s.bacc;
        SensorState r;
        r.bgyr = s.bgyr + dt * v3(imu13[7], imu13[8], imu13[9]);
        r.bacc = s.bacc + dt * v3(imu13[10], imu13[11], imu13[12]);
        const V3 ivd = q_rot(s.pose.R, acc) + v3(0, 0, -kGravity); // inertialVelocityDiff
        const V3 wv = q_rot(s.pose.R, s.vel);
        Pose pc;
        pc.R = so3_exp(dt * gyr);
        pc.x = q_rot(q_inv(s.pose.R), dt * wv + (0.5 * dt * dt) * ivd);
        r.pose = pose_mul(s.pose, pc);
        r.vel = q_rot(q_inv(r.pose.R), wv + dt * ivd);
        r.cam = s.cam;
        pack_sensor(r, sens.data() + 23 * (size_t)k);
        const Pose T = pose_mul(pose_mul(pose_inv(s.cam), pose_inv(pc)), s.cam);
        const double t7[7] = {T.R.w, T.R.x, T.R.y, T.R.z, T.x.x, T.x.y, T.x.z};
        for (int r7 = 0; r7 < 7; ++r7)
            e->h[(size_t)r7 * P + k] = t7[r7];
    }
    if (N > 0) {
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipMemcpy2D(e->d_pose, sizeof(double) * e->ldp, e->h.data(), sizeof(double) * P, sizeof(double) * P, 7, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_ens_integrate, dim3(blocks(P, 256), N), dim3(256), 0, e->stream, P, e->d_pose, e->d_pts[e->cur], e->Nalloc(), e->ldp);
        HIPCHK(hipGetLastError());
        ++e->launches;
        EQFCHK(spin_stream(e->stream));
    }
    e->sensor.swap(sens);
    e->w_valid = false;
    return 0;
}

int eqf_ensemble_errors(eqf_ensemble* e, eqf_ctx* c, double* eps) {
    if (!eps)
        return EQF_E_BAD_ARG;
    EQFCHK(ens_errors_front(e, c));
    const EnsCountersKept keep(c);
    EQFCHK(sync_ctx(c));
    const int P = e->P, n = c->n();
    e->h.resize((size_t)n * P);
    HIPCHK(hipMemcpy2D(e->h.data(), sizeof(double) * P, e->d_E, sizeof(double) * e->ldp, sizeof(double) * P, n, hipMemcpyDeviceToHost));
    for (int k = 0; k < P; ++k)
        for (int r = 0; r < n; ++r)
            eps[r + (size_t)n * k] = e->h[(size_t)r * P + k];
    return 0;
}

int eqf_ensemble_nees(eqf_ensemble* e, eqf_ctx* c, double* nees, double* mean) {
    EQFCHK(ens_errors_front(e, c));
    const EnsCountersKept keep(c);
    const int P = e->P, n = c->n(), np = n + (n & 1);
    // Z = [Sigma ; E^T]: rows [np, np + P) of W receive eps_k^T L^-T, NEES_k = |that row|^2 / n
    {
        const int rc = ens_factorise(e, c, P, 0);
        if (rc)
            return rc;
    }
    hipLaunchKernelGGL(k_ens_rowsumsq, dim3(blocks(P, 32)), dim3(256), 0, c->stream, P, np, e->ldz, e->d_W, e->d_out);
    HIPCHK(hipGetLastError());
    ++e->launches;
    EQFCHK(sync_ctx(c));
    e->h.resize(P);
    HIPCHK(hipMemcpy(e->h.data(), e->d_out, sizeof(double) * P, hipMemcpyDeviceToHost));
    double sum = 0.0;
    for (int k = 0; k < P; ++k) {
        const double v = e->h[k] / (double)n;
        if (nees)
            nees[k] = v;
        sum += v;
    }
    if (mean)
        *mean = sum / (double)P;
    return 0;
}

int eqf_ensemble_covariance(eqf_ensemble* e, eqf_ctx* c, double* cov) {
    if (!cov)
        return EQF_E_BAD_ARG;
    EQFCHK(ens_errors_front(e, c));
    const EnsCountersKept keep(c);
    const int n = c->n(), nt = blocks(n, 16);
    hipLaunchKernelGGL(k_ens_cov, dim3(nt, nt), dim3(64), 0, c->stream, n, e->P, e->d_E, e->ldp, e->d_cov);
    HIPCHK(hipGetLastError());
    ++e->launches;
    EQFCHK(sync_ctx(c));
    HIPCHK(hipMemcpy(cov, e->d_cov, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost));
    return 0;
}

int eqf_ensemble_resample(eqf_ensemble* e, int P_new, const int* src) {
    if (!e || !src || P_new < 1 || e->P < 1)
        return EQF_E_BAD_ARG;
    if (P_new > e->Pcap)
        return EQF_E_CAPACITY;
    for (int k = 0; k < P_new; ++k)
        if (src[k] < 0 || src[k] >= e->P)
            return EQF_E_BAD_ARG;
    const int N = e->N;
    if (N > 0) {
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipMemcpy(e->d_idx, src, sizeof(int) * P_new, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_ens_gather, dim3(blocks(P_new, 256), 3 * N), dim3(256), 0, e->stream, P_new, e->d_idx, e->d_pts[e->cur], e->d_pts[1 - e->cur], e->Nalloc(), N, e->ldp);
        HIPCHK(hipGetLastError());
        ++e->launches;
        EQFCHK(spin_stream(e->stream));
        e->cur = 1 - e->cur;
    }
    std::vector<double> sens(23 * (size_t)P_new);
    for (int k = 0; k < P_new; ++k)
        std::copy(e->sensor.begin() + 23 * (size_t)src[k], e->sensor.begin() + 23 * (size_t)src[k] + 23, sens.begin() + 23 * (size_t)k);
    e->sensor.swap(sens);
    e->P = P_new;
    e->w_valid = false;
    return 0;
}
