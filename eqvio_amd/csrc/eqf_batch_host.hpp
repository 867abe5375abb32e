// Filter batch, host side (include/eqf_batch.h; kernels in eqf_batch.hpp): B slots of <= 64 landmarks, one launch per entry point.
// Included by eqf_hip.hip behind the context path, in the same translation unit: it uses that file's unpack_sensor, compute_common_at, observer_host_step,
// sensor_lift_delta, nees_sensor_error, make_cam, HIPCHK and pick_ld.
//
// Every entry point that launches has the same shape: screen the entries on the host (BatchScreen), write one packet entry per accepted one into a pinned
// buffer (BatchPacket), one round trip to the device (batch_round_trip), then the host's half of the results.
#pragma once

namespace {
// a pinned host packet and its device copy
template <typename T> struct BatchPacket {
    T* h = nullptr;
    T* d = nullptr;
    int cap = 0;
    // room for n entries: a packet that is too small is freed and allocated anew (nothing in it outlives a call)
    int grow(int n) {
        if (n <= cap)
            return 0;
        release();
        HIPCHK(hipHostMalloc((void**)&h, sizeof(T) * n, hipHostMallocDefault));
        HIPCHK(hipMalloc((void**)&d, sizeof(T) * n));
        cap = n;
        return 0;
    }
    void release() {
        if (h)
            (void)hipHostFree(h);
        (void)hipFree(d);
        h = nullptr, d = nullptr, cap = 0;
    }
};
} // namespace

struct eqf_batch {
    struct Slot {
        SensorState xi0{};
        GroupSensor X{};
        std::vector<int> ids;
        int cur = 0;
        int flags = 0;
        double depth = 0.0;
        long nees_lu = 0; // eqf_batch_nees entries answered by the partial-pivot fallback
        int inn_dof = 0;  // the last step's innovation statistics (eqf_batch_last_innovation)
        double inn_nis = 0.0, inn_logdet = 0.0;
        long tot_updates = 0, tot_dof = 0; // their sums over the steps that carried EQF_BATCH_UPDATED, in step order (eqf_batch_innovation_totals)
        double tot_nis = 0.0, tot_logdet = 0.0;
        int ric_samples = 0, ric_squarings = 0; // the last accurate or discrete step's counters (eqf_batch_last_riccati); 0 after a fast step or a copy into the slot
        eqvio_settings set{}; // the slot's own settings (eqf_batch_set_slot_settings; eqf_batch_create's until then)
        BatchSlotSet ss{};    // what the kernels read of them: copied into the slot's packet entry of every step
    };
    int device = 0, slots = 0, cap = 0;
    hipStream_t stream = nullptr;
    BatchBufs buf{}; // the slots' Sigma, landmark and scratch buffers
    BatchPacket<BatchIn> in; // eqf_batch_step
    BatchPacket<BatchOut> out;
    BatchPacket<ObsStep> steps;
    BatchPacket<RicStep> rsteps; // eqf_batch_step_accurate: the sensor terms of A and B per sample
    BatchPacket<DiscStep> dsteps; // eqf_batch_step_discrete: the sensor terms of B, the sample and the sensor parts of xi0 and X per sample
    BatchPacket<BatchNormalIn> nrm; // the three step calls: the sensor blocks of M and M^-1 of the Normal slots, at the entry's place in the packet
    BatchPacket<NeesIn> nin; // eqf_batch_nees, eqf_batch_consistency
    BatchPacket<NeesOut> nout;
    BatchPacket<eqf_batch_consistency_record> rec;
    BatchPacket<AugIn> ain;  // eqf_batch_augment
    BatchPacket<CopyIn> cin; // eqf_batch_copy_slots
    BatchPacket<RechartIn> rin; // eqf_batch_convert_chart
    BatchPacket<BridgeIn> brin; // eqf_batch_load_ctx
    BatchPacket<EstIn> ein;  // eqf_batch_estimates
    BatchPacket<eqf_batch_estimate_record> erec;
    BatchPacket<PredIn> pin; // eqf_batch_predictions
    BatchPacket<eqf_batch_prediction_record> prec;
    std::vector<Slot> s;
};

namespace {
GroupSensor group_identity() {
    GroupSensor g;
    g.bgyr = v3(0, 0, 0);
    g.bacc = v3(0, 0, 0);
    g.A = pose_identity();
    g.w = v3(0, 0, 0);
    g.B = pose_identity();
    return g;
}
// the slot's current landmark planes on the host: 8 doubles per landmark (q0[3], Q[4], a)
int batch_fetch_landmarks(eqf_batch* b, int slot, std::vector<double>& out) {
    const int N = (int)b->s[slot].ids.size();
    std::vector<double> pl((size_t)BATCH_PLANES * BATCH_L);
    HIPCHK(hipMemcpy(pl.data(), b->buf.lm_of(slot, b->s[slot].cur), sizeof(double) * pl.size(), hipMemcpyDeviceToHost));
    out.assign(8 * (size_t)N, 0.0);
    for (int i = 0; i < N; ++i) {
        for (int c = 0; c < 3; ++c)
            out[8 * i + c] = pl[c * BATCH_L + i];
        for (int c = 0; c < 4; ++c)
            out[8 * i + 3 + c] = pl[(BATCH_QQ + c) * BATCH_L + i];
        out[8 * i + 7] = pl[BATCH_QA * BATCH_L + i];
    }
    return 0;
}
bool batch_slot_ok(const eqf_batch* b, int slot) { return b && slot >= 0 && slot < b->slots; }
// the settings checks eqf_batch_create and eqf_batch_set_slot_settings share: 0, EQF_E_BAD_ARG or EQF_E_UNSUPPORTED
int batch_settings_check(const eqvio_settings* st) {
    if (st->coordinateChoice != EQVIO_COORD_EUCLIDEAN && st->coordinateChoice != EQVIO_COORD_INVDEPTH && st->coordinateChoice != EQVIO_COORD_NORMAL)
        return EQF_E_BAD_ARG;
    if (!st->fastRiccati || st->coordinateChoice == EQVIO_COORD_NORMAL)
        return EQF_E_UNSUPPORTED; // accurate / discrete Riccati and the Normal chart: the per-context path (eqf_hip.h)
    return 0;
}
// the values the kernels read of a slot's settings
BatchSlotSet batch_slot_values(const eqvio_settings* st) {
    BatchSlotSet ss;
    ss.chart = st->coordinateChoice;
    ss.star = st->useEquivariantOutput;
    ss.discrete = st->useDiscreteInnovationLift;
    ss.median = st->useMedianDepth;
    ss.thrAbs = st->outlierThresholdAbs;
    ss.thrProb = st->outlierThresholdProb;
    ss.meas_var = st->measurementNoise * st->measurementNoise;
    ss.init_var = st->initialPointVariance;
    ss.init_depth = st->initialSceneDepth;
    const double qv[4] = {st->velGyrNoise * st->velGyrNoise, st->velAccNoise * st->velAccNoise, st->velGyrBiasWalk * st->velGyrBiasWalk,
                          st->velAccBiasWalk * st->velAccBiasWalk}; // constructInputGainMatrix (VIOFilterSettings.h:192-201)
    for (int i = 0; i < 12; ++i)
        ss.Qd[i] = qv[i / 3];
    const double pv[8] = {st->biasOmegaProcessVariance, st->biasAccelProcessVariance, st->attitudeProcessVariance, st->positionProcessVariance,
                          st->velocityProcessVariance,  st->cameraAttitudeProcessVariance, st->cameraPositionProcessVariance, st->pointProcessVariance};
    std::memcpy(ss.Pd, pv, sizeof(pv));
    return ss;
}
// every entry point that allocates, copies or launches runs on the batch's device, and leaves the caller's current device as it was
struct BatchDevice {
    int prev = -1;
    explicit BatchDevice(const eqf_batch* b) {
        if (hipGetDevice(&prev) != hipSuccess)
            prev = -1;
        if (b && prev != b->device)
            (void)hipSetDevice(b->device);
    }
    ~BatchDevice() {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};
// The screening of a call's entries: the slots the call has listed so far, and for every accepted entry e its place in the packet (in_of[e], else -1). What
// lists a slot differs between the entry points (include/eqf_batch.h) and stays in their loops: eqf_batch_step lists a slot when its entry is accepted, the
// others before their deeper checks, eqf_batch_copy_slots lists the destination only.
struct BatchScreen {
    std::vector<int> listed, in_of;
    int nin = 0; // accepted entries
    BatchScreen(const eqf_batch* b, int count) : listed(b->slots, 0), in_of(count, -1) {}
    // a slot of the batch that no earlier entry of the call has listed
    bool fresh(const eqf_batch* b, int slot) const { return batch_slot_ok(b, slot) && !listed[slot]; }
    void list(int slot) { listed[slot] = 1; }
    void accept(int e) { in_of[e] = nin++; }
};
// One round trip on the batch's stream: the first nin entries of the packet to the device, launch() (the kernel), the first nin entries of the results back
// (out, when the kernel has any for the host), and the stream synchronised.
template <typename In, typename Launch, typename Out = int>
int batch_round_trip(eqf_batch* b, const BatchPacket<In>& in, int nin, Launch launch, const BatchPacket<Out>* out = nullptr) {
    HIPCHK(hipMemcpyAsync(in.d, in.h, sizeof(In) * nin, hipMemcpyHostToDevice, b->stream));
    launch();
    HIPCHK(hipGetLastError());
    if (out)
        HIPCHK(hipMemcpyAsync(out->h, out->d, sizeof(Out) * nin, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}
} // namespace

int eqf_batch_create(eqf_batch** out, int device, int slots, int max_landmarks, const eqvio_settings* st) {
    if (!out || !st || slots < 1 || max_landmarks < 1 || max_landmarks > EQF_BATCH_MAX_LANDMARKS || device < 0)
        return EQF_E_BAD_ARG;
    if (int rc = batch_settings_check(st))
        return rc;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || device >= ndev)
        return EQF_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return EQF_E_NO_DEVICE;
    HIPCHK(hipSetDevice(device));
    eqf_batch* b = new eqf_batch();
    b->device = device;
    b->slots = slots;
    b->cap = max_landmarks;
    BatchBufs& bb = b->buf;
    bb.ld = pick_ld(BATCH_NMAX);
    bb.sig_stride = (size_t)bb.ld * BATCH_NMAX;
    bb.lm_stride = (size_t)BATCH_PLANES * BATCH_L;
    bb.scr_stride = batch_scr_doubles(bb.ld);
    b->s.resize(slots);
    for (auto& sl : b->s) {
        sl.xi0 = unpack_sensor(std::vector<double>{0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0}.data());
        sl.X = group_identity();
        sl.set = *st;
        sl.ss = batch_slot_values(st);
    }
    auto fail = [&](int rc) {
        eqf_batch_destroy(b);
        return rc;
    };
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess)
        return fail(EQF_E_CAPACITY);
    if (hipMalloc((void**)&bb.sig, sizeof(double) * bb.sig_stride * 2 * slots) != hipSuccess ||
        hipMalloc((void**)&bb.lm, sizeof(double) * bb.lm_stride * 2 * slots) != hipSuccess ||
        hipMalloc((void**)&bb.scr, sizeof(double) * bb.scr_stride * slots) != hipSuccess)
        return fail(EQF_E_CAPACITY);
    if (hipMemsetAsync(bb.sig, 0, sizeof(double) * bb.sig_stride * 2 * slots, b->stream) != hipSuccess ||
        hipMemsetAsync(bb.lm, 0, sizeof(double) * bb.lm_stride * 2 * slots, b->stream) != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess)
        return fail(EQF_E_CAPACITY);
    if (b->in.grow(std::min(slots, 64)) || b->out.grow(std::min(slots, 64)) || b->steps.grow(64 * 16))
        return fail(EQF_E_CAPACITY);
    *out = b;
    return EQF_OK;
}
void eqf_batch_destroy(eqf_batch* b) {
    if (!b)
        return;
    BatchDevice dev(b);
    if (b->stream)
        (void)hipStreamSynchronize(b->stream);
    (void)hipFree(b->buf.sig);
    (void)hipFree(b->buf.lm);
    (void)hipFree(b->buf.scr);
    b->in.release();
    b->out.release();
    b->steps.release();
    b->rsteps.release();
    b->dsteps.release();
    b->nrm.release();
    b->nin.release();
    b->nout.release();
    b->rec.release();
    b->ain.release();
    b->cin.release();
    b->rin.release();
    b->brin.release();
    b->ein.release();
    b->erec.release();
    b->pin.release();
    b->prec.release();
    if (b->stream)
        (void)hipStreamDestroy(b->stream);
    delete b;
}
int eqf_batch_slots(const eqf_batch* b) { return b ? b->slots : EQF_E_BAD_ARG; }
int eqf_batch_max_landmarks(const eqf_batch* b) { return b ? b->cap : EQF_E_BAD_ARG; }
int eqf_batch_num_landmarks(const eqf_batch* b, int slot) { return batch_slot_ok(b, slot) ? (int)b->s[slot].ids.size() : EQF_E_BAD_ARG; }
void* eqf_batch_stream(eqf_batch* b) { return b ? (void*)b->stream : nullptr; }
int eqf_batch_synchronize(eqf_batch* b) {
    if (!b)
        return EQF_E_BAD_ARG;
    BatchDevice dev(b);
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}

// No device work: the kernels' share of the values travels in the slot's packet entry of its next step, the host reads the rest where it packs an entry.
int eqf_batch_set_slot_settings(eqf_batch* b, int slot, const eqvio_settings* st) {
    if (!b || !st)
        return EQF_E_BAD_ARG;
    if (int rc = batch_settings_check(st))
        return rc;
    if (!batch_slot_ok(b, slot))
        return EQF_E_BAD_ARG;
    eqf_batch::Slot& sl = b->s[slot];
    if (st->coordinateChoice != sl.set.coordinateChoice && !sl.ids.empty())
        return EQF_E_BAD_ARG; // the slot's Sigma is in the old chart's coordinates
    sl.set = *st;
    sl.ss = batch_slot_values(st);
    return 0;
}
int eqf_batch_check_settings(const eqvio_settings* st) { return st ? batch_settings_check(st) : EQF_E_BAD_ARG; }
// The chart alone, Normal included: eqf_batch_set_slot_settings's rule for a slot that holds landmarks. No device work - the chart travels in the packet entry.
int eqf_batch_set_slot_chart(eqf_batch* b, int slot, int chart) {
    if (!batch_slot_ok(b, slot))
        return EQF_E_BAD_ARG;
    if (chart != EQVIO_COORD_EUCLIDEAN && chart != EQVIO_COORD_INVDEPTH && chart != EQVIO_COORD_NORMAL)
        return EQF_E_BAD_ARG;
    eqf_batch::Slot& sl = b->s[slot];
    if (chart != sl.set.coordinateChoice && !sl.ids.empty())
        return EQF_E_BAD_ARG; // the slot's Sigma is in the old chart's coordinates
    sl.set.coordinateChoice = chart;
    sl.ss.chart = chart;
    return 0;
}
int eqf_batch_get_slot_chart(const eqf_batch* b, int slot) { return batch_slot_ok(b, slot) ? b->s[slot].set.coordinateChoice : EQF_E_BAD_ARG; }
int eqf_batch_get_slot_settings(const eqf_batch* b, int slot, eqvio_settings* out) {
    if (!batch_slot_ok(b, slot) || !out)
        return EQF_E_BAD_ARG;
    *out = b->s[slot].set;
    return 0;
}

int eqf_batch_set_state(eqf_batch* b, int slot, const double* xi0_sensor, const double* X_sensor, const int* ids, const double* q0, const double* Q, int N) {
    if (!batch_slot_ok(b, slot) || !xi0_sensor || !X_sensor || N < 0 || N > b->cap || (N > 0 && (!ids || !q0 || !Q)))
        return EQF_E_BAD_ARG;
    eqf_batch::Slot& sl = b->s[slot];
    BatchDevice dev(b);
    HIPCHK(hipStreamSynchronize(b->stream));
    if (N > 0) {
        double *d_p = nullptr, *d_Q = nullptr;
        HIPCHK(hipMalloc((void**)&d_p, sizeof(double) * 8 * N));
        d_Q = d_p + 3 * N;
        HIPCHK(hipMemcpy(d_p, q0, sizeof(double) * 3 * N, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_Q, Q, sizeof(double) * 5 * N, hipMemcpyHostToDevice));
        double* lm = b->buf.lm_of(slot, sl.cur);
        hipLaunchKernelGGL(k_scatter_landmarks, dim3(1), dim3(64), 0, b->stream, N, 0, BATCH_L, d_p, d_Q, lm, lm + (size_t)BATCH_QQ * BATCH_L,
                           lm + (size_t)BATCH_QA * BATCH_L);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(b->stream));
        HIPCHK(hipFree(d_p));
    }
    sl.xi0 = unpack_sensor(xi0_sensor);
    sl.X = unpack_group(X_sensor);
    sl.ids.assign(ids, ids + N);
    return 0;
}
int eqf_batch_get_state(eqf_batch* b, int slot, double* xi0_sensor, double* X_sensor, int* ids, double* q0, double* Q, int cap) {
    if (!batch_slot_ok(b, slot))
        return EQF_E_BAD_ARG;
    eqf_batch::Slot& sl = b->s[slot];
    const int N = (int)sl.ids.size();
    if (N > cap)
        return EQF_E_CAPACITY;
    BatchDevice dev(b);
    HIPCHK(hipStreamSynchronize(b->stream));
    if (xi0_sensor)
        pack_sensor(sl.xi0, xi0_sensor);
    if (X_sensor)
        pack_group(sl.X, X_sensor);
    std::vector<double> lm;
    if (int rc = batch_fetch_landmarks(b, slot, lm))
        return rc;
    for (int i = 0; i < N; ++i) {
        if (ids)
            ids[i] = sl.ids[i];
        if (q0)
            for (int c = 0; c < 3; ++c)
                q0[3 * i + c] = lm[8 * i + c];
        if (Q)
            for (int c = 0; c < 5; ++c)
                Q[5 * i + c] = lm[8 * i + 3 + c];
    }
    return N;
}
int eqf_batch_set_sigma(eqf_batch* b, int slot, const double* sig, int n) {
    if (!batch_slot_ok(b, slot) || !sig || n != 21 + 3 * (int)b->s[slot].ids.size())
        return EQF_E_BAD_ARG;
    BatchDevice dev(b);
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipMemcpy2D(b->buf.sig_of(slot, b->s[slot].cur), sizeof(double) * b->buf.ld, sig, sizeof(double) * n, sizeof(double) * n, n, hipMemcpyHostToDevice));
    return 0;
}
int eqf_batch_get_sigma(eqf_batch* b, int slot, double* sig, int n) {
    if (!batch_slot_ok(b, slot) || !sig || n != 21 + 3 * (int)b->s[slot].ids.size())
        return EQF_E_BAD_ARG;
    BatchDevice dev(b);
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipMemcpy2D(sig, sizeof(double) * n, b->buf.sig_of(slot, b->s[slot].cur), sizeof(double) * b->buf.ld, sizeof(double) * n, n, hipMemcpyDeviceToHost));
    return 0;
}
int eqf_batch_state_estimate(eqf_batch* b, int slot, double* sensor, int* ids, double* p, int cap) {
    if (!batch_slot_ok(b, slot))
        return EQF_E_BAD_ARG;
    eqf_batch::Slot& sl = b->s[slot];
    const int N = (int)sl.ids.size();
    if (N > cap)
        return EQF_E_CAPACITY;
    BatchDevice dev(b);
    HIPCHK(hipStreamSynchronize(b->stream));
    if (sensor)
        pack_sensor(sensor_action(sl.X, sl.xi0), sensor);
    std::vector<double> lm;
    if (int rc = batch_fetch_landmarks(b, slot, lm))
        return rc;
    for (int i = 0; i < N; ++i) {
        if (ids)
            ids[i] = sl.ids[i];
        if (p) { // stateGroupAction landmark part: q_hat = Q^-1 q0 (VIOGroup.cpp:45-52)
            const double* e = lm.data() + 8 * i;
            const V3 qh = (1.0 / e[7]) * q_rot(q_inv(Qt{e[3], e[4], e[5], e[6]}), v3(e[0], e[1], e[2]));
            pack_v3(qh, p + 3 * i);
        }
    }
    return N;
}
int eqf_batch_sensor_estimate(const eqf_batch* b, int slot, double* sensor) {
    if (!batch_slot_ok(b, slot) || !sensor)
        return EQF_E_BAD_ARG;
    pack_sensor(sensor_action(b->s[slot].X, b->s[slot].xi0), sensor);
    return 0;
}
int eqf_batch_last_result(const eqf_batch* b, int slot, int* flags, double* depth) {
    if (!batch_slot_ok(b, slot))
        return EQF_E_BAD_ARG;
    if (flags)
        *flags = b->s[slot].flags;
    if (depth)
        *depth = b->s[slot].depth;
    return 0;
}

namespace {
// eqf_batch_step, eqf_batch_step_accurate and eqf_batch_step_discrete: one screening, one packet, one round trip, one host half of the results. STEP_ACCURATE:
// the frame's propagation is integrateUpToTime's with fastRiccati == false - the sensor terms of A and B at every sample's X ride along with the observer steps,
// and k_batch_riccati runs in front of k_batch_frame_tail on the same stream; imu13_mean and dt_total are not read. STEP_DISCRETE: the same with
// useDiscreteStateMatrix == true - what rides along per sample is the sensor terms of B, the sample and the sensor parts of xi0 and X (DiscStep), and
// k_batch_discrete runs in k_batch_riccati's place. (A template parameter: the fast instance is the function it was.)
enum { STEP_FAST, STEP_ACCURATE, STEP_DISCRETE };
// The sensor blocks of M and M^-1 of a Normal slot, as normal_congruence (eqf_hip.hip) fills them for a context: xi0's velocity and Ad(T0^-1) of its camera
// offset. dtP: dt P for the closing congruence of the fast step; null for the per-sample modes, which add their noise in Euclidean coordinates.
void batch_normal_pack(const SensorState& xi0, const double* dtP, BatchNormalIn& nb) {
    NormalM nm{};
    nm.v0[0] = xi0.vel.x, nm.v0[1] = xi0.vel.y, nm.v0[2] = xi0.vel.z;
    const M6 Ad = se3_Adjoint(pose_inv(xi0.cam));
    for (int e = 0; e < 36; ++e)
        nm.Ad[e] = Ad.a[e];
    nm.dir = -1;
    nb.inv = nm;
    nm.dir = +1;
    nm.addP = dtP ? 1 : 0;
    for (int k = 0; k < 8; ++k)
        nm.dtP[k] = dtP ? dtP[k] : 0.0;
    nb.fwd = nm;
}
// A step that lists Normal slots: their packet entries move behind the others' (both groups keep their order), scr.in_of follows, and every Normal entry gets its
// BatchNormalIn at its place in b->nrm, sent ahead on the batch's stream. nE: the entries in front. Functions of their own (noinline), so that a step without a
// Normal slot runs the host code it always ran.
__attribute__((noinline)) int batch_normal_partition(eqf_batch* b, BatchScreen& scr, int count, int nin, bool fast, int& nE) {
    std::vector<int> pos(nin);
    int nn = 0;
    for (int i = 0; i < nin; ++i)
        nn += b->in.h[i].ss.chart == EQVIO_COORD_NORMAL;
    nE = nin - nn;
    int ie = 0, in_ = nE;
    bool moved = false;
    for (int i = 0; i < nin; ++i) {
        pos[i] = b->in.h[i].ss.chart == EQVIO_COORD_NORMAL ? in_++ : ie++;
        moved = moved || pos[i] != i;
    }
    if (moved) {
        const std::vector<BatchIn> held(b->in.h, b->in.h + nin);
        for (int i = 0; i < nin; ++i)
            b->in.h[pos[i]] = held[i];
        for (int e = 0; e < count; ++e)
            if (scr.in_of[e] >= 0)
                scr.in_of[e] = pos[scr.in_of[e]];
    }
    if (int rc = b->nrm.grow(std::max(count, 64)))
        return rc;
    for (int i = nE; i < nin; ++i) {
        const BatchIn& in = b->in.h[i];
        const eqf_batch::Slot& sl = b->s[in.slot];
        double dtP[8];
        for (int k = 0; k < 8; ++k)
            dtP[k] = in.dt * sl.ss.Pd[k];
        batch_normal_pack(sl.xi0, fast ? dtP : nullptr, b->nrm.h[i]);
    }
    HIPCHK(hipMemcpyAsync(b->nrm.d + nE, b->nrm.h + nE, sizeof(BatchNormalIn) * nn, hipMemcpyHostToDevice, b->stream));
    return 0;
}
// the propagation of the Normal entries [nE, nE + nN) of a step's packet; the fast step's also their k_batch_frame_tail (the per-sample modes run one tail over all entries)
__attribute__((noinline)) void batch_launch_normal(eqf_batch* b, int mode, int nE, int nN) {
    const BatchNormalIn* nrm = b->nrm.d + nE;
    const BatchArgs ban{b->buf, b->in.d + nE, b->steps.d, b->out.d + nE};
    if (mode == STEP_ACCURATE) {
        const RicArgs ran{b->buf, b->in.d + nE, b->steps.d, b->rsteps.d, b->out.d + nE};
        hipLaunchKernelGGL(k_batch_riccati_normal, dim3(nN), dim3(BATCH_T), 0, b->stream, ran, nrm);
    } else if (mode == STEP_DISCRETE) {
        const DiscArgs dan{b->buf, b->in.d + nE, b->steps.d, b->dsteps.d, b->out.d + nE};
        hipLaunchKernelGGL(k_batch_discrete_normal, dim3(nN), dim3(BATCH_T), 0, b->stream, dan, nrm);
    } else {
        hipLaunchKernelGGL(k_batch_normal, dim3(nN), dim3(BATCH_T), 0, b->stream, ban, nrm);
        hipLaunchKernelGGL(k_batch_frame_tail, dim3(nN), dim3(BATCH_T), 0, b->stream, ban);
    }
}
template <int mode> int batch_step(eqf_batch* b, int count, const eqf_batch_frame* frames, int* status) {
    if (!b || count < 0 || (count > 0 && (!frames || !status)))
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchDevice dev(b);
    int total_steps = 0;
    for (int e = 0; e < count; ++e)
        total_steps += std::max(frames[e].k, 0);
    if (int rc = b->in.grow(count))
        return rc;
    if (int rc = b->out.grow(count))
        return rc;
    if (int rc = b->steps.grow(std::max(total_steps, 64)))
        return rc;
    constexpr bool accurate = mode != STEP_FAST; // a Riccati step per sample, by either of the two per-sample kernels
    if (mode == STEP_ACCURATE)
        if (int rc = b->rsteps.grow(std::max(total_steps, 64)))
            return rc;
    if (mode == STEP_DISCRETE)
        if (int rc = b->dsteps.grow(std::max(total_steps, 64)))
            return rc;
    // host half: validation, the landmark bookkeeping the ids decide, the sensor-level terms and the observer steps' sensor part
    BatchScreen scr(b, count);
    std::vector<GroupSensor> X_after(count);
    std::vector<std::vector<int>> surv_ids(count), new_ids(count);
    std::vector<int> removed_old(count, 0);
    int nsteps = 0, n_normal = 0;
    for (int e = 0; e < count; ++e) {
        const eqf_batch_frame& f = frames[e];
        status[e] = 0;
        if (!scr.fresh(b, f.slot) || f.M < 0 || f.k < 0 || (f.M > 0 && (!f.ids || !f.y)) || (!accurate && !f.imu13_mean) ||
            (f.k > 0 && (!f.imu13_k || !f.dt_k)) || !camera_ok(&f.cam)) {
            status[e] = EQF_E_BAD_ARG;
            continue;
        }
        bool asc = true, dts_ok = true;
        for (int s = 0; accurate && s < f.k; ++s) // a Riccati step per sample: its noise term is Q / dt
            dts_ok = dts_ok && std::isfinite(f.dt_k[s]) && f.dt_k[s] >= 0.0;
        for (int j = 1; j < f.M; ++j)
            asc = asc && f.ids[j] > f.ids[j - 1];
        if (!asc || !dts_ok) {
            status[e] = EQF_E_BAD_ARG;
            continue;
        }
        eqf_batch::Slot& sl = b->s[f.slot];
        const int N0 = (int)sl.ids.size();
        // removeOldLandmarks (VIOFilter.cpp:280-302) and the ids addNewLandmarks will append (:258-278)
        std::vector<int> surv;
        for (int i = 0; i < N0; ++i)
            if (!sl.set.removeLostLandmarks || std::binary_search(f.ids, f.ids + f.M, sl.ids[i]))
                surv.push_back(i);
        std::vector<int> midx(f.M);
        int nnew = 0;
        for (int j = 0; j < f.M; ++j) {
            int found = -1;
            for (size_t t = 0; t < surv.size(); ++t)
                if (sl.ids[surv[t]] == f.ids[j]) {
                    found = (int)t;
                    break;
                }
            if (found < 0)
                for (int i = 0; i < N0 && found < 0; ++i)
                    if (sl.ids[i] == f.ids[j])
                        found = -2; // unmeasured-and-removed cannot happen: a measured id survives
            midx[j] = found >= 0 ? found : -(1 + nnew++);
        }
        if ((int)surv.size() + nnew > b->cap || f.M > b->cap) {
            status[e] = EQF_E_CAPACITY; // the slot is not listed: a later entry of the call may still name it
            continue;
        }
        BatchIn& in = b->in.h[scr.nin];
        in.slot = f.slot;
        in.cur = sl.cur;
        in.Ns = (int)surv.size();
        in.M = f.M;
        in.nnew = nnew;
        in.k = f.k;
        in.obs_off = nsteps;
        in.max_outliers = (int)(size_t)((1.0 - sl.set.featureRetention) * f.M); // removeOutliers (VIOFilter.cpp:305)
        in.ss = sl.ss;
        Cam cam = make_cam(&f.cam);
        in.cam = cam;
        in.dt = accurate ? 0.0 : f.dt_total;
        for (size_t t = 0; t < surv.size(); ++t)
            in.surv[t] = (int)surv[t];
        for (int j = 0; j < f.M; ++j) {
            in.midx[j] = midx[j];
            in.y[2 * j] = f.y[2 * j];
            in.y[2 * j + 1] = f.y[2 * j + 1];
            if (midx[j] < 0) {
                const V3 br = cam_undistort(cam, f.y[2 * j], f.y[2 * j + 1]); // measurement.cameraPtr->undistortPoint (VIOFilter.cpp:264)
                const int r = -midx[j] - 1;
                in.bear[3 * r] = br.x, in.bear[3 * r + 1] = br.y, in.bear[3 * r + 2] = br.z;
                new_ids[e].push_back(f.ids[j]);
            }
        }
        Common cm;
        if (!accurate)
            compute_common_at(sl.X, sl.xi0, f.imu13_mean, cm, in.ck); // integrateRiccatiStateFast at the current X
        else
            std::memset(&in.ck, 0, sizeof(in.ck));
        GroupSensor X = sl.X;
        for (int s = 0; s < f.k; ++s) {
            if (mode == STEP_ACCURATE) { // integrateRiccatiStateAccurate at the X the samples before this one have produced
                RicStep& rs = b->rsteps.h[nsteps + s];
                rs.dt = f.dt_k[s];
                compute_common_at(X, sl.xi0, f.imu13_k + 13 * s, cm, rs.ck);
            } else if (mode == STEP_DISCRETE) { // integrateRiccatiStateDiscrete there: B's sensor terms, and what the device forms A_d from
                DiscStep& ds = b->dsteps.h[nsteps + s];
                ds.dt = f.dt_k[s];
                compute_common_at(X, sl.xi0, f.imu13_k + 13 * s, cm, ds.ck);
                std::memcpy(ds.imu, f.imu13_k + 13 * s, sizeof(ds.imu));
                ds.X = X;
                ds.xi0 = sl.xi0;
            }
            observer_host_step(X, sl.xi0, f.imu13_k + 13 * s, f.dt_k[s], sl.set.useDiscreteVelocityLift, b->steps.h[nsteps + s]);
        }
        nsteps += f.k;
        X_after[e] = X;
        for (int i : surv)
            surv_ids[e].push_back(sl.ids[i]);
        removed_old[e] = (int)surv.size() < N0;
        n_normal += sl.ss.chart == EQVIO_COORD_NORMAL;
        scr.list(f.slot);
        scr.accept(e);
    }
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    // The Normal slots' entries go behind the others' in the packet: entries [0, nE) are launched with the other charts' propagation, [nE, nin) with the Normal
    // chart's, each on its part of the packet. A step without a Normal slot packs and launches what it always did.
    int nE = nin;
    if (n_normal > 0)
        if (int rc = batch_normal_partition(b, scr, count, nin, !accurate, nE))
            return rc;
    const int nN = nin - nE;
    const BatchArgs ba{b->buf, b->in.d, b->steps.d, b->out.d};
    if (nsteps) // the observer steps ride along, in front of the launch on the same stream
        HIPCHK(hipMemcpyAsync(b->steps.d, b->steps.h, sizeof(ObsStep) * nsteps, hipMemcpyHostToDevice, b->stream));
    if (mode == STEP_ACCURATE && nsteps)
        HIPCHK(hipMemcpyAsync(b->rsteps.d, b->rsteps.h, sizeof(RicStep) * nsteps, hipMemcpyHostToDevice, b->stream));
    if (mode == STEP_DISCRETE && nsteps)
        HIPCHK(hipMemcpyAsync(b->dsteps.d, b->dsteps.h, sizeof(DiscStep) * nsteps, hipMemcpyHostToDevice, b->stream));
    const RicArgs ra{b->buf, b->in.d, b->steps.d, b->rsteps.d, b->out.d};
    const DiscArgs da{b->buf, b->in.d, b->steps.d, b->dsteps.d, b->out.d};
    const auto launch = [&] {
        if (mode == STEP_ACCURATE) {
            if (nE)
                hipLaunchKernelGGL(k_batch_riccati, dim3(nE), dim3(BATCH_T), 0, b->stream, ra);
            if (nN)
                batch_launch_normal(b, mode, nE, nN);
            hipLaunchKernelGGL(k_batch_frame_tail, dim3(nin), dim3(BATCH_T), 0, b->stream, ba);
        } else if (mode == STEP_DISCRETE) {
            if (nE)
                hipLaunchKernelGGL(k_batch_discrete, dim3(nE), dim3(BATCH_T), 0, b->stream, da);
            if (nN)
                batch_launch_normal(b, mode, nE, nN);
            hipLaunchKernelGGL(k_batch_frame_tail, dim3(nin), dim3(BATCH_T), 0, b->stream, ba);
        } else {
            if (nE)
                hipLaunchKernelGGL(k_batch_frame, dim3(nE), dim3(BATCH_T), 0, b->stream, ba);
            if (nN)
                batch_launch_normal(b, mode, nE, nN);
        }
    };
    if (int rc = batch_round_trip(b, b->in, nin, launch, &b->out))
        return rc;
    // host half of the results: landmark ids, the sensor lift
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0)
            continue;
        const BatchOut& o = b->out.h[scr.in_of[e]];
        eqf_batch::Slot& sl = b->s[frames[e].slot];
        sl.X = X_after[e];
        std::vector<int> ids;
        for (size_t t = 0; t < surv_ids[e].size(); ++t)
            if (!((o.outliers >> t) & 1ull))
                ids.push_back(surv_ids[e][t]);
        ids.insert(ids.end(), new_ids[e].begin(), new_ids[e].end());
        int flags = (removed_old[e] ? EQF_BATCH_REMOVED_OLD : 0) | ((o.did & BATCH_DID_OUTLIERS) ? EQF_BATCH_REMOVED_OUTLIERS : 0) |
                    ((o.did & BATCH_DID_ADDED) ? EQF_BATCH_ADDED : 0) | ((o.did & BATCH_DID_EMPTY) ? EQF_BATCH_EMPTY : 0);
        if (o.status == 0 && (o.did & BATCH_DID_UPDATE)) {
            sl.X = group_mul(sensor_lift_delta(o.gamma, sl.xi0, sl.set.coordinateChoice, sl.set.useDiscreteInnovationLift), sl.X);
            flags |= EQF_BATCH_UPDATED;
            if (o.did & BATCH_DID_INVALID) {
                std::vector<int> kept;
                for (size_t t = 0; t < ids.size(); ++t)
                    if (!((o.invalid >> t) & 1ull))
                        kept.push_back(ids[t]);
                ids.swap(kept);
                flags |= EQF_BATCH_REMOVED_INVALID;
            }
        } else if (o.status != 0) {
            status[e] = o.status;
        }
        sl.ids.swap(ids);
        sl.cur = o.cur;
        sl.flags = flags;
        sl.depth = o.depth;
        sl.inn_dof = o.dof;
        sl.inn_nis = o.nis;
        sl.inn_logdet = o.logdet;
        sl.ric_samples = accurate ? o.ric_samples : 0;
        sl.ric_squarings = accurate ? o.ric_squarings : 0;
        if (flags & EQF_BATCH_UPDATED) {
            sl.tot_updates += 1;
            sl.tot_dof += o.dof;
            sl.tot_nis += o.nis;
            sl.tot_logdet += o.logdet;
        }
        if ((int)sl.ids.size() != o.N)
            status[e] = EQF_E_BAD_ARG; // bookkeeping disagreement: cannot happen
    }
    return 0;
}
} // namespace

int eqf_batch_step(eqf_batch* b, int count, const eqf_batch_frame* frames, int* status) { return batch_step<STEP_FAST>(b, count, frames, status); }
int eqf_batch_step_accurate(eqf_batch* b, int count, const eqf_batch_frame* frames, int* status) { return batch_step<STEP_ACCURATE>(b, count, frames, status); }
int eqf_batch_step_discrete(eqf_batch* b, int count, const eqf_batch_frame* frames, int* status) { return batch_step<STEP_DISCRETE>(b, count, frames, status); }
int eqf_batch_last_riccati(const eqf_batch* b, int slot, int* samples, int* max_squarings) {
    if (!batch_slot_ok(b, slot))
        return EQF_E_BAD_ARG;
    if (samples)
        *samples = b->s[slot].ric_samples;
    if (max_squarings)
        *max_squarings = b->s[slot].ric_squarings;
    return 0;
}

int eqf_batch_last_innovation(const eqf_batch* b, int slot, int* dof, double* nis, double* logdet) {
    if (!batch_slot_ok(b, slot))
        return EQF_E_BAD_ARG;
    const eqf_batch::Slot& sl = b->s[slot];
    if (dof)
        *dof = sl.inn_dof;
    if (nis)
        *nis = sl.inn_nis;
    if (logdet)
        *logdet = sl.inn_logdet;
    return 0;
}
int eqf_batch_innovation_totals(const eqf_batch* b, int slot, long* updates, long* dof, double* nis, double* logdet) {
    if (!batch_slot_ok(b, slot))
        return EQF_E_BAD_ARG;
    const eqf_batch::Slot& sl = b->s[slot];
    if (updates)
        *updates = sl.tot_updates;
    if (dof)
        *dof = sl.tot_dof;
    if (nis)
        *nis = sl.tot_nis;
    if (logdet)
        *logdet = sl.tot_logdet;
    return 0;
}
int eqf_batch_reset_innovation_totals(eqf_batch* b, int slot) {
    if (!b || slot >= b->slots)
        return EQF_E_BAD_ARG;
    for (int k = slot < 0 ? 0 : slot; k < (slot < 0 ? b->slots : slot + 1); ++k) {
        eqf_batch::Slot& sl = b->s[k];
        sl.tot_updates = sl.tot_dof = 0;
        sl.tot_nis = sl.tot_logdet = 0.0;
    }
    return 0;
}

namespace {
// The host half eqf_batch_nees and eqf_batch_consistency share: the per-entry refusals, and for every accepted entry its packet in b->nin (the sensor
// entries of eps - eqf_compute_nees's code -, the true points in state order). b->nin holds count entries.
BatchScreen batch_nees_pack(eqf_batch* b, int count, const eqf_batch_truth* truths, int* status) {
    BatchScreen scr(b, count);
    std::vector<int> jt;
    std::vector<std::pair<int, int>> order;
    for (int e = 0; e < count; ++e) {
        const eqf_batch_truth& t = truths[e];
        status[e] = 0;
        if (!scr.fresh(b, t.slot) || !t.sensor || t.n_true < 0 || (t.n_true > 0 && (!t.ids || !t.p))) {
            status[e] = EQF_E_BAD_ARG;
            continue;
        }
        scr.list(t.slot);
        const eqf_batch::Slot& sl = b->s[t.slot];
        const int N = (int)sl.ids.size();
        order.resize(N);
        for (int i = 0; i < N; ++i)
            order[i] = {sl.ids[i], i};
        std::sort(order.begin(), order.end());
        jt.assign(N, -1);
        for (int k = 0; k < t.n_true; ++k) { // the first true landmark of an id, as eqf_compute_nees
            const auto it = std::lower_bound(order.begin(), order.end(), std::make_pair(t.ids[k], -1));
            if (it != order.end() && it->first == t.ids[k] && jt[it->second] < 0)
                jt[it->second] = k;
        }
        if (std::find(jt.begin(), jt.end(), -1) != jt.end()) {
            status[e] = EQF_E_BAD_ARG; // the reference asserts the true state holds every filter landmark
            continue;
        }
        NeesIn& in = b->nin.h[scr.nin];
        in.slot = t.slot;
        in.cur = sl.cur;
        in.N = N;
        in.chart = sl.set.coordinateChoice;
        nees_sensor_error(sl.xi0, sl.X, sl.set.coordinateChoice, t.sensor, in.eps);
        for (int i = 0; i < N; ++i)
            for (int c = 0; c < 3; ++c)
                in.p[3 * i + c] = t.p[3 * jt[i] + c];
        scr.accept(e);
    }
    return scr;
}
} // namespace

int eqf_batch_nees(eqf_batch* b, int count, const eqf_batch_truth* truths, double* nees, int* status) {
    if (!b || count < 0 || (count > 0 && (!truths || !nees || !status)))
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchDevice dev(b);
    if (int rc = b->nin.grow(count))
        return rc;
    if (int rc = b->nout.grow(count))
        return rc;
    for (int e = 0; e < count; ++e)
        nees[e] = std::nan("");
    const BatchScreen scr = batch_nees_pack(b, count, truths, status);
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    const NeesArgs na{b->buf, b->nin.d, b->nout.d};
    const auto launch = [&] { hipLaunchKernelGGL(k_batch_nees, dim3(nin), dim3(BATCH_T), 0, b->stream, na); };
    if (int rc = batch_round_trip(b, b->nin, nin, launch, &b->nout))
        return rc;
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0)
            continue;
        const NeesOut& o = b->nout.h[scr.in_of[e]];
        eqf_batch::Slot& sl = b->s[truths[e].slot];
        nees[e] = o.sumsq / (double)(21 + 3 * (int)sl.ids.size());
        sl.nees_lu += o.lu;
    }
    return 0;
}
int eqf_batch_consistency(eqf_batch* b, int count, const eqf_batch_truth* truths, eqf_batch_consistency_record* out, int* status) {
    if (!b || count < 0 || (count > 0 && (!truths || !out || !status)))
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchDevice dev(b);
    if (int rc = b->nin.grow(count))
        return rc;
    if (int rc = b->rec.grow(count))
        return rc;
    const BatchScreen scr = batch_nees_pack(b, count, truths, status);
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    const NeesArgs na{b->buf, b->nin.d, nullptr}; // the kernel writes the records instead
    const auto launch = [&] { hipLaunchKernelGGL(k_batch_consistency, dim3(nin), dim3(BATCH_T), 0, b->stream, na, b->rec.d); };
    if (int rc = batch_round_trip(b, b->nin, nin, launch, &b->rec))
        return rc;
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0)
            continue;
        eqf_batch::Slot& sl = b->s[truths[e].slot];
        eqf_batch_consistency_record& r = out[e];
        r = b->rec.h[scr.in_of[e]];
        const int N = (int)sl.ids.size();
        r.nees = r.nees / (double)(21 + 3 * N); // the kernel left eps^T Sigma^-1 eps there
        for (int i = 0; i < EQF_BATCH_MAX_LANDMARKS; ++i)
            r.ids[i] = i < N ? sl.ids[i] : 0;
        sl.nees_lu += r.lu;
    }
    return 0;
}
// One packet, one launch of k_batch_estimate over the accepted entries, one copy back, one synchronisation. The host's part of a record (N, ids, the sensor
// estimate by eqf_batch_state_estimate's expression) is written into out[e] after the copy; a refused entry's out[e] is never touched.
int eqf_batch_estimates(eqf_batch* b, int count, const int* slots, eqf_batch_estimate_record* out, int* status) {
    if (!b || count < 0 || !slots || !out || !status)
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchScreen scr(b, count);
    for (int e = 0; e < count; ++e) { // the refusals, before any device is looked at
        status[e] = 0;
        if (!scr.fresh(b, slots[e])) {
            status[e] = EQF_E_BAD_ARG;
            continue;
        }
        scr.list(slots[e]);
        scr.accept(e);
    }
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    BatchDevice dev(b);
    if (int rc = b->ein.grow(nin))
        return rc;
    if (int rc = b->erec.grow(nin))
        return rc;
    std::vector<SensorState> est(nin);
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0)
            continue;
        const eqf_batch::Slot& sl = b->s[slots[e]];
        EstIn& in = b->ein.h[scr.in_of[e]];
        in.slot = slots[e];
        in.cur = sl.cur;
        in.N = (int)sl.ids.size();
        in.pad = 0;
        est[scr.in_of[e]] = sensor_action(sl.X, sl.xi0);
        in.pc = pose_mul(est[scr.in_of[e]].pose, est[scr.in_of[e]].cam);
    }
    const EstArgs ea{b->buf, b->ein.d, b->erec.d};
    const auto launch = [&] { hipLaunchKernelGGL(k_batch_estimate, dim3(nin), dim3(BATCH_T), 0, b->stream, ea); };
    if (int rc = batch_round_trip(b, b->ein, nin, launch, &b->erec))
        return rc;
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0)
            continue;
        const eqf_batch::Slot& sl = b->s[slots[e]];
        eqf_batch_estimate_record& r = out[e];
        r = b->erec.h[scr.in_of[e]]; // p, p_world, sigma_sensor
        const int N = (int)sl.ids.size();
        r.N = N;
        r.reserved = 0;
        pack_sensor(est[scr.in_of[e]], r.sensor);
        for (int i = 0; i < EQF_BATCH_MAX_LANDMARKS; ++i)
            r.ids[i] = i < N ? sl.ids[i] : 0;
    }
    return 0;
}
namespace {
// integrateSystemFunction (VIOState.cpp:28-68), sensor part, with the arithmetic of the single filter's host mirror (eqvio_amd/host/VIOFilter.cpp): s becomes
// the integrated state; returns the step's cameraPoseChangeInv, which takes every camera-frame landmark along
Pose predict_sensor_step(SensorState& s, const double* imu13, double dt) {
    const V3 gyr = v3(imu13[1], imu13[2], imu13[3]) - s.bgyr; // v_est = velocity - bias (IMUVelocity.cpp:52-58)
    const V3 acc = v3(imu13[4], imu13[5], imu13[6]) - s.bacc;
    const V3 gravity{0, 0, -kGravity};
    SensorState ns;
    ns.bgyr = s.bgyr + dt * v3(imu13[7], imu13[8], imu13[9]);
    ns.bacc = s.bacc + dt * v3(imu13[10], imu13[11], imu13[12]);
    Pose poseChange;
    poseChange.R = so3_exp(dt * gyr);
    const V3 inertialStep = dt * q_rot(s.pose.R, s.vel) + (0.5 * dt * dt) * (q_rot(s.pose.R, acc) + gravity);
    poseChange.x = q_rot(q_inv(s.pose.R), inertialStep);
    ns.pose = pose_mul(s.pose, poseChange);
    const V3 inertialVelocityDiff = q_rot(s.pose.R, acc) + gravity;
    ns.vel = q_rot(q_inv(ns.pose.R), q_rot(s.pose.R, s.vel) + dt * inertialVelocityDiff);
    ns.cam = s.cam;
    const Pose cameraPoseChangeInv = pose_mul(pose_mul(pose_inv(s.cam), pose_inv(poseChange)), s.cam);
    s = ns;
    return cameraPoseChangeInv;
}
} // namespace

// One packet, one launch of k_batch_predict over the accepted entries, one copy back, one synchronisation. The host does the sensor-level chain of
// predictState (k steps on 23 doubles) and folds the steps' cameraPoseChangeInv into one pose, so a packet entry has a fixed size whatever k is; its part of a
// record (N, ids, the predicted sensor state) is written into out[e] after the copy; a refused entry's out[e] is never touched.
int eqf_batch_predictions(eqf_batch* b, int count, const eqf_batch_prediction_entry* entries, eqf_batch_prediction_record* out, int* status) {
    if (!b || count < 0 || (count > 0 && (!entries || !out || !status)))
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchScreen scr(b, count);
    for (int e = 0; e < count; ++e) { // the refusals, before any device is looked at
        const eqf_batch_prediction_entry& p = entries[e];
        status[e] = 0;
        bool ok = scr.fresh(b, p.slot) && camera_ok(&p.cam) && p.k >= 0 && (p.k == 0 || (p.imu13_k && p.dt_k));
        for (int j = 0; ok && j < p.k; ++j)
            ok = std::isfinite(p.dt_k[j]) && p.dt_k[j] >= 0.0;
        if (!ok) {
            status[e] = EQF_E_BAD_ARG;
            continue;
        }
        scr.list(p.slot);
        scr.accept(e);
    }
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    BatchDevice dev(b);
    if (int rc = b->pin.grow(nin))
        return rc;
    if (int rc = b->prec.grow(nin))
        return rc;
    std::vector<SensorState> pred(nin);
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0)
            continue;
        const eqf_batch_prediction_entry& p = entries[e];
        const eqf_batch::Slot& sl = b->s[p.slot];
        PredIn& in = b->pin.h[scr.in_of[e]];
        in.slot = p.slot;
        in.cur = sl.cur;
        in.N = (int)sl.ids.size();
        in.chart = sl.set.coordinateChoice;
        in.cam = make_cam(&p.cam);
        SensorState& s = pred[scr.in_of[e]];
        s = sensor_action(sl.X, sl.xi0);
        in.T = pose_identity();
        for (int j = 0; j < p.k; ++j)
            in.T = pose_mul(predict_sensor_step(s, p.imu13_k + 13 * j, p.dt_k[j]), in.T);
    }
    const PredArgs pa{b->buf, b->pin.d, b->prec.d};
    const auto launch = [&] { hipLaunchKernelGGL(k_batch_predict, dim3(nin), dim3(BATCH_PRED_T), 0, b->stream, pa); };
    if (int rc = batch_round_trip(b, b->pin, nin, launch, &b->prec))
        return rc;
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0)
            continue;
        const eqf_batch::Slot& sl = b->s[entries[e].slot];
        eqf_batch_prediction_record& r = out[e];
        r = b->prec.h[scr.in_of[e]]; // p, y, out_cov
        const int N = (int)sl.ids.size();
        r.N = N;
        r.reserved = 0;
        pack_sensor(pred[scr.in_of[e]], r.sensor);
        for (int i = 0; i < EQF_BATCH_MAX_LANDMARKS; ++i)
            r.ids[i] = i < N ? sl.ids[i] : 0;
    }
    return 0;
}
int eqf_batch_nees_lu_fallbacks(const eqf_batch* b, int slot, long* count) {
    if (!batch_slot_ok(b, slot) || !count)
        return EQF_E_BAD_ARG;
    *count = b->s[slot].nees_lu;
    return 0;
}

int eqf_batch_augment(eqf_batch* b, int count, const eqf_batch_augment_entry* entries, int* status) {
    if (!b || count < 0 || (count > 0 && (!entries || !status)))
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchDevice dev(b);
    if (int rc = b->ain.grow(count))
        return rc;
    BatchScreen scr(b, count);
    std::vector<std::vector<int>> ids_after(count);
    for (int e = 0; e < count; ++e) {
        const eqf_batch_augment_entry& a = entries[e];
        status[e] = 0;
        if (!scr.fresh(b, a.slot) || a.n_new < 0 || a.n_prov < 0 || (a.n_new > 0 && !a.new_ids) || (a.n_prov > 0 && (!a.prov_ids || !a.prov_p))) {
            status[e] = EQF_E_BAD_ARG;
            continue;
        }
        scr.list(a.slot);
        const eqf_batch::Slot& sl = b->s[a.slot];
        const int N0 = (int)sl.ids.size();
        // removeOldLandmarks(newIds) (VIOFilter.cpp:280-302): the landmarks whose id is in newIds stay, in state order
        std::vector<int> keep, ids;
        for (int i = 0; i < N0; ++i)
            if (std::find(a.new_ids, a.new_ids + a.n_new, sl.ids[i]) != a.new_ids + a.n_new) {
                keep.push_back(i);
                ids.push_back(sl.ids[i]);
            }
        const int nk = (int)keep.size();
        // the ids of newIds not in the state, in newIds order, with the provided state's first landmark of that id (VIOFilter.cpp:118-127)
        std::vector<int> from;
        bool missing = false;
        for (int j = 0; j < a.n_new && !missing; ++j) {
            const int id = a.new_ids[j];
            if (std::find(ids.begin(), ids.begin() + nk, id) != ids.begin() + nk)
                continue;
            const int* it = std::find(a.prov_ids, a.prov_ids + a.n_prov, id);
            if (it == a.prov_ids + a.n_prov)
                missing = true;
            from.push_back((int)(it - a.prov_ids));
            ids.push_back(id);
        }
        if (missing) {
            status[e] = EQF_E_BAD_ARG;
            continue;
        }
        if ((int)ids.size() > b->cap) {
            status[e] = EQF_E_CAPACITY;
            continue;
        }
        if (nk == N0 && from.empty())
            continue; // nothing leaves, nothing comes: the slot stays as it is
        AugIn& in = b->ain.h[scr.nin];
        in.slot = a.slot;
        in.cur = sl.cur;
        in.Nk = nk;
        in.nnew = (int)from.size();
        in.init_var = sl.set.initialPointVariance;
        for (int i = 0; i < nk; ++i)
            in.keep[i] = keep[i];
        for (size_t r = 0; r < from.size(); ++r)
            for (int c = 0; c < 3; ++c)
                in.p[3 * r + c] = a.prov_p[3 * (size_t)from[r] + c];
        ids_after[e].swap(ids);
        scr.accept(e);
    }
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    const AugArgs aa{b->buf, b->ain.d};
    const auto launch = [&] { hipLaunchKernelGGL(k_batch_augment, dim3(nin), dim3(BATCH_T), 0, b->stream, aa); };
    if (int rc = batch_round_trip(b, b->ain, nin, launch))
        return rc;
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0)
            continue;
        eqf_batch::Slot& sl = b->s[entries[e].slot];
        sl.ids.swap(ids_after[e]);
        sl.cur ^= 1;
    }
    return 0;
}

// One launch for every accepted entry, one synchronisation. Everything that refuses an entry is decided on the host before the launch.
int eqf_batch_copy_slots(eqf_batch* b, int count, const int* src, const int* dst, int* status) {
    if (!b || count < 0 || !src || !dst || !status)
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchScreen scr(b, count); // lists destinations
    for (int e = 0; e < count; ++e) {
        status[e] = 0;
        if (!batch_slot_ok(b, src[e]) || !scr.fresh(b, dst[e])) {
            status[e] = EQF_E_BAD_ARG;
            continue;
        }
        const eqf_batch::Slot &from = b->s[src[e]], &to = b->s[dst[e]];
        if (!from.ids.empty() && to.set.coordinateChoice != from.set.coordinateChoice) {
            status[e] = EQF_E_BAD_ARG; // the source's Sigma is in its own chart's coordinates (eqf_batch_set_slot_settings's rule)
            continue;
        }
        scr.list(dst[e]);
        if (src[e] != dst[e])
            scr.accept(e);
    }
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    if (b->buf.ld % 2 || b->buf.sig_stride % 2 || b->buf.lm_stride % 2)
        return EQF_E_BAD_ARG; // k_batch_copy moves pairs of doubles: a column, a plane and a buffer must start on 16 bytes (pick_ld gives an even ld today)
    BatchDevice dev(b);
    if (int rc = b->cin.grow(nin))
        return rc;
    // the sources' host halves as they are BEFORE the call: a slot may be a destination of one entry and the source of another
    struct HostHalf {
        SensorState xi0;
        GroupSensor X;
        std::vector<int> ids;
    };
    std::vector<HostHalf> held(nin);
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0)
            continue;
        const eqf_batch::Slot &from = b->s[src[e]], &to = b->s[dst[e]];
        CopyIn& in = b->cin.h[scr.in_of[e]];
        in.src = src[e];
        in.scur = from.cur;
        in.dst = dst[e];
        in.dnxt = to.cur ^ 1;
        in.N = (int)from.ids.size();
        held[scr.in_of[e]] = HostHalf{from.xi0, from.X, from.ids};
    }
    const CopyArgs ca{b->buf, b->cin.d};
    const auto launch = [&] { hipLaunchKernelGGL(k_batch_copy, dim3(nin, BATCH_COPY_CHUNKS), dim3(BATCH_T), 0, b->stream, ca); };
    if (int rc = batch_round_trip(b, b->cin, nin, launch))
        return rc;
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0)
            continue;
        eqf_batch::Slot& to = b->s[dst[e]];
        HostHalf& h = held[scr.in_of[e]];
        to.xi0 = h.xi0;
        to.X = h.X;
        to.ids.swap(h.ids);
        to.cur ^= 1;
        to.flags = 0; // the last step's outcome was another state's: as a slot that never stepped
        to.depth = 0.0;
        to.inn_dof = 0;
        to.inn_nis = to.inn_logdet = 0.0;
        to.ric_samples = to.ric_squarings = 0;
    }
    return 0;
}

// One launch of k_batch_rechart over the entries that change something on the device, one synchronisation; nothing of Sigma crosses to the host. The host
// supplies what M_normal's sensor block needs of xi0 (batch_normal_pack's values). An entry whose slot holds no landmark while neither chart is Normal changes
// no number - T is the identity on the 21 sensor coordinates - and is eqf_batch_set_slot_chart's relabelling.
int eqf_batch_convert_chart(eqf_batch* b, int count, const int* slots, const int* charts, int* status) {
    if (!b || count < 0 || !slots || !charts || !status)
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchScreen scr(b, count);
    std::vector<char> relabel(count, 0);
    for (int e = 0; e < count; ++e) { // the refusals, before any device is looked at
        status[e] = 0;
        if (!scr.fresh(b, slots[e])) {
            status[e] = EQF_E_BAD_ARG;
            continue;
        }
        scr.list(slots[e]);
        const int to = charts[e];
        if (to != EQVIO_COORD_EUCLIDEAN && to != EQVIO_COORD_INVDEPTH && to != EQVIO_COORD_NORMAL) {
            status[e] = EQF_E_BAD_ARG;
            continue;
        }
        const eqf_batch::Slot& sl = b->s[slots[e]];
        const int from = sl.set.coordinateChoice;
        if (to == from)
            continue; // the slot's own chart: nothing to do
        if (sl.ids.empty() && to != EQVIO_COORD_NORMAL && from != EQVIO_COORD_NORMAL)
            relabel[e] = 1;
        else
            scr.accept(e);
    }
    const int nin = scr.nin;
    if (nin > 0) {
        BatchDevice dev(b);
        if (int rc = b->rin.grow(nin))
            return rc;
        for (int e = 0; e < count; ++e) {
            if (scr.in_of[e] < 0)
                continue;
            const eqf_batch::Slot& sl = b->s[slots[e]];
            RechartIn& in = b->rin.h[scr.in_of[e]];
            in.slot = slots[e];
            in.cur = sl.cur;
            in.N = (int)sl.ids.size();
            in.from = sl.set.coordinateChoice;
            in.to = charts[e];
            in.sdir = in.to == EQVIO_COORD_NORMAL ? +1 : (in.from == EQVIO_COORD_NORMAL ? -1 : 0);
            BatchNormalIn nb;
            batch_normal_pack(sl.xi0, nullptr, nb);
            std::memcpy(in.v0, nb.fwd.v0, sizeof(in.v0));
            std::memcpy(in.Ad, nb.fwd.Ad, sizeof(in.Ad));
        }
        const RechartArgs ra{b->buf, b->rin.d};
        const auto launch = [&] { hipLaunchKernelGGL(k_batch_rechart, dim3(nin), dim3(BATCH_T), 0, b->stream, ra); };
        if (int rc = batch_round_trip(b, b->rin, nin, launch))
            return rc;
    }
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0 && !relabel[e])
            continue;
        eqf_batch::Slot& sl = b->s[slots[e]];
        sl.set.coordinateChoice = charts[e];
        sl.ss.chart = charts[e];
        if (scr.in_of[e] >= 0)
            sl.cur ^= 1;
    }
    return 0;
}

namespace {
// what both directions of the bridge refuse of a context, before any device work: another device, the Normal chart (its sensor block of Sigma is in other
// coordinates), the float Sigma store
int bridge_ctx_check(const eqf_batch* b, const eqf_ctx* c) {
    if (c->device != b->device)
        return EQF_E_BAD_ARG;
    if (c->chart == EQVIO_COORD_NORMAL || c->sig32)
        return EQF_E_UNSUPPORTED;
    return 0;
}
// the context's current buffers as k_batch_bridge takes them: read after enter(), which may flip them
BridgeCtx bridge_ctx_buffers(eqf_ctx* c) { return BridgeCtx{c->sigma(), c->q0(), c->Qq(), c->Qa(), c->ld, c->Ncap}; }
// k_batch_bridge moves pairs of doubles (k_batch_copy's rule, for both sides)
bool bridge_aligned(const eqf_batch* b, const eqf_ctx* c) {
    return b->buf.ld % 2 == 0 && b->buf.sig_stride % 2 == 0 && c->ld % 2 == 0 && reinterpret_cast<uintptr_t>(c->d_sigma[c->cur]) % 16 == 0;
}
} // namespace

// The context is entered the way eqf_get_state enters it - an update taken from the early doorbell settled, held landmarks appended, a pending reshape flushed,
// the observer's stream joined -, the packet and the one launch go onto the CONTEXT's stream behind all of that, and the one wait is the context's. The batch is
// idle between its calls (every one of them ends in a synchronisation), so nothing of the batch's stream has to be ordered.
int eqf_batch_load_ctx(eqf_batch* b, eqf_ctx* src, int count, const int* slots, int* status) {
    if (!b || !src || !slots || !status || count < 0)
        return EQF_E_BAD_ARG;
    if (int rc = bridge_ctx_check(b, src))
        return rc;
    if (src->N > b->cap)
        return EQF_E_CAPACITY;
    if (count == 0)
        return 0;
    BatchScreen scr(b, count);
    for (int e = 0; e < count; ++e) {
        status[e] = 0;
        if (!scr.fresh(b, slots[e]) || (src->N > 0 && b->s[slots[e]].set.coordinateChoice != src->chart)) {
            status[e] = EQF_E_BAD_ARG; // the context's Sigma is in its own chart's coordinates (eqf_batch_set_slot_settings's rule)
            continue;
        }
        scr.list(slots[e]);
        scr.accept(e);
    }
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    BatchDevice dev(b);
    if (int rc = b->brin.grow(nin))
        return rc;
    if (int rc = enter(src))
        return rc;
    if (int rc = join_observer(src))
        return rc;
    if (!bridge_aligned(b, src))
        return EQF_E_BAD_ARG; // (pick_ld gives even leading dimensions and hipMalloc 16-byte aligned buffers today)
    for (int e = 0; e < count; ++e)
        if (scr.in_of[e] >= 0)
            b->brin.h[scr.in_of[e]] = BridgeIn{slots[e], b->s[slots[e]].cur ^ 1};
    const BridgeArgs ga{b->buf, bridge_ctx_buffers(src), b->brin.d, BridgeIn{0, 0}, src->N};
    HIPCHK(hipMemcpyAsync(b->brin.d, b->brin.h, sizeof(BridgeIn) * nin, hipMemcpyHostToDevice, src->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_batch_bridge<false>), dim3(nin, BATCH_COPY_CHUNKS), dim3(BATCH_T), 0, src->stream, ga);
    HIPCHK(hipGetLastError());
    if (int rc = sync_ctx(src))
        return rc;
    for (int e = 0; e < count; ++e) {
        if (scr.in_of[e] < 0)
            continue;
        eqf_batch::Slot& to = b->s[slots[e]];
        to.xi0 = src->xi0;
        to.X = src->X;
        to.ids = src->ids;
        to.cur ^= 1;
        to.flags = 0; // eqf_batch_copy_slots's rule: the last step's outcome was another state's
        to.depth = 0.0;
        to.inn_dof = 0;
        to.inn_nis = to.inn_logdet = 0.0;
        to.ric_samples = to.ric_squarings = 0;
    }
    return 0;
}

// eqf_set_state + eqf_set_sigma with the slot's values, the landmarks and Sigma arriving by one launch on the context's stream instead of two copies from the
// host: the same entry (enter, capacity), the same bookkeeping (estimate cache, device measurement, held landmarks, the landmark generation - which drops a
// staged measurement, the id lookup and the mapped ids), the same rounding of Sigma for EQF_OPT_SIGMA_FP32 = 1, and one wait at the end.
int eqf_batch_store_ctx(eqf_batch* b, int slot, eqf_ctx* dst) {
    if (!b || !dst || !batch_slot_ok(b, slot))
        return EQF_E_BAD_ARG;
    if (int rc = bridge_ctx_check(b, dst))
        return rc;
    const eqf_batch::Slot& sl = b->s[slot];
    const int N = (int)sl.ids.size();
    if (N > 0 && sl.set.coordinateChoice != dst->chart)
        return EQF_E_BAD_ARG;
    BatchDevice dev(b);
    if (int rc = enter(dst))
        return rc;
    if (N > dst->Ncap)
        if (int rc = grow_capacity(dst, std::max(N, 2 * dst->Ncap)))
            return rc;
    if (int rc = join_observer(dst))
        return rc;
    if (!bridge_aligned(b, dst))
        return EQF_E_BAD_ARG;
    const BridgeArgs ga{b->buf, bridge_ctx_buffers(dst), nullptr, BridgeIn{slot, sl.cur}, N};
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_batch_bridge<true>), dim3(1, BATCH_COPY_CHUNKS), dim3(BATCH_T), 0, dst->stream, ga);
    HIPCHK(hipGetLastError());
    dst->est_valid = false, ++dst->est_epoch; // eqf_set_state's lines
    dst->meas_valid = false;
    dst->n_held = 0, dst->held_in_memory = false;
    dst->xi0 = sl.xi0;
    dst->X = sl.X;
    dst->ids = sl.ids;
    dst->N = N;
    dst->dev_N = N;
    ++dst->lm_gen;
    if (int rc = round_sigma(dst)) // eqf_set_sigma's (a launch of its own, only with EQF_OPT_SIGMA_FP32 = 1)
        return rc;
    return sync_ctx(dst);
}
