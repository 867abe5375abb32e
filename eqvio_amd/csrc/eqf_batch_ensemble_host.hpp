// Particle ensembles against batch slots, host side (include/eqf_batch_ensemble.h; kernels in eqf_batch_ensemble.hpp). Included by eqf_hip.hip behind the
// single-filter ensemble's files, in the same translation unit: it uses eqf_batch_host.hpp's eqf_batch, BatchPacket, BatchScreen, BatchDevice and
// batch_slot_ok, and HIPCHK / EQFCHK / pick_ld / blocks. Nothing of the batch or of the single-filter ensemble is changed by it, and no call writes anything
// of a slot: the kernels read the slot's current Sigma and landmark planes in place, the host reads xi0, X, the ids, the chart and the current-buffer index.
//
// Every compute call has the batch calls' shape: screen the entries on the host, one packet entry per accepted one, the packet to the device, the call's fixed
// chain of launches on the batch's stream, one copy back (the pivot flags, behind them for nees the values), one synchronisation.
#pragma once
#include "eqf_batch_ensemble.h"

namespace {
struct BensOutState; // the device memory of include/eqf_batch_ensemble_output.h's calls (eqf_batch_ensemble_output_host.hpp), made at their first use
void bens_output_free(BensOutState* s);
} // namespace

struct eqf_bens {
    struct Cloud {
        int P = 0, N = 0;
        std::vector<int> ids;
    };
    eqf_batch* b = nullptr;
    int Pcap = 0;
    BensBufs eb{};
    BatchPacket<BensIn> in;
    BatchPacket<int> flag;      // flag.d is eb.flag
    std::vector<double> h;      // host staging
    std::vector<Cloud> c;
    long launches = 0, factorisations = 0;
    std::vector<void*> own;
    std::vector<char> w_valid;  // per slot: eqf_bens_likelihood's kept weights stand; every call that changes the slot's cloud clears it
    BensOutState* os = nullptr;
    void* fd = nullptr;         // eqf_bens_follow's packets on the device (eqf_batch_ensemble_follow_host.hpp), made at its first use; one of `own`
};

namespace {
template <class T> int bens_alloc(eqf_bens* e, T*& p, size_t count) {
    if (hipMalloc((void**)&p, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) {
        p = nullptr;
        return EQF_E_CAPACITY;
    }
    e->own.push_back(p);
    return 0;
}
// what the kernels read of the slot from the host's half of it
void bens_fill_slot(const eqf_bens* e, int slot, BensIn& in) {
    const eqf_batch::Slot& sl = e->b->s[slot];
    std::memset(&in, 0, sizeof(BensIn));
    in.slot = slot;
    in.cur = sl.cur;
    in.N = (int)sl.ids.size();
    in.P = e->c[slot].P;
    in.chart = sl.set.coordinateChoice;
    in.xi0 = sl.xi0;
    in.X = sl.X;
}
// the filter's landmark i is the cloud's landmark match[i]; EQF_E_BAD_ARG when the cloud does not hold a filter id (the reference asserts there)
int bens_match(const eqf_bens* e, int slot, int* match) {
    const eqf_bens::Cloud& cl = e->c[slot];
    const std::vector<int>& fid = e->b->s[slot].ids;
    std::vector<std::pair<int, int>> mine(cl.N);
    for (int t = 0; t < cl.N; ++t)
        mine[t] = {cl.ids[t], t};
    std::sort(mine.begin(), mine.end());
    for (size_t i = 0; i < fid.size(); ++i) {
        const auto it = std::lower_bound(mine.begin(), mine.end(), std::make_pair(fid[i], -1));
        if (it == mine.end() || it->first != fid[i])
            return EQF_E_BAD_ARG;
        match[i] = it->second;
    }
    return 0;
}
BensArgs bens_args(const eqf_bens* e) { return BensArgs{e->b->buf, e->eb, e->in.d}; }
// the largest P and N over the packet's first nin entries: the launch grids (a workgroup beyond its entry's own sizes returns at once)
void bens_extent(const eqf_bens* e, int nin, int& Pmax, int& Nmax) {
    Pmax = 1, Nmax = 0;
    for (int t = 0; t < nin; ++t) {
        Pmax = std::max(Pmax, e->in.h[t].P);
        Nmax = std::max(Nmax, e->in.h[t].N);
    }
}
// computeNEES's eps of the packet's entries into their slots' E: one launch
void bens_launch_errors(eqf_bens* e, int nin) {
    int Pmax, Nmax;
    bens_extent(e, nin, Pmax, Nmax);
    hipLaunchKernelGGL(k_bens_errors, dim3(blocks(Pmax, BATCH_T), 1 + Nmax, nin), dim3(BATCH_T), 0, e->b->stream, bens_args(e));
    ++e->launches;
}
// the errors / nees screening of one slot: its packet entry, or the code
int bens_errors_entry(const eqf_bens* e, int slot, BensIn& in) {
    if (e->c[slot].P < 1)
        return EQF_E_BAD_ARG;
    bens_fill_slot(e, slot, in);
    return bens_match(e, slot, in.match);
}
} // namespace

int eqf_bens_create(eqf_bens** out, eqf_batch* batch, int max_particles) {
    if (!out || !batch || max_particles < 1)
        return EQF_E_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || batch->device >= ndev)
        return EQF_E_NO_DEVICE;
    BatchDevice dev(batch);
    eqf_bens* e = new eqf_bens();
    e->b = batch;
    e->Pcap = max_particles;
    e->c.resize(batch->slots);
    e->w_valid.assign(batch->slots, 0);
    BensBufs& eb = e->eb;
    eb.ldp = pick_ld(max_particles);
    const size_t B = (size_t)batch->slots, ldp = (size_t)eb.ldp;
    int rc = bens_alloc(e, eb.sens, B * 23 * ldp);
    if (!rc)
        rc = bens_alloc(e, eb.pts, B * 3 * BATCH_L * ldp);
    if (!rc)
        rc = bens_alloc(e, eb.E, B * BENS_NP * ldp);
    if (!rc)
        rc = bens_alloc(e, eb.L, B * BENS_NP * BENS_LDL);
    if (!rc)
        rc = bens_alloc(e, eb.out, B * ldp);
    if (!rc && (e->in.grow(batch->slots) || e->flag.grow(batch->slots)))
        rc = EQF_E_CAPACITY;
    if (rc) {
        eqf_bens_destroy(e);
        return EQF_E_CAPACITY;
    }
    eb.flag = e->flag.d;
    *out = e;
    return 0;
}

void eqf_bens_destroy(eqf_bens* e) {
    if (!e)
        return;
    BatchDevice dev(e->b);
    for (void* p : e->own)
        (void)hipFree(p);
    e->in.release();
    e->flag.release();
    bens_output_free(e->os);
    delete e;
}

int eqf_bens_size(const eqf_bens* e, int slot, int* P, int* N) {
    if (!e || !batch_slot_ok(e->b, slot))
        return EQF_E_BAD_ARG;
    if (P)
        *P = e->c[slot].P;
    if (N)
        *N = e->c[slot].N;
    return 0;
}

int eqf_bens_stats(eqf_bens* e, long* launches, long* factorisations, int reset) {
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

int eqf_bens_set(eqf_bens* e, int slot, int P, int N, const int* ids, const double* sensor, const double* p) {
    if (!e || !batch_slot_ok(e->b, slot) || P < 0 || N < 0 || (P > 0 && !sensor) || (N > 0 && !ids) || (P > 0 && N > 0 && !p))
        return EQF_E_BAD_ARG;
    if (P > e->Pcap || N > BATCH_L)
        return EQF_E_CAPACITY;
    {
        std::vector<int> sorted(ids, ids + N);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return EQF_E_BAD_ARG;
    }
    BatchDevice dev(e->b);
    const size_t ldp = (size_t)e->eb.ldp;
    if (P > 0) {
        e->h.resize((size_t)(23 + 3 * N) * P);
        double* hs = e->h.data();
        double* hp = hs + (size_t)23 * P;
        for (int k = 0; k < P; ++k) {
            for (int c = 0; c < 23; ++c)
                hs[(size_t)c * P + k] = sensor[23 * (size_t)k + c];
            for (int i = 0; i < N; ++i)
                for (int c = 0; c < 3; ++c)
                    hp[((size_t)c * N + i) * P + k] = p[3 * ((size_t)N * k + i) + c];
        }
        HIPCHK(hipMemcpy2D(e->eb.sens_of(slot), sizeof(double) * ldp, hs, sizeof(double) * P, sizeof(double) * P, 23, hipMemcpyHostToDevice));
        for (int c = 0; c < 3 && N > 0; ++c)
            HIPCHK(hipMemcpy2D(e->eb.pts_of(slot) + (size_t)c * BATCH_L * ldp, sizeof(double) * ldp, hp + (size_t)c * N * P, sizeof(double) * P, sizeof(double) * P, N,
                               hipMemcpyHostToDevice));
    }
    e->c[slot].P = P;
    e->c[slot].N = N;
    e->c[slot].ids.assign(ids, ids + N);
    e->w_valid[slot] = 0;
    return 0;
}

int eqf_bens_get(eqf_bens* e, int slot, int* ids, double* sensor, double* p, int capP, int capN) {
    if (!e || !batch_slot_ok(e->b, slot))
        return EQF_E_BAD_ARG;
    const eqf_bens::Cloud& cl = e->c[slot];
    const int P = cl.P, N = cl.N;
    if (P > capP || N > capN)
        return EQF_E_CAPACITY;
    if (ids)
        std::copy(cl.ids.begin(), cl.ids.end(), ids);
    if (P == 0 || (!sensor && !(p && N > 0)))
        return P;
    BatchDevice dev(e->b);
    const size_t ldp = (size_t)e->eb.ldp;
    e->h.resize((size_t)(23 + 3 * N) * P);
    double* hs = e->h.data();
    double* hp = hs + (size_t)23 * P;
    if (sensor) {
        HIPCHK(hipMemcpy2D(hs, sizeof(double) * P, e->eb.sens_of(slot), sizeof(double) * ldp, sizeof(double) * P, 23, hipMemcpyDeviceToHost));
        for (int k = 0; k < P; ++k)
            for (int c = 0; c < 23; ++c)
                sensor[23 * (size_t)k + c] = hs[(size_t)c * P + k];
    }
    if (p && N > 0) {
        for (int c = 0; c < 3; ++c)
            HIPCHK(hipMemcpy2D(hp + (size_t)c * N * P, sizeof(double) * P, e->eb.pts_of(slot) + (size_t)c * BATCH_L * ldp, sizeof(double) * ldp, sizeof(double) * P, N,
                               hipMemcpyDeviceToHost));
        for (int k = 0; k < P; ++k)
            for (int i = 0; i < N; ++i)
                for (int c = 0; c < 3; ++c)
                    p[3 * ((size_t)N * k + i) + c] = hp[((size_t)c * N + i) * P + k];
    }
    return P;
}

int eqf_bens_sample_seeded(eqf_bens* e, int count, const eqf_bens_sample_entry* entries, int* status) {
    if (!e || count < 0 || (count > 0 && (!entries || !status)))
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchScreen scr(e->b, count);
    std::vector<int> ent; // the call's entry of every packet entry
    for (int t = 0; t < count; ++t) {
        const eqf_bens_sample_entry& se = entries[t];
        if (!scr.fresh(e->b, se.slot) || se.P < 1) {
            status[t] = EQF_E_BAD_ARG;
            continue;
        }
        scr.list(se.slot);
        if (se.P > e->Pcap) {
            status[t] = EQF_E_CAPACITY;
            continue;
        }
        BensIn& in = e->in.h[scr.nin];
        bens_fill_slot(e, se.slot, in);
        in.P = se.P;
        in.seed = se.seed;
        in.stream = se.stream;
        status[t] = 0;
        scr.accept(t);
        ent.push_back(t);
    }
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    BatchDevice dev(e->b);
    int Pmax, Nmax;
    bens_extent(e, nin, Pmax, Nmax);
    hipStream_t st = e->b->stream;
    EQFCHK(batch_round_trip(
        e->b, e->in, nin,
        [&] {
            const BensArgs a = bens_args(e);
            hipLaunchKernelGGL(k_bens_factor, dim3(nin), dim3(BATCH_T), 0, st, a);
            hipLaunchKernelGGL(k_bens_sample_eps, dim3(blocks(Pmax, 16), nin), dim3(64), 0, st, a);
            hipLaunchKernelGGL(k_bens_sample_apply, dim3(blocks(Pmax, BATCH_T), 1 + Nmax, nin), dim3(BATCH_T), 0, st, a);
        },
        &e->flag));
    e->launches += 3;
    e->factorisations += nin;
    for (int q = 0; q < nin; ++q) {
        const int slot = e->in.h[q].slot;
        if (e->flag.h[q]) {
            status[ent[q]] = EQF_E_NOT_SPD;
            continue;
        }
        e->c[slot].P = e->in.h[q].P;
        e->c[slot].N = e->in.h[q].N;
        e->c[slot].ids = e->b->s[slot].ids;
        e->w_valid[slot] = 0;
    }
    return 0;
}

int eqf_bens_integrate(eqf_bens* e, int count, const eqf_bens_integrate_entry* entries, int* status) {
    if (!e || count < 0 || (count > 0 && (!entries || !status)))
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchScreen scr(e->b, count);
    for (int t = 0; t < count; ++t) {
        const eqf_bens_integrate_entry& ie = entries[t];
        if (!scr.fresh(e->b, ie.slot)) {
            status[t] = EQF_E_BAD_ARG;
            continue;
        }
        scr.list(ie.slot);
        if (!ie.imu13 || e->c[ie.slot].P < 1) {
            status[t] = EQF_E_BAD_ARG;
            continue;
        }
        BensIn& in = e->in.h[scr.nin];
        bens_fill_slot(e, ie.slot, in);
        in.N = e->c[ie.slot].N; // the cloud's own landmarks move, whatever the slot holds
        std::memcpy(in.imu, ie.imu13, sizeof(in.imu));
        in.dt = ie.dt;
        if (ie.sigma6) {
            in.noisy = 1;
            std::memcpy(in.sigma6, ie.sigma6, sizeof(in.sigma6));
            in.seed = ie.seed;
            in.stream = ie.stream;
        }
        status[t] = 0;
        scr.accept(t);
        e->w_valid[ie.slot] = 0;
    }
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    BatchDevice dev(e->b);
    int Pmax, Nmax;
    bens_extent(e, nin, Pmax, Nmax);
    hipStream_t st = e->b->stream;
    EQFCHK(batch_round_trip(e->b, e->in, nin, [&] {
        const BensArgs a = bens_args(e);
        hipLaunchKernelGGL(k_bens_integrate_sensor, dim3(blocks(Pmax, BATCH_T), nin), dim3(BATCH_T), 0, st, a);
        hipLaunchKernelGGL(k_bens_integrate_points, dim3(blocks(Pmax, BATCH_T), std::max(Nmax, 1), nin), dim3(BATCH_T), 0, st, a);
    }));
    e->launches += 2;
    return 0;
}

int eqf_bens_errors(eqf_bens* e, int slot, double* eps) {
    if (!e || !eps || !batch_slot_ok(e->b, slot))
        return EQF_E_BAD_ARG;
    BensIn in;
    EQFCHK(bens_errors_entry(e, slot, in));
    e->in.h[0] = in;
    BatchDevice dev(e->b);
    EQFCHK(batch_round_trip(e->b, e->in, 1, [&] { bens_launch_errors(e, 1); }));
    const int P = in.P, n = 21 + 3 * in.N;
    e->h.resize((size_t)n * P);
    HIPCHK(hipMemcpy2D(e->h.data(), sizeof(double) * P, e->eb.E_of(slot), sizeof(double) * e->eb.ldp, sizeof(double) * P, n, hipMemcpyDeviceToHost));
    for (int k = 0; k < P; ++k)
        for (int r = 0; r < n; ++r)
            eps[r + (size_t)n * k] = e->h[(size_t)r * P + k];
    return 0;
}

int eqf_bens_nees(eqf_bens* e, int count, const int* slots, double* nees_out, double* mean_out, int* status) {
    if (!e || count < 0 || (count > 0 && (!slots || !status)))
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchScreen scr(e->b, count);
    std::vector<int> ent;
    for (int t = 0; t < count; ++t) {
        if (!scr.fresh(e->b, slots[t])) {
            status[t] = EQF_E_BAD_ARG;
            continue;
        }
        scr.list(slots[t]);
        status[t] = bens_errors_entry(e, slots[t], e->in.h[scr.nin]);
        if (status[t])
            continue;
        scr.accept(t);
        ent.push_back(t);
    }
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    BatchDevice dev(e->b);
    int Pmax, Nmax;
    bens_extent(e, nin, Pmax, Nmax);
    hipStream_t st = e->b->stream;
    const size_t ldp = (size_t)e->eb.ldp;
    e->h.resize((size_t)nin * ldp);
    HIPCHK(hipMemcpyAsync(e->in.d, e->in.h, sizeof(BensIn) * nin, hipMemcpyHostToDevice, st));
    bens_launch_errors(e, nin);
    {
        const BensArgs a = bens_args(e);
        hipLaunchKernelGGL(k_bens_factor, dim3(nin), dim3(BATCH_T), 0, st, a);
        hipLaunchKernelGGL(k_bens_solve, dim3(blocks(Pmax, 16), nin), dim3(64), 0, st, a);
    }
    HIPCHK(hipGetLastError());
    e->launches += 2;
    e->factorisations += nin;
    HIPCHK(hipMemcpyAsync(e->flag.h, e->flag.d, sizeof(int) * nin, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(e->h.data(), e->eb.out, sizeof(double) * nin * ldp, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int q = 0; q < nin; ++q) {
        const int t = ent[q], P = e->in.h[q].P;
        if (e->flag.h[q]) {
            status[t] = EQF_E_NOT_SPD;
            continue;
        }
        const double* v = e->h.data() + (size_t)q * ldp;
        double sum = 0.0;
        for (int k = 0; k < P; ++k)
            sum += v[k];
        if (nees_out)
            std::copy(v, v + P, nees_out + (size_t)t * e->Pcap);
        if (mean_out)
            mean_out[t] = sum / (double)P;
    }
    return 0;
}
