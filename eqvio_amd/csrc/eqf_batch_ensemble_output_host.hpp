// The measurement side of the particle ensembles against batch slots, host side (include/eqf_batch_ensemble_output.h; kernels in
// eqf_batch_ensemble_output.hpp). Included by eqf_hip.hip behind eqf_batch_ensemble_host.hpp, whose struct eqf_bens, bens_errors_entry, bens_launch_errors and
// bens_extent it uses; camera_ok, make_cam, BatchScreen, BatchPacket, BatchDevice and HIPCHK / EQFCHK / blocks are the translation unit's.
//
// The calls have the batch calls' shape: screen the entries on the host, one packet entry per accepted one, the packet to the device, the call's fixed chain of
// launches on the batch's stream, at most one copy back, one synchronisation. Their device memory (BensOutState) is made at their first use and freed by
// eqf_bens_destroy. The existing calls know of it only through eqf_bens::w_valid, the per-slot flag of the kept weights.
#pragma once
#include "eqf_batch_ensemble_output.h"

namespace {
struct BensOutState {
    BensOutBufs ob{};
    double* res = nullptr; // [scal 4 B | ll B ldp | w B ldp]: what one copy brings back
    BatchPacket<BensOutIn> in;
    double* d_cov = nullptr;
    int cov_cap = 0;
    std::vector<double> h;
    std::vector<int> hsrc;
};
void bens_output_free(BensOutState* s) {
    if (!s)
        return;
    (void)hipFree(s->res);
    (void)hipFree(s->ob.cum);
    (void)hipFree(s->ob.G);
    (void)hipFree(s->ob.src);
    (void)hipFree(s->d_cov);
    s->in.release();
    delete s;
}
// the state of these calls, made at the first of them; EQF_E_CAPACITY when an allocation fails (nothing is kept then)
int bens_output_state(eqf_bens* e, BensOutState*& out) {
    if (e->os) {
        out = e->os;
        return 0;
    }
    BatchDevice dev(e->b);
    BensOutState* s = new BensOutState();
    const size_t B = (size_t)e->b->slots, ldp = (size_t)e->eb.ldp;
    bool ok = hipMalloc((void**)&s->res, sizeof(double) * (4 * B + 2 * B * ldp)) == hipSuccess;
    ok = ok && hipMalloc((void**)&s->ob.cum, sizeof(double) * B * ldp) == hipSuccess;
    ok = ok && hipMalloc((void**)&s->ob.G, sizeof(double) * B * BENS_GP * ldp) == hipSuccess;
    ok = ok && hipMalloc((void**)&s->ob.src, sizeof(int) * B * ldp) == hipSuccess;
    ok = ok && s->in.grow((int)B) == 0;
    if (!ok) {
        (void)hipGetLastError();
        bens_output_free(s);
        return EQF_E_CAPACITY;
    }
    s->ob.scal = s->res;
    s->ob.ll = s->res + 4 * B;
    s->ob.w = s->ob.ll + B * ldp;
    e->os = s;
    out = s;
    return 0;
}
// the cloud's place of every measured id; EQF_E_BAD_ARG for an id it does not hold or a repeated one (M <= the cloud's N is the caller's check)
int bens_match_ids(const eqf_bens::Cloud& cl, const int* ids, int M, int* match) {
    std::vector<std::pair<int, int>> mine(cl.N);
    for (int t = 0; t < cl.N; ++t)
        mine[t] = {cl.ids[t], t};
    std::sort(mine.begin(), mine.end());
    std::vector<char> seen(cl.N, 0);
    for (int j = 0; j < M; ++j) {
        const auto it = std::lower_bound(mine.begin(), mine.end(), std::make_pair(ids[j], -1));
        if (it == mine.end() || it->first != ids[j] || seen[it->second])
            return EQF_E_BAD_ARG;
        seen[it->second] = 1;
        match[j] = it->second;
    }
    return 0;
}
BensOutArgs bens_out_args(const eqf_bens* e, const BensOutState* s) { return BensOutArgs{e->eb, s->ob, s->in.d}; }
} // namespace

int eqf_bens_likelihood(eqf_bens* e, int count, const eqf_bens_likelihood_entry* entries, double* loglik_out, double* weights_out, double* logsumexp_out,
                        double* ess_out, int* status) {
    if (!e || count < 0 || (count > 0 && (!entries || !status)))
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchScreen scr(e->b, count);
    std::vector<int> ent; // the call's entry of every packet entry
    std::vector<BensOutIn> pk; // the packet, screened before any device work
    int Pmax = 1;
    for (int t = 0; t < count; ++t) {
        const eqf_bens_likelihood_entry& le = entries[t];
        status[t] = EQF_E_BAD_ARG;
        if (!scr.fresh(e->b, le.slot))
            continue;
        scr.list(le.slot);
        const eqf_bens::Cloud& cl = e->c[le.slot];
        if (le.M < 0 || (le.M > 0 && (!le.cam || !le.ids || !le.y)) || (le.cam && !camera_ok(le.cam)) || cl.P < 1 || le.M > cl.N || !(le.meas_var > 0.0) ||
            !std::isfinite(le.meas_var))
            continue;
        BensOutIn in;
        std::memset(&in, 0, sizeof(BensOutIn));
        if (bens_match_ids(cl, le.ids, le.M, in.match))
            continue;
        in.slot = le.slot;
        in.P = cl.P;
        in.N = cl.N;
        in.M = le.M;
        in.meas_var = le.meas_var;
        if (le.cam)
            in.cam = make_cam(le.cam);
        if (le.M > 0)
            std::memcpy(in.y, le.y, sizeof(double) * 2 * le.M);
        Pmax = std::max(Pmax, cl.P);
        pk.push_back(in);
        status[t] = 0;
        scr.accept(t);
        ent.push_back(t);
    }
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    BensOutState* s = nullptr;
    EQFCHK(bens_output_state(e, s));
    std::memcpy(s->in.h, pk.data(), sizeof(BensOutIn) * nin);
    BatchDevice dev(e->b);
    hipStream_t st = e->b->stream;
    const size_t B = (size_t)e->b->slots, ldp = (size_t)e->eb.ldp;
    for (int q = 0; q < nin; ++q)
        e->w_valid[s->in.h[q].slot] = 0; // from here on the kept weights are being replaced
    HIPCHK(hipMemcpyAsync(s->in.d, s->in.h, sizeof(BensOutIn) * nin, hipMemcpyHostToDevice, st));
    {
        const BensOutArgs a = bens_out_args(e, s);
        hipLaunchKernelGGL(k_bens_loglik, dim3(blocks(Pmax, 32), nin), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_bens_weights, dim3(nin), dim3(256), 0, st, a);
    }
    HIPCHK(hipGetLastError());
    e->launches += 2;
    // one copy back: the scalars, and the rows as far as the caller asks for them
    const size_t back = weights_out ? 4 * B + B * ldp + (size_t)nin * ldp : (loglik_out ? 4 * B + (size_t)nin * ldp : 4 * (size_t)nin);
    s->h.resize(back);
    HIPCHK(hipMemcpyAsync(s->h.data(), s->res, sizeof(double) * back, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int q = 0; q < nin; ++q) {
        const int t = ent[q], P = s->in.h[q].P;
        const double* sc = s->h.data() + 4 * (size_t)q;
        if (sc[3] == 0.0) {
            status[t] = EQF_E_NONFINITE; // nothing kept
            continue;
        }
        if (loglik_out)
            std::copy_n(s->h.data() + 4 * B + (size_t)q * ldp, P, loglik_out + (size_t)t * e->Pcap);
        if (weights_out)
            std::copy_n(s->h.data() + 4 * B + B * ldp + (size_t)q * ldp, P, weights_out + (size_t)t * e->Pcap);
        if (logsumexp_out)
            logsumexp_out[t] = sc[0] + std::log(sc[1]);
        if (ess_out)
            ess_out[t] = 1.0 / sc[2];
        e->w_valid[s->in.h[q].slot] = 1;
    }
    return 0;
}

int eqf_bens_resample_weighted_seeded(eqf_bens* e, int count, const eqf_bens_resample_entry* entries, int* src_out, int* status) {
    if (!e || count < 0 || (count > 0 && (!entries || !status)))
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    BatchScreen scr(e->b, count);
    std::vector<int> ent;
    std::vector<BensOutIn> pk;
    int Pmax = 1, Nmax = 0;
    for (int t = 0; t < count; ++t) {
        const eqf_bens_resample_entry& re = entries[t];
        if (!scr.fresh(e->b, re.slot) || re.P_new < 1) {
            status[t] = EQF_E_BAD_ARG;
            continue;
        }
        scr.list(re.slot);
        if (re.P_new > e->Pcap) {
            status[t] = EQF_E_CAPACITY;
            continue;
        }
        if (!e->w_valid[re.slot]) {
            status[t] = EQF_E_BAD_ARG;
            continue;
        }
        const eqf_bens::Cloud& cl = e->c[re.slot];
        BensOutIn in;
        std::memset(&in, 0, sizeof(BensOutIn));
        in.slot = re.slot;
        in.P = cl.P;
        in.N = cl.N;
        in.P_new = re.P_new;
        in.seed = re.seed;
        in.stream = re.stream;
        Pmax = std::max(Pmax, re.P_new);
        Nmax = std::max(Nmax, cl.N);
        pk.push_back(in);
        status[t] = 0;
        scr.accept(t);
        ent.push_back(t);
    }
    const int nin = scr.nin;
    if (nin == 0)
        return 0;
    BensOutState* s = nullptr;
    EQFCHK(bens_output_state(e, s));
    std::memcpy(s->in.h, pk.data(), sizeof(BensOutIn) * nin);
    BatchDevice dev(e->b);
    hipStream_t st = e->b->stream;
    const size_t ldp = (size_t)e->eb.ldp;
    for (int q = 0; q < nin; ++q)
        e->w_valid[s->in.h[q].slot] = 0;
    HIPCHK(hipMemcpyAsync(s->in.d, s->in.h, sizeof(BensOutIn) * nin, hipMemcpyHostToDevice, st));
    {
        const BensOutArgs a = bens_out_args(e, s);
        const dim3 grid(blocks(Pmax, 256), 23 + 3 * Nmax, nin);
        hipLaunchKernelGGL(k_bens_pick, dim3(blocks(Pmax, 256), nin), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_bens_gather, grid, dim3(256), 0, st, a, 0);
        hipLaunchKernelGGL(k_bens_gather, grid, dim3(256), 0, st, a, 1);
    }
    HIPCHK(hipGetLastError());
    e->launches += 3;
    if (src_out) {
        s->hsrc.resize((size_t)nin * ldp);
        HIPCHK(hipMemcpyAsync(s->hsrc.data(), s->ob.src, sizeof(int) * nin * ldp, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int q = 0; q < nin; ++q) {
        const BensOutIn& in = s->in.h[q];
        e->c[in.slot].P = in.P_new;
        if (src_out)
            std::copy_n(s->hsrc.data() + (size_t)q * ldp, in.P_new, src_out + (size_t)ent[q] * e->Pcap);
    }
    return 0;
}

int eqf_bens_covariance(eqf_bens* e, int count, const int* slots, double* cov_out, int* status) {
    if (!e || count < 0 || (count > 0 && (!slots || !cov_out || !status)))
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
    BensOutState* s = nullptr;
    EQFCHK(bens_output_state(e, s));
    BatchDevice dev(e->b);
    constexpr size_t NN = (size_t)BATCH_NMAX * BATCH_NMAX;
    if (nin > s->cov_cap) { // the staging of the results, grown to the call's accepted entries
        double* p = nullptr;
        if (hipMalloc((void**)&p, sizeof(double) * NN * nin) != hipSuccess) {
            (void)hipGetLastError();
            return EQF_E_CAPACITY;
        }
        (void)hipFree(s->d_cov);
        s->d_cov = p;
        s->cov_cap = nin;
    }
    int Pmax, Nmax;
    bens_extent(e, nin, Pmax, Nmax);
    hipStream_t st = e->b->stream;
    HIPCHK(hipMemcpyAsync(e->in.d, e->in.h, sizeof(BensIn) * nin, hipMemcpyHostToDevice, st));
    bens_launch_errors(e, nin);
    const int nt = (21 + 3 * Nmax + 15) / 16;
    hipLaunchKernelGGL(k_bens_cov, dim3(nt * (nt + 1) / 2, nin), dim3(64), 0, st, bens_args(e), s->d_cov);
    HIPCHK(hipGetLastError());
    ++e->launches;
    s->h.resize(NN * nin);
    HIPCHK(hipMemcpyAsync(s->h.data(), s->d_cov, sizeof(double) * NN * nin, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int q = 0; q < nin; ++q) {
        const size_t n = 21 + 3 * (size_t)e->in.h[q].N;
        std::copy_n(s->h.data() + NN * q, n * n, cov_out + NN * ent[q]);
    }
    return 0;
}
