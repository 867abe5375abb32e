// eqf_bens_follow, host side (eqvio_amd/csrc/eqf_batch_ensemble_follow.h; kernels in eqf_batch_ensemble_follow.hpp). Included at the end of eqf_hip.hip behind
// eqf_batch_ensemble_follow.hpp, in the same translation unit: it uses eqf_batch_ensemble_host.hpp's struct eqf_bens, bens_alloc and bens_fill_slot,
// eqf_batch_ensemble_output_host.hpp's bens_output_state (the second place G and its lazy allocation), and BatchDevice, HIPCHK / EQFCHK / blocks.
//
// The file has two halves. The first is the PLAN - per entry which landmarks a cloud keeps, drops and gains and where the kept ones come from, and per call
// the refusals (bens_follow_screen) - as functions of id lists that make no HIP call and need nothing of the translation unit but the error codes: with
// EQF_BENS_FOLLOW_PLAN_ONLY defined the file ends behind it, so that a stand-alone program can include and drive it. The second half is the call: screen,
// one packet in, the fixed chain of launches on the batch's stream, the pivot flags back, then the host's id lists, kept-weight flags and counters.
#pragma once
#include "eqf_batch_ensemble_follow.h"
#include <algorithm>
#include <utility>
#include <vector>

namespace {
constexpr int BENS_FOLLOW_L = 64; // landmarks of a slot and of a cloud at the most (EQF_BATCH_MAX_LANDMARKS)
struct BensFollowPlan {
    int nK = 0, nD = 0, nA = 0; // kept, dropped, added
    bool noop = false;          // nothing dropped, nothing added, every kept landmark at its place: nothing is touched
    bool moves = false;         // a kept landmark changes its place
    int from[BENS_FOLLOW_L] = {}; // i < nK: the cloud's old place of the slot's landmark i
};
// The plan of one entry from the slot's ids F (N of them, in state order) and the cloud's ids G (NG of them, distinct, in any order) with P particles.
// 0 and the plan, or the entry's code: EQF_E_BAD_ARG an empty cloud, EQF_E_UNSUPPORTED the suffix rule is broken (an id the cloud lacks sits in front of one
// it holds in the slot's order). Sizes beyond 64 cannot come from an eqf_bens; they are EQF_E_CAPACITY here.
int bens_follow_plan(const int* F, int N, const int* G, int NG, int P, BensFollowPlan& pl) {
    pl = BensFollowPlan();
    if (P < 1 || N < 0 || NG < 0 || (N > 0 && !F) || (NG > 0 && !G))
        return EQF_E_BAD_ARG;
    if (N > BENS_FOLLOW_L || NG > BENS_FOLLOW_L)
        return EQF_E_CAPACITY;
    std::vector<std::pair<int, int>> mine(NG);
    for (int t = 0; t < NG; ++t)
        mine[t] = {G[t], t};
    std::sort(mine.begin(), mine.end());
    bool missing = false;
    for (int i = 0; i < N; ++i) {
        const auto it = std::lower_bound(mine.begin(), mine.end(), std::make_pair(F[i], -1));
        const bool held = it != mine.end() && it->first == F[i];
        if (held && missing)
            return EQF_E_UNSUPPORTED;
        if (!held) {
            missing = true;
            continue;
        }
        pl.from[pl.nK] = it->second;
        pl.moves = pl.moves || it->second != pl.nK;
        ++pl.nK;
    }
    pl.nA = N - pl.nK;
    pl.nD = NG - pl.nK;
    pl.noop = pl.nA == 0 && pl.nD == 0 && !pl.moves;
    return 0;
}
// What the screening reads of one slot: the slot's ids in state order, the cloud's ids, its particles.
struct BensFollowView {
    const int* F;
    int N;
    const int* G;
    int NG, P;
};
// The screening of a whole call, before any device work: status[t] and, where it is 0, plans[t] for every entry. EQF_E_BAD_ARG for a slot outside
// [0, slots) or one an earlier entry of the call has listed (refused or not); otherwise the entry's plan or its code.
void bens_follow_screen(int slots, const BensFollowView* views, int count, const int* entry_slots, BensFollowPlan* plans, int* status) {
    std::vector<char> listed(slots > 0 ? slots : 0, 0);
    for (int t = 0; t < count; ++t) {
        const int slot = entry_slots[t];
        if (slot < 0 || slot >= slots || listed[slot]) {
            status[t] = EQF_E_BAD_ARG;
            continue;
        }
        listed[slot] = 1;
        const BensFollowView& v = views[slot];
        status[t] = bens_follow_plan(v.F, v.N, v.G, v.NG, v.P, plans[t]);
    }
}
} // namespace

#ifndef EQF_BENS_FOLLOW_PLAN_ONLY
static_assert(BENS_FOLLOW_L == BATCH_L, "the plan's landmark capacity is the batch's");

int eqf_bens_follow(eqf_bens* e, int count, const eqf_bens_follow_entry* entries, int* n_dropped, int* n_added, int* status) {
    if (!e || count < 0 || (count > 0 && (!entries || !status)))
        return EQF_E_BAD_ARG;
    if (count == 0)
        return 0;
    struct Todo {
        int t; // the call's entry
        BensFollowPlan pl;
    };
    std::vector<BensFollowView> views(e->b->slots);
    for (int k = 0; k < e->b->slots; ++k)
        views[k] = BensFollowView{e->b->s[k].ids.data(), (int)e->b->s[k].ids.size(), e->c[k].ids.data(), e->c[k].N, e->c[k].P};
    std::vector<int> slots_of(count);
    for (int t = 0; t < count; ++t)
        slots_of[t] = entries[t].slot;
    std::vector<BensFollowPlan> plans(count);
    bens_follow_screen(e->b->slots, views.data(), count, slots_of.data(), plans.data(), status);
    std::vector<Todo> add, move, host; // accepted entries that add (device work, a factorisation), that only move planes, that change the id list alone
    for (int t = 0; t < count; ++t) {
        if (status[t])
            continue;
        const Todo td{t, plans[t]};
        if (td.pl.noop) { // nothing is touched: the kept weights stand
            if (n_dropped)
                n_dropped[t] = 0;
            if (n_added)
                n_added[t] = 0;
            continue;
        }
        (td.pl.nA > 0 ? add : (td.pl.moves ? move : host)).push_back(td);
    }
    const int nadd = (int)add.size(), nin = nadd + (int)move.size();
    bool anymove = !move.empty();
    for (const Todo& td : add)
        anymove = anymove || td.pl.moves;
    if (nin > 0) {
        BatchDevice dev(e->b);
        BensOutState* os = nullptr;
        if (anymove)
            EQFCHK(bens_output_state(e, os)); // the second place: EQF_E_CAPACITY for the call, nothing touched
        const size_t B = (size_t)e->b->slots;
        if (!e->fd) {
            char* p = nullptr;
            EQFCHK(bens_alloc(e, p, B * (2 * sizeof(BensIn) + sizeof(BensFollowIn))));
            e->fd = p;
        }
        // one packet: [errors' entries, N = the kept landmarks | the factor's entries, N = the slot's | the entries of this file's kernels], adding ones first
        const size_t off_fac = sizeof(BensIn) * nadd, off_fol = 2 * off_fac, bytes = off_fol + sizeof(BensFollowIn) * nin;
        e->h.resize((bytes + sizeof(double) - 1) / sizeof(double));
        char* hp = reinterpret_cast<char*>(e->h.data());
        BensIn* h_err = reinterpret_cast<BensIn*>(hp);
        BensIn* h_fac = reinterpret_cast<BensIn*>(hp + off_fac);
        BensFollowIn* h_fol = reinterpret_cast<BensFollowIn*>(hp + off_fol);
        int Pmax = 1, Nmax = 0, PmaxA = 1, NKmax = 0;
        for (int q = 0; q < nin; ++q) {
            const Todo& td = q < nadd ? add[q] : move[q - nadd];
            const eqf_bens_follow_entry& fe = entries[td.t];
            BensIn in;
            bens_fill_slot(e, fe.slot, in);
            BensFollowIn& f = h_fol[q];
            std::memset(&f, 0, sizeof(BensFollowIn));
            f.slot = fe.slot;
            f.cur = in.cur;
            f.N = in.N;
            f.P = in.P;
            f.nK = td.pl.nK;
            f.chart = in.chart;
            std::copy_n(td.pl.from, td.pl.nK, f.from);
            Pmax = std::max(Pmax, in.P);
            Nmax = std::max(Nmax, in.N);
            if (q >= nadd)
                continue;
            f.seed = fe.seed;
            f.stream = fe.stream;
            h_fac[q] = in;
            in.N = td.pl.nK;
            std::copy_n(td.pl.from, td.pl.nK, in.match);
            h_err[q] = in;
            PmaxA = std::max(PmaxA, in.P);
            NKmax = std::max(NKmax, td.pl.nK);
        }
        hipStream_t st = e->b->stream;
        char* dp = static_cast<char*>(e->fd);
        HIPCHK(hipMemcpyAsync(dp, hp, bytes, hipMemcpyHostToDevice, st));
        const BensFollowArgs fa{e->b->buf, e->eb, anymove ? os->ob.G : nullptr, reinterpret_cast<const BensFollowIn*>(dp + off_fol), nadd};
        if (nadd > 0) {
            const BensArgs a_err{e->b->buf, e->eb, reinterpret_cast<const BensIn*>(dp)};
            const BensArgs a_fac{e->b->buf, e->eb, reinterpret_cast<const BensIn*>(dp + off_fac)};
            hipLaunchKernelGGL(k_bens_errors, dim3(blocks(PmaxA, BATCH_T), 1 + NKmax, nadd), dim3(BATCH_T), 0, st, a_err);
            hipLaunchKernelGGL(k_bens_factor, dim3(nadd), dim3(BATCH_T), 0, st, a_fac);
            hipLaunchKernelGGL(k_bens_follow_eps, dim3(blocks(PmaxA, 16), nadd), dim3(64), 0, st, fa);
            e->launches += 3;
            e->factorisations += nadd;
        }
        const dim3 grid(blocks(Pmax, BATCH_T), std::max(Nmax, 1), nin);
        if (anymove) {
            hipLaunchKernelGGL(k_bens_follow_place, grid, dim3(BATCH_T), 0, st, fa, 0);
            ++e->launches;
        }
        hipLaunchKernelGGL(k_bens_follow_place, grid, dim3(BATCH_T), 0, st, fa, 1);
        ++e->launches;
        HIPCHK(hipGetLastError());
        if (nadd > 0)
            HIPCHK(hipMemcpyAsync(e->flag.h, e->flag.d, sizeof(int) * nadd, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    // the host's half, behind the flags: the id lists, the kept weights, the counts
    for (const std::vector<Todo>* list : {&add, &move, &host})
        for (size_t q = 0; q < list->size(); ++q) {
            const Todo& td = (*list)[q];
            const int slot = entries[td.t].slot;
            if (list == &add && e->flag.h[q]) {
                status[td.t] = EQF_E_NOT_SPD; // the planes have not moved
                continue;
            }
            e->c[slot].ids = e->b->s[slot].ids;
            e->c[slot].N = (int)e->c[slot].ids.size();
            e->w_valid[slot] = 0;
            if (n_dropped)
                n_dropped[td.t] = td.pl.nD;
            if (n_added)
                n_added[td.t] = td.pl.nA;
        }
    return 0;
}
#endif
