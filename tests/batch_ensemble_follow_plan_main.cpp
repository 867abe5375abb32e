// Stand-alone driver of eqf_bens_follow's plan (eqvio_amd/csrc/eqf_batch_ensemble_follow_host.hpp, first half): no HIP, no device, no library.
// tests/test_batch_ensemble_follow_api.py builds it with g++ -fsanitize=address,undefined and runs it.
// stdin, any number of calls:
//   slots
//   P N f_0 .. f_(N-1) NG g_0 .. g_(NG-1)        once per slot: the cloud's particles, the slot's ids in state order, the cloud's ids
//   count s_0 .. s_(count-1)                     the call's entries
// stdout, one line per entry: status, and where it is 0: nK nD nA noop moves from_0 .. from_(nK-1)
#define EQF_BENS_FOLLOW_PLAN_ONLY
#include "../eqvio_amd/csrc/eqf_batch_ensemble_follow_host.hpp"

#include <cstdio>
#include <iostream>
#include <memory>
#include <vector>

int main() {
    int slots;
    while (std::cin >> slots) {
        // exactly-sized heap arrays: a read past either end of an id list is an AddressSanitizer report
        std::vector<std::unique_ptr<int[]>> own;
        std::vector<BensFollowView> views(slots);
        for (BensFollowView& v : views) {
            std::cin >> v.P >> v.N;
            own.emplace_back(new int[v.N > 0 ? v.N : 0]);
            for (int i = 0; i < v.N; ++i)
                std::cin >> own.back()[i];
            v.F = own.back().get();
            std::cin >> v.NG;
            own.emplace_back(new int[v.NG > 0 ? v.NG : 0]);
            for (int i = 0; i < v.NG; ++i)
                std::cin >> own.back()[i];
            v.G = own.back().get();
        }
        int count;
        std::cin >> count;
        std::unique_ptr<int[]> entry(new int[count]);
        for (int t = 0; t < count; ++t)
            std::cin >> entry[t];
        std::unique_ptr<BensFollowPlan[]> plans(new BensFollowPlan[count]);
        std::unique_ptr<int[]> status(new int[count]);
        bens_follow_screen(slots, views.data(), count, entry.get(), plans.get(), status.get());
        for (int t = 0; t < count; ++t) {
            std::printf("%d", status[t]);
            if (status[t] == 0) {
                const BensFollowPlan& pl = plans[t];
                std::printf(" %d %d %d %d %d", pl.nK, pl.nD, pl.nA, (int)pl.noop, (int)pl.moves);
                for (int i = 0; i < pl.nK; ++i)
                    std::printf(" %d", pl.from[i]);
            }
            std::printf("\n");
        }
    }
    return 0;
}
