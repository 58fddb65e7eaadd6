// TEST INFRASTRUCTURE: raise_dynamic_lds_limit (trackformer_amd/csrc/host_dispatch.h) under threads, as a stand-alone host
// program over the HIP stub next to it; tests/test_host_dispatch_threads.py builds it with -fsanitize=thread and with
// -fsanitize=address,undefined and runs it.  8 threads call the helper for more functions than the table has slots on 4
// devices, each in an order of its own.  A function that got a slot has every (function, device) pair raised exactly once;
// one that arrived at a full table is raised on every call and still succeeds; a device without a bit in the mask is refused
// without a call.  Prints "ok" and returns 0, or says what it found and returns 1.
#include <stdio.h>

#include <thread>
#include <vector>

#include "host_dispatch.h"

namespace hipstub {
char functions[kFunctions];
std::atomic<int> raised[kFunctions][kDevices];
thread_local int device = 0;
}  // namespace hipstub

int main()
{
    constexpr int kThreads = 8, kDevs = 4, kRounds = 3, kFns = tfm::kLdsLimitSlots + 40;
    static_assert(kFns <= hipstub::kFunctions, "the stub holds every function");
    std::atomic<int> failed{0};
    std::vector<std::thread> threads;
    for (int t = 0; t < kThreads; ++t)
        threads.emplace_back([t, &failed] {
            for (int round = 0; round < kRounds; ++round)
                for (int i = 0; i < kFns; ++i) {
                    const int f = (i * (2 * t + 1) + 37 * t) % kFns;   // an odd stride: every function once per round
                    for (int d = 0; d < kDevs; ++d) {
                        hipstub::device = (d + t) % kDevs;
                        if (!tfm::raise_dynamic_lds_limit(&hipstub::functions[f])) failed.fetch_add(1);
                    }
                }
        });
    for (std::thread &th : threads) th.join();
    int once = 0, always = 0, other = 0;
    for (int f = 0; f < kFns; ++f) {
        int n1 = 0, nall = 0;
        for (int d = 0; d < kDevs; ++d) {
            const int n = hipstub::raised[f][d].load();
            n1 += n == 1;
            nall += n == kThreads * kRounds;
        }
        if (n1 == kDevs) ++once;
        else if (nall == kDevs) ++always;
        else ++other;
    }
    hipstub::device = 64;   // no bit in a slot's mask
    const bool refused = !tfm::raise_dynamic_lds_limit(&hipstub::functions[0]) && hipstub::raised[0][64].load() == 0;
    const bool ok = failed.load() == 0 && once == tfm::kLdsLimitSlots && always == kFns - tfm::kLdsLimitSlots && other == 0 && refused && tfm::num_cus() == 4;
    printf("%s: %d calls failed; %d functions raised once per device (slots: %d), %d on every call, %d otherwise; device 64 %s\n", ok ? "ok" : "FAILED",
           failed.load(), once, tfm::kLdsLimitSlots, always, other, refused ? "refused" : "NOT refused");
    return ok ? 0 : 1;
}
