// trackformer_amd/csrc/msda_dispatch.h -- the host-side dispatch layer of the MSDeformAttn kernels, shared by
// msda_hip.hip and msda_pquad.hip (host code only): option tables, the tile-plan memo and the tile counting function,
// on top of the family-neutral host_dispatch.h (kernel variants, 0/1 environment flags, the dynamic-LDS limit).
#ifndef TF_MSDA_DISPATCH_H_
#define TF_MSDA_DISPATCH_H_

#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>

#include "host_dispatch.h"
#include "launch_status.h"
#include "msda_common.h"

namespace tfm {

// TF_MSDA_VERBOSE: on when set, to whatever value
inline bool msda_verbose()
{
    static const bool on = getenv("TF_MSDA_VERBOSE") != nullptr;
    return on;
}

// Largest number of queries any TH x TW tile holds (exact, same integer partition as the kernels: tfq_tile_bound).
inline long long tile_max_queries(const LevelTable &lt, int L, int th, int tw)
{
    const int H0 = lt.H[0], W0 = lt.W[0];
    long long max_nq = 0;
    for (int y0 = 0; y0 < H0; y0 += th)
        for (int x0 = 0; x0 < W0; x0 += tw) {
            const int y1 = (y0 + th < H0) ? y0 + th : H0, x1 = (x0 + tw < W0) ? x0 + tw : W0;
            long long nq = 0;
            for (int l = 0; l < L; ++l) {
                const long long Hl = lt.H[l], Wl = lt.W[l];
                const long long ny = (2 * y1 * Hl + H0 - 1) / (2LL * H0) - (2 * y0 * Hl + H0 - 1) / (2LL * H0);
                const long long nx = (2 * x1 * Wl + W0 - 1) / (2LL * W0) - (2 * x0 * Wl + W0 - 1) / (2LL * W0);
                nq += ny * nx;
            }
            if (nq > max_nq) max_nq = nq;
        }
    return max_nq;
}

// Process-wide integer knobs of one kernel family: set by name (tf_msda_set_option) or, before the first use, from a
// comma-separated key=value list in the environment (TF_MSDA_QUAD="ta=12,waves=8", TF_MSDA_PQUAD="on=0").  Every
// change bumps the epoch, which invalidates the per-thread tile plans.
template <int N>
struct OptionTable {
    const char *env;
    const char *const *names;   // tf_msda_set_option
    const char *const *keys;    // environment list
    const int *defaults;
    std::atomic<int> value[N];
    std::atomic<int> epoch_{0};
    std::once_flag once;

    void init()
    {
        std::call_once(once, [this] {
            for (int i = 0; i < N; ++i) value[i].store(defaults[i]);
            const char *p = getenv(env);
            while (p && *p) {
                const char *eq = strchr(p, '=');
                if (!eq) break;
                for (int i = 0; i < N; ++i)
                    if ((size_t)(eq - p) == strlen(keys[i]) && strncmp(p, keys[i], eq - p) == 0) value[i].store(atoi(eq + 1));
                const char *c = strchr(eq, ',');
                p = c ? c + 1 : nullptr;
            }
        });
    }
    // every value, and the epoch they belong to
    int load(int (&o)[N])
    {
        init();
        for (int i = 0; i < N; ++i) o[i] = value[i].load(std::memory_order_relaxed);
        return epoch_.load(std::memory_order_relaxed);
    }
    // the previous value, or `unknown` when the table has no such name
    int set(const char *name, int v, int unknown = INT_MIN)
    {
        init();
        for (int i = 0; i < N; ++i)
            if (strcmp(name, names[i]) == 0) {
                const int prev = value[i].exchange(v);
                epoch_.fetch_add(1);
                return prev;
            }
        return unknown;
    }
};

// Per-thread memo of the last tile plan: the plan (or the refusal) made for this key and level table.
//     static thread_local PlanMemo<P, K> memo;
//     if (memo.hit({...}, lt)) { *out = memo.plan; return memo.ok; }      -- a miss records the key, as a refusal
//     ...  memo.keep(plan);
template <typename P, int K>
struct PlanMemo {
    bool valid = false, ok = false;
    int key[K];
    LevelTable lt;
    P plan;

    bool hit(const int (&k)[K], const LevelTable &t)
    {
        if (valid && memcmp(key, k, sizeof(key)) == 0 && memcmp(&lt, &t, sizeof(lt)) == 0) return true;
        valid = true;
        ok = false;
        memcpy(key, k, sizeof(key));
        lt = t;
        return false;
    }
    void keep(const P &p)
    {
        plan = p;
        ok = true;
    }
};

}  // namespace tfm

#endif  // TF_MSDA_DISPATCH_H_
