// trackformer_amd/csrc/msda_dispatch.h -- the host-side dispatch layer of the MSDeformAttn kernels, shared by
// msda_hip.hip and msda_pquad.hip (host code only): kernel variants, option tables, 0/1 environment flags, the
// dynamic-LDS limit, the tile-plan memo and the tile counting function.
#ifndef TF_MSDA_DISPATCH_H_
#define TF_MSDA_DISPATCH_H_

#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>

#include "msda_common.h"

namespace tfm {

// A kernel and the name tf_msda_last_kernel reports for it, chosen together by one selection function per kernel
// family: the launch and note_kernel use the same variant.  `name` is a string literal.
struct KernelVariant {
    const void *fn;
    const char *name;
};

// 0/1 environment flag: unset -> dflt, set -> off only when its first character is '0'.  (Read once by the caller:
// `static const bool on = env_flag(...)`.)
inline bool env_flag(const char *name, bool dflt)
{
    const char *e = getenv(name);
    return e ? e[0] != '0' : dflt;
}
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

// The dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) is an attribute of a function ON A DEVICE: raised
// once per (function, current device).  One slot per function with a bit per device (64 devices; the slots outnumber
// the ~60 instantiations that need it); a hit reads two atomics, the first use of a pair takes the lock.
constexpr int kLdsLimitSlots = 128;
struct LdsLimitSlot {
    std::atomic<const void *> fn{nullptr};
    std::atomic<unsigned long long> devs{0};
};
// The slot of `fn` (slots fill in order and are never released), or null.
inline LdsLimitSlot *lds_limit_find(LdsLimitSlot *slots, const void *fn)
{
    for (int i = 0; i < kLdsLimitSlots; ++i) {
        const void *f = slots[i].fn.load(std::memory_order_acquire);
        if (f == fn) return &slots[i];
        if (!f) break;
    }
    return nullptr;
}
inline bool raise_dynamic_lds_limit(const void *fn)
{
    static LdsLimitSlot slots[kLdsLimitSlots];
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    const unsigned long long bit = 1ull << dev;
    LdsLimitSlot *s = lds_limit_find(slots, fn);
    if (s && (s->devs.load(std::memory_order_acquire) & bit)) return true;
    std::lock_guard<std::mutex> guard(mu);
    s = lds_limit_find(slots, fn);
    if (s && (s->devs.load(std::memory_order_relaxed) & bit)) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return false;
    for (int i = 0; !s && i < kLdsLimitSlots; ++i)
        if (!slots[i].fn.load(std::memory_order_relaxed)) {
            s = &slots[i];
            s->fn.store(fn, std::memory_order_release);
        }
    if (s) s->devs.fetch_or(bit, std::memory_order_release);
    return true;
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
