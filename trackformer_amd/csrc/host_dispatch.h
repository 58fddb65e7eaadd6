// trackformer_amd/csrc/host_dispatch.h -- host-side launch plumbing shared by every translation unit of libtf_msda.so,
// MSDeformAttn and dense alike (host code only): kernel variants, 0/1 environment flags, the dynamic-LDS limit, the
// compute-unit count and the process-wide knobs of the dense kernels.  What needs a LevelTable is in msda_dispatch.h.
#ifndef TF_HOST_DISPATCH_H_
#define TF_HOST_DISPATCH_H_

#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <atomic>
#include <mutex>

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

// Compute units of the device that was current at the first call, for the whole process (256 when it cannot be read).
// The block-shape rules of msda_pquad.hip, ffn_fused.hip and linear_stream.hip each kept such a static of their own;
// on a machine of identical cards this one holds what those three held.
inline int num_cus()
{
    static const int n = [] {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
        }
        return cus;
    }();
    return n;
}

// The dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) is an attribute of a function ON A DEVICE: raised
// once per (function, current device), to the 160 KB of a CU whatever the launch asks for -- the attribute is the bound
// a launch's dynamic LDS size is checked against, not an allocation; the launch passes its real size.  One slot per
// function with a bit per device (64 devices); a hit reads two atomics per slot walked, the first use of a pair takes
// the lock.  A full table stays correct (the pair is raised again on every launch), so the slots outnumber the
// instantiations that can get here, as counted in the built code objects: 59 of MSDeformAttn (32 msda_fwd_f32_quad, 16
// msda_fwd_f32_pquad, 10 msda_fwd_f32_pquad2, msda_bwd_f32_sorted2) and 64 dense ones (18 ffn_fused_kernel, 18
// linear_res_ln_kernel, 4 linear_groups_kernel, 8 dma_gemm_kernel, 16 attention kernels; most launchers ask only when
// the tile exceeds 64 KB, so fewer arrive) -- 123 of 256.
constexpr int kLdsLimitSlots = 256;
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

// The process-wide knobs of the dense kernels (tf_msda_set_option; include/tf_msda.h has what each one selects).  One
// descriptor per knob in msda_hip.hip (kDenseKnobs): its name, the environment variable read at its first use, its
// default, and what a value outside its range becomes -- the same rule for the environment and for the setter.
enum DenseKnob { kKnobFfnTi, kKnobFfnTailSplit, kKnobLinlnTi, kKnobGroupsTi, kKnobLinearStreamTi, kKnobConvHalo, kKnobLinearDma,
                 kKnobMhaMfma, kKnobWgradMsplit, kKnobCount };
int dense_knob(DenseKnob k);                                // the value in force
int dense_knob_set(const char *name, int v, int unknown);   // the value that was in force, or `unknown`: no such knob

}  // namespace tfm

#endif  // TF_HOST_DISPATCH_H_
