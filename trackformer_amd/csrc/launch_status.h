// trackformer_amd/csrc/launch_status.h -- the launch status of every entry point of libtf_msda.so (host code only): one
// recorder for the hipError_t behind TF_MSDA_ERR_LAUNCH, shared by every translation unit, MSDeformAttn and dense alike.
#ifndef TF_LAUNCH_STATUS_H_
#define TF_LAUNCH_STATUS_H_

#include <hip/hip_runtime.h>

#include "tf_msda.h"

namespace tfm {

// hipError_t of the most recent FAILING HIP call on this thread, 0 if none (tf_msda_last_hip_error).  An inline variable:
// one per shared object, whichever translation unit records.
inline thread_local int g_last_hip_error = 0;
inline int record_hip(hipError_t e)
{
    if (e == hipSuccess) return TF_MSDA_OK;
    g_last_hip_error = (int)e;
    return TF_MSDA_ERR_LAUNCH;
}
// After a launch written as <<<>>> or hipLaunchKernelGGL.
inline int launched() { return record_hip(hipGetLastError()); }

}  // namespace tfm

#endif  // TF_LAUNCH_STATUS_H_
