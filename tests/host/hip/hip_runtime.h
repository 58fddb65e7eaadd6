// TEST INFRASTRUCTURE: the few HIP runtime calls trackformer_amd/csrc/host_dispatch.h and launch_status.h make, as a host stub for
// tests/host/lds_limit_threads.cpp and tests/host/launch_status.cpp -- a current device per thread that the test sets, a
// hipFuncSetAttribute that counts its calls per (function, device), and a hipGetLastError that returns what the test set
// on that thread.  No GPU, no ROCm headers.
#ifndef TF_TEST_HIP_STUB_H_
#define TF_TEST_HIP_STUB_H_

#include <atomic>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
constexpr int hipFuncAttributeMaxDynamicSharedMemorySize = 8;
struct hipDeviceProp_t {
    int multiProcessorCount;
};

namespace hipstub {
constexpr int kFunctions = 300, kDevices = 65;
extern char functions[kFunctions];                          // &functions[i]: the "kernel" i
extern std::atomic<int> raised[kFunctions][kDevices];       // hipFuncSetAttribute calls per (function, device)
extern thread_local int device;
inline thread_local hipError_t last_error = hipSuccess;     // what hipGetLastError returns on this thread
}  // namespace hipstub

inline hipError_t hipGetDevice(int *dev)
{
    *dev = hipstub::device;
    return hipSuccess;
}
inline hipError_t hipGetLastError() { return hipstub::last_error; }
inline hipError_t hipGetDeviceProperties(hipDeviceProp_t *prop, int)
{
    prop->multiProcessorCount = 4;
    return hipSuccess;
}
inline hipError_t hipFuncSetAttribute(const void *fn, int, int)
{
    hipstub::raised[static_cast<const char *>(fn) - hipstub::functions][hipstub::device].fetch_add(1, std::memory_order_relaxed);
    return hipSuccess;
}

#endif  // TF_TEST_HIP_STUB_H_
