// TEST INFRASTRUCTURE: the launch status of trackformer_amd/csrc/launch_status.h (record_hip / launched and the per-thread
// code tf_msda_last_hip_error returns), as a stand-alone host program over the HIP stub next to it;
// tests/test_host_launch_status.py builds it plain and with -fsanitize=thread and runs it.  No launch fails here: the stub's
// hipGetLastError returns what the program set on that thread.
//   * a success returns TF_MSDA_OK and leaves the stored code as it was
//   * a failure on thread A returns TF_MSDA_ERR_LAUNCH and stores its code on A alone: thread B still reads 0
//   * a later success on A leaves the code in place ("the most recent FAILING call")
// Prints "ok" and returns 0, or says what it found and returns 1.
#include <stdio.h>

#include <thread>

#include "launch_status.h"

namespace {
int failures = 0;
void expect(bool cond, const char *what)
{
    if (!cond) {
        printf("FAILED: %s\n", what);
        ++failures;
    }
}
}  // namespace

int main()
{
    // the main thread is thread B: it never fails
    expect(tfm::g_last_hip_error == 0, "the stored code starts at 0");
    hipstub::last_error = hipSuccess;
    expect(tfm::launched() == TF_MSDA_OK, "success returns TF_MSDA_OK");
    expect(tfm::g_last_hip_error == 0, "success leaves the stored code at 0");

    int a_status = 0, a_code = 0, a_later_status = -99, a_later_code = 0, a_direct = 0, a_direct_code = 0;
    std::thread a([&] {
        hipstub::last_error = 719;
        a_status = tfm::launched();
        a_code = tfm::g_last_hip_error;
        hipstub::last_error = hipSuccess;
        a_later_status = tfm::launched();
        a_later_code = tfm::g_last_hip_error;
        a_direct = tfm::record_hip(1);   // the return value of a launch call, not hipGetLastError
        a_direct_code = tfm::g_last_hip_error;
    });
    a.join();
    expect(a_status == TF_MSDA_ERR_LAUNCH, "error 719 on thread A returns TF_MSDA_ERR_LAUNCH");
    expect(a_code == 719, "thread A stores 719");
    expect(a_later_status == TF_MSDA_OK, "a later success on A returns TF_MSDA_OK");
    expect(a_later_code == 719, "a later success on A leaves 719 in place");
    expect(a_direct == TF_MSDA_ERR_LAUNCH && a_direct_code == 1, "record_hip stores the code it is given");
    expect(tfm::g_last_hip_error == 0, "thread B still reads 0");
    expect(tfm::launched() == TF_MSDA_OK && tfm::g_last_hip_error == 0, "thread B still succeeds");

    if (failures == 0) printf("ok: launch status per thread, most recent failing call kept\n");
    return failures == 0 ? 0 : 1;
}
