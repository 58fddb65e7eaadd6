"""The launch status of csrc/launch_status.h (record_hip / launched: what tf_msda_last_hip_error reports) on the CPU:
tests/host/launch_status.cpp -- a stand-alone program with its own main over a HIP stub (tests/host/hip/hip_runtime.h) -- is
built with the host compiler, plain and with ThreadSanitizer, and run as a plain executable.  The program checks that a
success leaves the stored code alone, that a failure is stored on the failing thread only and that a later success keeps it;
a sanitizer report makes it exit non-zero.  No launch fails anywhere: the stub's hipGetLastError returns what the program
set.  Nothing that is loaded into Python is sanitised."""
import os
import subprocess

import pytest

from tests.emu import build_emu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "trackformer_amd", "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")


@pytest.mark.parametrize("sanitizer", [None, "thread"])
def test_launch_status_per_thread(sanitizer, tmp_path):
    cxx = build_emu.find_compiler()
    if cxx is None:
        pytest.skip("no host clang++")
    exe = str(tmp_path / "launch_status")
    flags = ["-fsanitize=" + sanitizer, "-fno-sanitize-recover=all"] if sanitizer else []
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-pthread"] + flags + [
        "-I", os.path.join(HERE, "host"), "-I", CSRC, "-I", INCLUDE, os.path.join(HERE, "host", "launch_status.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if sanitizer and built.returncode != 0 and ("libclang_rt" in built.stderr or "sanitizer" in built.stderr.lower()):
        pytest.skip("the host compiler has no -fsanitize=%s runtime" % sanitizer)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok") and "Sanitizer" not in run.stderr
