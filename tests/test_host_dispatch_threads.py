"""raise_dynamic_lds_limit (csrc/host_dispatch.h) under threads and sanitizers, on the CPU: tests/host/lds_limit_threads.cpp
-- a stand-alone program with its own main over a HIP stub (tests/host/hip/hip_runtime.h) -- is built with the host
compiler's ThreadSanitizer, then with AddressSanitizer + UndefinedBehaviorSanitizer, and run as a plain executable.  The
program checks the counts (every pair inside the table raised exactly once, pairs beyond it still succeed); a sanitizer
report makes it exit non-zero.  Nothing that is loaded into Python is sanitised."""
import os
import subprocess

import pytest

from tests.emu import build_emu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "trackformer_amd", "csrc")


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_lds_limit_helper_under_threads(sanitizer, tmp_path):
    cxx = build_emu.find_compiler()
    if cxx is None:
        pytest.skip("no host clang++")
    exe = str(tmp_path / "lds_limit_threads")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all",
           "-I", os.path.join(HERE, "host"), "-I", CSRC, os.path.join(HERE, "host", "lds_limit_threads.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("libclang_rt" in built.stderr or "sanitizer" in built.stderr.lower()):
        pytest.skip("the host compiler has no -fsanitize=%s runtime" % sanitizer)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.startswith("ok") and "Sanitizer" not in run.stderr
