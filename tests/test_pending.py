"""Lazy completion (ntlink_amd/csrc/pending.h) on the host: tests/pool/pending_check.cpp over the scripted HIP runtime
(tests/pool/hip/hip_runtime.h) -- one stream advanced by hand, slots that are a plain array, holds that are counters.  A stand-alone
program with its own main, built with g++ and a sanitizer and run as a child process: no GPU, no Python extension."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL = os.path.join(ROOT, "tests", "pool")


# (the sanitizers' runtimes are linked statically: the program stands alone, whatever else the process's environment loads)
@pytest.mark.parametrize("sanitizer,runtime", [("address,undefined", ["-static-libasan", "-static-libubsan"]), ("thread", ["-static-libtsan"])],
                         ids=["asan_ubsan", "tsan"])
def test_pending_check(sanitizer, runtime, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path / "pending_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all", *runtime,
                           "-I", POOL, os.path.join(POOL, "pending_check.cpp"), "-o", exe, "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="halt_on_error=0 exitcode=66")
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and "pending_check: ok" in run.stdout and "Sanitizer" not in run.stderr, run.stdout[-4000:] + run.stderr[-4000:]
