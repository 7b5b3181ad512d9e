"""Memory check of the verbose-mapping reader (ntl_vmap_*, ntlink_amd/csrc/ntl_io.cpp): tests/pool/vmap_check.cpp feeds it truncated
files, lines without a newline at the end, empty tokens and 11-digit numbers.  A stand-alone program with its own main, built with g++
and AddressSanitizer / UBSan together with ntl_io.cpp and run as a child process: no GPU, no Python extension."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# (the sanitizers' runtimes are linked statically: the program stands alone, whatever else the process's environment loads)
def test_vmap_check(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path / "vmap_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", os.path.join(ROOT, "tests", "pool", "vmap_check.cpp"),
                           os.path.join(ROOT, "ntlink_amd", "csrc", "ntl_io.cpp"), "-o", exe, "-lz", "-ldl", "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", NTL_IO_THREADS="4")
    env.pop("NTL_IO_MIN_CHUNK", None)
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and "vmap_check: ok" in run.stdout and "Sanitizer" not in run.stderr, run.stdout[-4000:] + run.stderr[-4000:]
