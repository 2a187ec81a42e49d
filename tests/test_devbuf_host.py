"""The owners of device memory (csrc/mg_devbuf.h: DevBuf, DVector, DevTemp) under AddressSanitizer and
UndefinedBehaviorSanitizer, without a GPU: tests/host/devbuf_check.cpp compiles the header against a counting stand-in
for hipMalloc / hipFree / hipMemsetAsync / hipGetErrorString and runs as a program of its own."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffer_types_are_clean_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "devbuf_check")
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    # the sanitizer runtime linked into the program itself (GCC links it as a shared library unless told otherwise)
    static = ["-static-libsan"] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *static, "-o", exe,
                            os.path.join(ROOT, "tests", "host", "devbuf_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    # (leaks are the stand-in's to count: it knows every live allocation; LeakSanitizer needs ptrace rights a test user may lack)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ledger at zero" in run.stdout
