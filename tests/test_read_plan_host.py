"""The read plan on the CPU (tests/cpp/read_plan_test.cc): the task decoder of
dlsm_amd/csrc/read_plan.h against brute force (every slot, empty levels, picks
at count-1, count and UINT32_MAX, bits at and above n_slots), the planner in
dlsm_amd/csrc/host_plan.h (digits, grid, workspace layout) and a host model of
the histogram / scan / scatter passes against a stable sort.  Built twice as a
stand-alone program: plain, and under AddressSanitizer + UBSan.  No GPU needed."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "read_plan_test.cc")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(exe, env=None):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout[-4000:] + out.stderr[-4000:]
    return out


def test_read_plan_host(tmp_path):
    exe = tmp_path / "read_plan_test"
    subprocess.run(["g++", "-O2"] + FLAGS + [SRC, "-o", str(exe)], check=True)
    _run(exe)


def test_read_plan_host_under_asan_ubsan(tmp_path):
    exe = tmp_path / "read_plan_test_san"
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("clang++")
    assert cxx, "clang++ (ROCm LLVM) is needed for the sanitizer build"
    subprocess.run([cxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                   [SRC, "-o", str(exe)], check=True)
    out = _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
