"""The crc32c algebra on the CPU (tests/cpp/crc32c_algebra_test.cc): the
host-callable functions of dlsm_amd/csrc/crc32c_dev.h against the known answers
of util/crc32c_test.cc, the table of squares, x^bits against single steps and an
independent square-and-multiply, the word step against four byte steps, the
concatenation identity and the leading-zero rule, and Mask.  Built twice as a
stand-alone program: plain, and under AddressSanitizer + UBSan.  No GPU needed."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "crc32c_algebra_test.cc")
FLAGS = ["-std=c++17"]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(exe, env=None):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout[-4000:] + out.stderr[-4000:]
    return out


def test_crc32c_algebra_host(tmp_path):
    exe = tmp_path / "crc32c_algebra_test"
    subprocess.run(["g++", "-O2"] + FLAGS + [SRC, "-o", str(exe)], check=True)
    _run(exe)


def test_crc32c_algebra_host_under_asan_ubsan(tmp_path):
    exe = tmp_path / "crc32c_algebra_test_san"
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("clang++")
    assert cxx, "clang++ (ROCm LLVM) is needed for the sanitizer build"
    subprocess.run([cxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                   [SRC, "-o", str(exe)], check=True)
    out = _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
