"""The read plan on the CPU (tests/cpp/read_plan_test.cc): the task decoder of
dlsm_amd/csrc/read_plan.h against brute force (every slot, empty levels, picks
at count-1, count and UINT32_MAX, bits at and above n_slots), the planner in
dlsm_amd/csrc/host_plan.h (digits, grid, workspace layout) and a host model of
the histogram / scan / scatter passes against a stable sort.  Built twice as a
stand-alone program: plain, and under AddressSanitizer + UBSan.  The kernels are
compiled for gfx950 and must use no scratch.  No GPU needed."""
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


def test_plan_kernels_use_no_scratch(tmp_path):
    """The histogram and scatter kernels run two 1,024-thread workgroups per CU:
    no spill (DESIGN §6 on scratch under that shape).  Compiled for gfx950 on
    the CPU, read from the compiler's resource usage."""
    import re

    src = os.path.join(ROOT, "dlsm_amd", "csrc", "read_plan.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--offload-device-only", "-c", src, "-o", str(tmp_path / "k.o"),
                        "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            usage[name] = int(m.group(1))
    plan = {k: v for k, v in usage.items() if "plan_" in k or "masks_advance" in k}
    assert len(plan) == 12, sorted(usage)  # hist x 3, scan, scatter x 6, bounds, masks_advance
    assert all(v == 0 for v in plan.values()), plan
