"""The shard route (dlsm_shard_route_dev) on the CPU.

tests/cpp/shard_route_test.cc: the shard search the kernels run
(dlsm_amd/csrc/shard_route.h) against std::map<std::string, int>::upper_bound
on adversarial bounds, the planner and a host model of the passes against a
stable sort -- built twice as a stand-alone program, plain and under
AddressSanitizer + UBSan.  tests/cpp/adapter_shard_test.cc: the adapter's
ShardRouter::Shard and host route on the same cases, and the C ABI's argument
checks.  No GPU needed.  DBImpl_Sharding needs the RDMA Env and cannot run
here, so these cases are hand-derived from db/db_impl_sharding.h:41-55 and
include/TimberSaw/slice.h:112-122."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shard_route_test.cc")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(exe, env=None):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout[-4000:] + out.stderr[-4000:]
    return out


def test_shard_route_host(tmp_path):
    exe = tmp_path / "shard_route_test"
    subprocess.run(["g++", "-O2"] + FLAGS + [SRC, "-o", str(exe)], check=True)
    _run(exe)


def test_shard_route_host_under_asan_ubsan(tmp_path):
    exe = tmp_path / "shard_route_test_san"
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("clang++")
    assert cxx, "clang++ (ROCm LLVM) is needed for the sanitizer build"
    subprocess.run([cxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                   [SRC, "-o", str(exe)], check=True)
    out = _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


def test_route_kernels_use_no_scratch(tmp_path):
    """The count and scatter kernels run two 1,024-thread workgroups per CU: no
    spill (DESIGN §6 on scratch under that shape).  Compiled for gfx950 on the
    CPU, read from the compiler's resource usage."""
    import re

    src = os.path.join(ROOT, "dlsm_amd", "csrc", "shard_route.hip")
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
    route = {k: v for k, v in usage.items() if "route_" in k}
    assert len(route) == 6, sorted(usage)  # count x 2, scan, scatter x 3
    assert all(v == 0 for v in route.values()), route


def compile_adapter_shard_test(tmp_path):
    exe = tmp_path / "adapter_shard_test"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fno-rtti", "-fno-exceptions", "-pthread",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "adapter_shard_test.cc"),
                    "-L", os.path.join(ROOT, "dlsm_amd", "lib"), "-ldlsm_bloom",
                    "-Wl,-rpath," + os.path.join(ROOT, "dlsm_amd", "lib"),
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", str(exe)], check=True)
    return exe


def test_adapter_shard_router_on_cpu(tmp_path):
    exe = compile_adapter_shard_test(tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK adapter shard host" in out.stdout, out.stdout + out.stderr


def test_abi_argument_checks_without_a_device():
    """Bounds out of order, n_shards of 0 and 512 and NULL arguments are
    DLSM_E_ARG before any device is touched (the context is NULL here)."""
    import dlsm_amd
    from dlsm_amd import _lib as L

    lib = dlsm_amd.lib()

    def create(bounds, n=None, ptrs=True, lens=True):
        arrs = [C.create_string_buffer(bytes(b), len(b) + 1) for b in bounds]
        pa = (C.c_void_p * max(len(bounds), 1))(*[C.addressof(a) for a in arrs])
        la = (C.c_uint64 * max(len(bounds), 1))(*[len(b) for b in bounds])
        h = C.c_void_p(1)
        st = lib.dlsm_shardmap_create(None, pa if ptrs else None, la if lens else None,
                                      len(bounds) if n is None else n, C.byref(h))
        assert h.value is None
        return st

    assert create([b"b", b"a"]) == L.DLSM_E_ARG
    assert create([b"a", b"a"]) == L.DLSM_E_ARG
    assert create([b"ab", b"a"]) == L.DLSM_E_ARG
    assert create([b"a", b"b"], n=0) == L.DLSM_E_ARG
    many = [bytes([i >> 8, i & 255]) for i in range(512)]
    assert create(many) == L.DLSM_E_ARG              # 512 shards
    assert create([b"a", b"b"], ptrs=False) == L.DLSM_E_ARG
    assert create([b"a", b"b"], lens=False) == L.DLSM_E_ARG
    assert create([b"a", b"b"]) == L.DLSM_E_ARG      # well-formed bounds, NULL context
    assert lib.dlsm_shardmap_create(None, None, None, 1, None) == L.DLSM_E_ARG
    assert dlsm_amd.shard_route_cap(0, 1) == 8
    assert dlsm_amd.shard_route_cap(5, 16) == 56     # 5 + 3 * 17
    assert dlsm_amd.shard_route_cap(6, 16) == 60     # 57 rounded up
    assert dlsm_amd.shard_route_cap(1, 511) == 1540
    assert dlsm_amd.MAX_SHARDS == 511 and dlsm_amd.ROUTE_ALIGN == 4
    c = dlsm_amd.shard_route_chunk()
    assert c >= 64 and c % 64 == 0
