"""The table index and the index seek (dlsm_tableindex, dlsm_index_seek_dev) on
the CPU.

tests/cpp/index_seek_test.cc: the decoder, comparator, validation rules, fence
window and state decision the kernels run (dlsm_amd/csrc/index_seek.h) against a
linear scan, one block per rejection reason, and the open's planner -- built
twice as a stand-alone program, plain and under AddressSanitizer + UBSan.
tests/cpp/adapter_index_test.cc: the adapter's host::IndexBlockSeek and
TableIndex on the all-host path and under fault injection.  No GPU needed.
Block and BlockBuilder need the RDMA headers and cannot be compiled here, so
the writers in these tests (C++ and dlsm_amd/index_block.py) restate
table/block_builder.cc:74-127 by hand."""
import bisect
import os
import re
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "index_seek_test.cc")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(exe, env=None):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout[-4000:] + out.stderr[-4000:]
    return out


def test_index_seek_host(tmp_path):
    exe = tmp_path / "index_seek_test"
    subprocess.run(["g++", "-O2"] + FLAGS + [SRC, "-o", str(exe)], check=True)
    _run(exe)


def test_index_seek_host_under_asan_ubsan(tmp_path):
    exe = tmp_path / "index_seek_test_san"
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("clang++")
    assert cxx, "clang++ (ROCm LLVM) is needed for the sanitizer build"
    subprocess.run([cxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                   [SRC, "-o", str(exe)], check=True)
    out = _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


def test_index_kernels_use_no_scratch(tmp_path):
    """The seek and open kernels hold no per-lane arrays: no spill.  Compiled
    for gfx950 on the CPU, read from the compiler's resource-usage remarks."""
    src = os.path.join(ROOT, "dlsm_amd", "csrc", "index_seek.hip")
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
    index = {k: v for k, v in usage.items() if "index_" in k}
    assert len(index) == 4, sorted(usage)  # header, entries, seek x 2 (file_begin in LDS or not)
    assert all(v == 0 for v in index.values()), index


def compile_adapter_index_test(tmp_path):
    exe = tmp_path / "adapter_index_test"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fno-rtti", "-fno-exceptions", "-pthread",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "adapter_index_test.cc"),
                    "-L", os.path.join(ROOT, "dlsm_amd", "lib"), "-ldlsm_bloom",
                    "-Wl,-rpath," + os.path.join(ROOT, "dlsm_amd", "lib"),
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", str(exe)], check=True)
    return exe


def test_adapter_table_index_on_cpu(tmp_path):
    exe = compile_adapter_index_test(tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK adapter index host" in out.stdout, out.stdout + out.stderr


def test_python_writer_and_host_seek_against_bisect():
    """dlsm_amd/index_block.py's two writers agree byte for byte, the library's
    host-only check accepts what they write, and dlsm_index_block_seek answers
    like bisect over (user_key, 2**64 - 1 - trailer)."""
    import dlsm_amd
    from dlsm_amd import index_block as ib

    rng = np.random.default_rng(11)
    M = 2**64 - 1
    rows = sorted({(b"%020d" % int(v), int(s), int(t)) for v, s, t in
                   zip(rng.integers(0, 300, 600), rng.integers(1, 50, 600), rng.choice([0, 1, 1, 1, 2], 600))},
                  key=lambda r: (r[0], M - ((r[1] << 8) | r[2])))
    rows = [r for j, r in enumerate(rows) if j == 0 or (r[0], r[1]) != (rows[j - 1][0], rows[j - 1][1])]
    offs = rng.integers(0, 1 << 40, len(rows)).astype(np.uint64) >> rng.integers(0, 40, len(rows)).astype(np.uint64)
    sizes = rng.integers(1, 70_000, len(rows)).astype(np.uint64)
    ikeys = [ib.internal_key(*r) for r in rows]
    contents = ib.build_index_contents(ikeys, list(zip(offs.tolist(), sizes.tolist())))
    fixed = ib.build_index_contents_fixed(np.frombuffer(b"".join(ikeys), dtype=np.uint8).reshape(len(rows), 28),
                                          offs, sizes)
    assert fixed.tobytes() == contents
    assert dlsm_amd.index_block_check(contents) == len(rows)
    assert dlsm_amd.index_block_check(contents[:-4] + struct.pack("<I", len(rows) + 1)) is None
    block = ib.seal(contents)
    assert block[:-5] == contents and block[-5] == 0
    assert struct.unpack("<I", block[-4:])[0] == dlsm_amd.crc32c_mask(dlsm_amd.crc32c(contents + b"\0"))
    keys = [(r[0], M - ((r[1] << 8) | r[2])) for r in rows]
    for v in range(-1, 302):
        uk = b"%020d" % max(v, 0) if v >= 0 else b""
        for snap in (0, 10, 25, 49, (1 << 56) - 1):
            i = bisect.bisect_left(keys, (uk, M - ((snap << 8) | 1)))
            want = (0, 0, 0, 0)
            if i < len(keys):
                t = (M - keys[i][1]) & 0xFF
                if t > 1 or keys[i][0] == uk:
                    want = (3 if t > 1 else (1 if t == 1 else 2), int(offs[i]), int(sizes[i]), 4)
            assert dlsm_amd.index_block_seek(contents, uk, snap, 4) == want, (uk, snap)


def test_abi_argument_checks_without_a_device():
    import ctypes as C

    import dlsm_amd
    from dlsm_amd import _lib as L

    lib = dlsm_amd.lib()
    h = C.c_void_p(1)
    assert lib.dlsm_tableindex_create_blocks(None, None, None, 1, 0, 1, None, C.byref(h)) == L.DLSM_E_ARG
    assert h.value is None
    assert lib.dlsm_tableindex_create_blocks(None, None, None, 0, 0, 1, None, None) == L.DLSM_E_ARG
    assert lib.dlsm_tableindex_destroy(None) == L.DLSM_OK
    assert lib.dlsm_tableindex_size(None, None, None, None) == L.DLSM_E_ARG
    assert lib.dlsm_index_seek_dev(None, None, None, 0, None, None, 0, None, None, None, None) == L.DLSM_E_ARG
    assert lib.dlsm_index_seek(None, None, None, 0, None, None, 0, None, None, None, None) == L.DLSM_E_ARG
    assert lib.dlsm_index_block_check(None, 4, None) == L.DLSM_E_ARG
    assert dlsm_amd.BLOCK_INDEX == 5 and dlsm_amd.KV_HANDLE.itemsize == 16
    assert dlsm_amd.index_fence_interval() >= 2 and dlsm_amd.index_seek_block() % 64 == 0
