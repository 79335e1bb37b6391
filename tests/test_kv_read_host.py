"""The value read (dlsm_tabledata, dlsm_kv_read_dev) on the CPU.

tests/cpp/kv_read_test.cc: the chunk lookup and the pair decision the kernels run
(dlsm_amd/csrc/kv_read.h) against a linear scan, one pair per rejection reason,
the copy's unit driven span by span against a concatenation, and the planner
against brute force -- built twice as a stand-alone program, plain and under
AddressSanitizer + UBSan.  tests/cpp/adapter_kv_test.cc: the adapter's
TableData on the all-host path.  No GPU needed.  TableBuilder_BACS needs the
RDMA headers and cannot be compiled here, so the writers in these tests (C++ and
dlsm_amd/data_region.py) restate table/table_builder_bacs.cpp:221-226 by hand."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kv_read_test.cc")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
NOTFOUND, FOUND, DELETED, CORRUPT = 0, 1, 2, 3


def _run(exe, env=None):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout[-4000:] + out.stderr[-4000:]
    return out


def test_kv_read_host(tmp_path):
    exe = tmp_path / "kv_read_test"
    subprocess.run(["g++", "-O2"] + FLAGS + [SRC, "-o", str(exe)], check=True)
    _run(exe)


def test_kv_read_host_under_asan_ubsan(tmp_path):
    exe = tmp_path / "kv_read_test_san"
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("clang++")
    assert cxx, "clang++ (ROCm LLVM) is needed for the sanitizer build"
    subprocess.run([cxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                   [SRC, "-o", str(exe)], check=True)
    out = _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


def test_kv_kernels_use_no_scratch(tmp_path):
    """The size, offset and copy kernels hold no per-lane arrays: no spill.
    Compiled for gfx950 on the CPU, read from the compiler's resource-usage
    remarks."""
    src = os.path.join(ROOT, "dlsm_amd", "csrc", "kv_read.hip")
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
    kv = {k: v for k, v in usage.items() if "kv_" in k}
    assert len(kv) == 3, sorted(usage)  # size, offsets (with the scan of the partial sums), copy
    assert all(v == 0 for v in kv.values()), kv


def compile_adapter_kv_test(tmp_path):
    exe = tmp_path / "adapter_kv_test"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fno-rtti", "-fno-exceptions", "-pthread",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "adapter_kv_test.cc"),
                    "-L", os.path.join(ROOT, "dlsm_amd", "lib"), "-ldlsm_bloom",
                    "-Wl,-rpath," + os.path.join(ROOT, "dlsm_amd", "lib"),
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", str(exe)], check=True)
    return exe


def test_adapter_table_data_on_cpu(tmp_path):
    exe = compile_adapter_kv_test(tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK adapter kv host" in out.stdout, out.stdout + out.stderr


def model(chunks, handle, user_key):
    """The rules of include/dlsm_bloom.h for one FOUND Get, over the bytes."""
    off, size = handle
    ends = np.cumsum([len(c) for c in chunks]).tolist()
    c = next((j for j, e in enumerate(ends) if e > off), None)
    if size < 16 or c is None or off + size > ends[c]:
        return CORRUPT, None
    at = off - (ends[c - 1] if c else 0)
    p = chunks[c][at:at + size]
    ks, vs = struct.unpack_from("<II", p)
    if ks < 8 or 8 + ks + vs != size or p[ks] > 1 or p[8:ks] != user_key:
        return CORRUPT, None
    return (FOUND, p[8 + ks:]) if p[ks] == 1 else (DELETED, None)


def test_python_writers_and_host_pair_read_against_the_model():
    """dlsm_amd/data_region.py's two writers agree byte for byte, and
    dlsm_kv_pair_read answers like the model for every pair, for handles off
    by one in each field, and for the wrong key."""
    import dlsm_amd
    from dlsm_amd import data_region as dr
    from dlsm_amd import index_block as ib

    rng = np.random.default_rng(21)
    n, klen, vlen = 300, 28, 13
    uks = [b"%020d" % (7 * j) for j in range(n)]
    iks = [ib.internal_key(k, 100 + j, 0 if j % 11 == 3 else 1) for j, k in enumerate(uks)]
    vals = rng.integers(0, 256, (n, vlen), dtype=np.uint8)
    pairs = [(k, v.tobytes()) for k, v in zip(iks, vals)]
    chunks, handles = dr.build_region(pairs)
    region, offs, sizes = dr.build_region_fixed(np.frombuffer(b"".join(iks), dtype=np.uint8).reshape(n, klen), vals)
    assert len(chunks) == 1 and region.tobytes() == chunks[0]
    assert offs.tolist() == [h[0] for h in handles] and sizes.tolist() == [h[1] for h in handles]
    assert dr.pair_bytes(iks[0], b"abc") == struct.pack("<II", 28, 3) + iks[0] + b"abc"
    # chunked: no pair straddles, the offsets run on, the bytes are the same
    cut, handles2 = dr.build_region(pairs, chunk_bytes=500)
    assert len(cut) > 10 and handles2 == handles and b"".join(cut) == chunks[0]
    assert all(len(c) <= 500 and len(c) % (8 + klen + vlen) == 0 for c in cut)
    big, hb = dr.build_region([(iks[0], b"x" * 900), (iks[1], b"y")], chunk_bytes=500)  # a pair larger than a chunk
    assert [len(c) for c in big] == [936, 37] and hb == [(0, 936), (936, 37)]
    # variable lengths, several chunks
    lens = rng.integers(0, 200, n)
    vpairs = [(ib.internal_key(k[:1 + j % 20], 5, j % 2), rng.integers(0, 256, int(l), dtype=np.uint8).tobytes())
              for j, (k, l) in enumerate(zip(uks, lens))]
    vchunks, vh = dr.build_region(vpairs, chunk_bytes=700)
    seen = set()
    for lay, hs, ps in ((chunks, handles, pairs), (cut, handles2, pairs), (vchunks, vh, vpairs)):
        for (off, size), (ik, v) in zip(hs, ps):
            uk = ik[:-8]
            want = (FOUND, v) if ik[-8] == 1 else (DELETED, None)
            assert model(lay, (off, size), uk) == want
            assert dlsm_amd.kv_pair_read(lay, (off, size), uk) == want
            for h, k in (((off + 1, size), uk), ((off, size + 1), uk), ((off, size - 1), uk), ((off, 15), uk),
                         ((off + size, size), uk), ((off, size), uk + b"\0"), ((off, size), uk[:-1] if uk else b"q")):
                got = dlsm_amd.kv_pair_read(lay, h, k)
                assert got == model(lay, h, k), (h, k)
                seen.add(got[0])
            for s in (NOTFOUND, DELETED, CORRUPT):  # other incoming states pass through, the handle unread
                assert dlsm_amd.kv_pair_read(lay, (1 << 60, 0xFFFFFFFF), uk, state=s) == (s, None)
    assert seen == {CORRUPT}  # every handle or key that is off by one is rejected
    assert dlsm_amd.kv_pair_read([], (0, 16), b"") == (CORRUPT, None)


def test_abi_argument_checks_without_a_device():
    import ctypes as C

    import dlsm_amd
    from dlsm_amd import _lib as L

    lib = dlsm_amd.lib()
    h = C.c_void_p(1)
    begin = (C.c_uint32 * 2)(0, 0)
    assert lib.dlsm_tabledata_create(None, None, begin, 1, 0, C.byref(h)) == L.DLSM_E_ARG
    assert h.value is None
    assert lib.dlsm_tabledata_create(None, None, begin, 1, 0, None) == L.DLSM_E_ARG
    assert lib.dlsm_tabledata_destroy(None) == L.DLSM_OK
    assert lib.dlsm_tabledata_size(None, None, None, None) == L.DLSM_E_ARG
    assert lib.dlsm_kv_read_dev(None, None, None, None, None, 0, None, None, None, None, 0, None) == L.DLSM_E_ARG
    assert lib.dlsm_kv_read(None, None, None, None, None, 0, None, None, None, None, 0, None) == L.DLSM_E_ARG
    st = C.c_uint8(FOUND)
    assert lib.dlsm_kv_pair_read(None, 0, None, None, 0, C.byref(st), None, None) == L.DLSM_E_ARG
    assert dlsm_amd.kv_read_chunk() % 64 == 0 and dlsm_amd.kv_read_span() % 16 == 0
    ms, wgs = (C.c_double * 3)(), C.c_uint32(9)
    assert lib.dlsm_kv_read_stats(None, ms, C.byref(wgs)) == L.DLSM_E_ARG
    assert lib.dlsm_abi_version() == 1
