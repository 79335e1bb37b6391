"""The table build (dlsm_table_build) on the CPU.

tests/cpp/table_build_test.cc drives the rules the kernels run
(dlsm_amd/csrc/table_build.h) against a plain writer, built twice as a
stand-alone program: plain and under AddressSanitizer + UBSan.  The host form of
the ABI call is compared with dlsm_amd/data_region.py and
dlsm_amd/index_block.py, which never call it.  No GPU needed."""
import ctypes as C_
import os
import shutil
import subprocess

import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from dlsm_amd import data_region as dr
from dlsm_amd import index_block as ib
from table_build_cases import KEYS, VALUES, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "table_build_test.cc")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
C, Sp = dlsm_amd.table_build_chunk(), dlsm_amd.table_build_span()


def _run(exe, env=None):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout[-4000:] + out.stderr[-4000:]
    return out


def test_rules_program(tmp_path):
    exe = tmp_path / "table_build_test"
    subprocess.run(["g++", "-O2"] + FLAGS + [SRC, "-o", str(exe)], check=True)
    _run(exe)


def test_rules_program_under_asan_ubsan(tmp_path):
    exe = tmp_path / "table_build_test_san"
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("clang++")
    assert cxx, "clang++ (ROCm LLVM) is needed for the sanitizer build"
    subprocess.run([cxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                   [SRC, "-o", str(exe)], check=True)
    out = _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


VAR, MIX = KEYS["var"], VALUES["mix"]
CASES = {f"n{n}": (n, VAR, MIX, {}) for n in (0, 1, 2, C - 1, C, C + 1, 2 * C + 3)}
CASES.update({f"v{v}": (C + 1, lambda j: 28, lambda j, v=v: v, {"fixed": True}) for v in (0, 1, 15, 16, 17, 400)})
CASES.update({"k8": (C + 1, lambda j: 8, lambda j: 1, {"fixed": True}), "past-2^21": (6 * C, lambda j: 28, lambda j: 400, {}),
              "chunk-exact": (300, VAR, MIX, {"first": 40, "less": 0}), "chunk-minus1": (300, VAR, MIX, {"first": 40, "less": 1}),
              "chunk-oversize": (300, VAR, MIX, {"chunk_bytes": 15}), "cap-data": (300, VAR, MIX, {"data_cap": 1003}),
              "cap-index": (300, VAR, MIX, {"index_cap": 8192 + 7}), "cap-trailer": (300, VAR, MIX, {"index_cap": -2}),
              "cap-chunk": (300, VAR, MIX, {"chunk_bytes": 1000, "chunk_cap": 5}),
              "cap-0": (300, VAR, MIX, {"data_cap": 0, "index_cap": 0, "chunk_cap": 0})})


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_host_form_against_the_python_writers(case):
    n, klen, vlen, kw = CASES[case]
    kw = dict(kw)
    iks, vals = make(n, klen, vlen)
    first = None
    if "first" in kw:  # the exact sum of the first pairs must not cut; a byte less must
        sums = np.cumsum([8 + len(k) + len(v) for k, v in zip(iks, vals)])
        first = int(sums[kw["first"] - 1 - kw["less"]])
        kw["chunk_bytes"] = int(sums[kw.pop("first") - 1]) - kw.pop("less")
    chunks, handles = dr.build_region(list(zip(iks, vals)), kw.get("chunk_bytes") or None)
    region, block = b"".join(chunks), ib.build_index_block(iks, handles)
    ends = np.cumsum([len(c) for c in chunks]).tolist()
    assert first is None or ends[0] == first
    if kw.get("index_cap") == -2:
        kw["index_cap"] = len(block) - 2
    vb = np.frombuffer(b"".join(vals) + b"\0" * 16, dtype=np.uint8)
    if kw.pop("fixed", False):
        keys = Keys(np.frombuffer(b"".join(iks) + b"\0" * 16, dtype=np.uint8), n, len(iks[0]))
        data, index, ce, built = dlsm_amd.table_build(keys, vb, value_len=len(vals[0]), **kw)
    else:
        vo = np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(np.uint64)
        data, index, ce, built = dlsm_amd.table_build(Keys.pack(iks), vb, value_off=vo, **kw)
    caps = [kw.get("data_cap", len(region)), kw.get("index_cap", len(block)), kw.get("chunk_cap", len(ends))]
    over = [len(region) > caps[0], len(block) > caps[1], len(ends) > caps[2]]
    oversize = any(s > kw.get("chunk_bytes", 1 << 62) for _, s in handles) and bool(kw.get("chunk_bytes"))
    assert built == (len(region), len(block), len(ends), over[0] + 2 * over[1] + 4 * over[2] + 64 * oversize)
    assert data.tobytes() == region[:caps[0]] and ce.tolist() == ends[:caps[2]]
    want = block[:caps[1]]
    if over[1]:  # no trailer unless the whole block fits: the bytes there stay as they were (zero)
        want = want[:len(block) - 5] + b"\0" * max(0, len(want) - (len(block) - 5))
    assert index.tobytes() == want
    if not over[1]:
        assert dlsm_amd.index_block_check(block[:-5]) == n and dlsm_amd.index_block_check(index.tobytes()[:-5]) == n


def test_abi_argument_checks_without_a_device():
    from dlsm_amd import _lib as L

    lib = dlsm_amd.lib()
    ti, to, b = L.dlsm_table_input(), L.dlsm_table_output(), (C_.c_uint64 * 4)()
    for f in (lib.dlsm_table_build, lib.dlsm_table_build_dev):
        assert f(None, None, None) == L.DLSM_E_ARG and f(None, C_.byref(ti), C_.byref(to)) == L.DLSM_E_ARG  # no `built`
    to.built = C_.addressof(b)
    assert lib.dlsm_table_build_dev(None, C_.byref(ti), C_.byref(to)) == L.DLSM_E_ARG  # the device form needs a context
    ti.keys.n = 1 << 32
    assert lib.dlsm_table_build(None, C_.byref(ti), C_.byref(to)) == L.DLSM_E_ARG
    ti.keys.n = 0
    assert lib.dlsm_table_build(None, C_.byref(ti), C_.byref(to)) == L.DLSM_OK and list(b) == [0, 9, 1, 2 | 4]
    assert dlsm_amd.table_build_bound(3, 84, 300) == (408, 186) and C % 64 == 0 and Sp % 16 == 0
    assert lib.dlsm_table_build_stats(None, None, None) == L.DLSM_E_ARG and lib.dlsm_abi_version() == 1
