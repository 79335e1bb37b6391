"""The compaction output (dlsm_compaction_output) on the CPU.

tests/cpp/compaction_output_test.cc drives the rules the kernels run
(dlsm_amd/csrc/compaction_output.h) against the reference's pair-by-pair loop
and a plain writer, built twice as a stand-alone program: plain and under
AddressSanitizer + UBSan.  The host form of the ABI call is compared with a
Python walk of the cut rule and the host table build of every file's pairs.  No
GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from compaction_output_cases import CASES, expected, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "compaction_output_test.cc")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(exe, env=None):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout[-4000:] + out.stderr[-4000:]
    return out


def test_rules_program(tmp_path):
    exe = tmp_path / "compaction_output_test"
    subprocess.run(["g++", "-O2"] + FLAGS + [SRC, "-o", str(exe)], check=True)
    _run(exe)


def test_rules_program_under_asan_ubsan(tmp_path):
    exe = tmp_path / "compaction_output_test_san"
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("clang++")
    assert cxx, "clang++ (ROCm LLVM) is needed for the sanitizer build"
    subprocess.run([cxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS +
                   [SRC, "-o", str(exe)], check=True)
    out = _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


def host(name, pair_cap_extra=0, **kw):
    """The host form over a case's run, the inputs pair_cap_extra pairs longer than n_out says."""
    _, _, _, mfb, cb = CASES[name]
    iks, vals, *_ = expected(name)
    n = len(iks)
    extra = [iks[-1]] * pair_cap_extra if n else []
    kb, ko, kl = pack(iks + extra)
    vb, vo, vl = pack(vals + [vals[-1] for _ in extra])
    merged = np.array([n + 7, n, 0, 0, 0], dtype=np.uint64)
    return dlsm_amd.compaction_output(Keys(kb, n + len(extra), kl, ko), vb, merged, value_off=vo, value_len=vl,
                                      max_file_bytes=mfb, chunk_bytes=cb, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_host_form_matches_the_walk_and_the_table_build(name):
    _, _, want, recs, built = expected(name)
    tables, files, b = host(name, pair_cap_extra=3)
    assert b == built
    assert files.tolist() == recs
    assert [(d.tobytes(), e.tolist(), x.tobytes()) for d, e, x in tables] == want


def test_host_form_caps_and_flagged_input():
    _, _, want, recs, built = expected("varint-chunks")
    for i, cap in enumerate(("data_cap", "index_cap", "chunk_cap", "file_cap")):
        tables, files, b = host("varint-chunks", **{cap: built[(1, 2, 3, 0)[i]] - 1})
        assert b == built[:4] + (built[4] | (1, 2, 4, dlsm_amd.OUTPUT_FILE_CAP)[i],)
        last = len(recs) - 1
        assert files.tolist() == recs[:len(files)] and len(files) == last + (cap != "file_cap")
        for f, ((d, e, x), w) in enumerate(zip(tables, want)):
            cut = f == last and cap in ("data_cap", "index_cap")
            assert d.tobytes() == (w[0][:len(d)] if cut else w[0]) and e.tolist() == w[1][:len(e)]
            assert x.tobytes()[:len(x) - 5 * cut] == (w[2][:len(x) - 5] if cut else w[2])
    iks, vals, *_ = expected("exact")
    kb, ko, kl = pack(iks)
    vb, vo, vl = pack(vals)
    for merged in ([25, 25, 0, 0, 4], [30, 26, 0, 0, 0]):  # a flagged merge; n_out past pair_cap
        _, files, b = dlsm_amd.compaction_output(Keys(kb, 25, kl, ko), vb, merged, value_len=vl, max_file_bytes=640)
        assert b[4] == dlsm_amd.OUTPUT_INPUT_FLAGGED and len(files) == 0
    with pytest.raises(dlsm_amd.DlsmError) as e:
        dlsm_amd.compaction_output(Keys(kb, 25, kl, ko), vb, [25, 25, 0, 0, 0], value_len=vl,
                                   file_cap=dlsm_amd.OUTPUT_MAX_FILES + 1)
    assert e.value.status == -1  # DLSM_E_ARG
