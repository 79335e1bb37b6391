"""The compaction filters (dlsm_compaction_filters) on the CPU: the host form of
the ABI call against the oracle's full filter over every file's user keys, and
the host planning (dlsm::plan in host_plan.h) against brute force in
tests/cpp/compaction_filters_plan_test.cc, over the cuts of the case table.  No
GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from compaction_filters_cases import CASES, expected, file_records, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "compaction_filters_plan_test.cc")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]


def host(name, pair_cap_extra=3, merged=None, **kw):
    """The host form over a case's cut run, the keys pair_cap_extra pairs longer than n_out says."""
    iks, sizes, bpk = CASES[name]
    n = len(iks)
    kb, ko, kl = pack(iks + [iks[-1]] * pair_cap_extra)
    files, out_built = file_records(sizes)
    return dlsm_amd.compaction_filters(Keys(kb, n + pair_cap_extra, kl, ko), merged or [n + 7, n, 0, 0, 0], files, out_built,
                                       bits_per_key=bpk, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_host_form_matches_the_oracle(name):
    want, recs, built = expected(name)
    blocks, got_recs, b = host(name)
    assert b == built and got_recs.tolist() == recs
    assert [x.tobytes() for x in blocks] == want


def test_host_form_caps_flagged_input_and_arguments():
    want, recs, built = expected("straddle")
    blocks, got_recs, b = host("straddle", filters_cap=built[1] // 2)
    assert b == (built[0], built[1], dlsm_amd.FILTERS_CAP) and got_recs.tolist() == recs
    assert [None if x is None else x.tobytes() for x in blocks] == [w if r[0] + r[1] <= built[1] // 2 else None
                                                                    for w, r in zip(want, recs)]
    iks, sizes, _ = CASES["straddle"]
    kb, ko, kl = pack(iks)
    files, out_built = file_records(sizes)
    keys = Keys(kb, len(iks), kl, ko)
    for merged, fl, ob in (([150, 150, 0, 0, 4], files, out_built), ([160, 151, 0, 0, 0], files, out_built),
                           ([150, 150, 0, 0, 0], files, [38, 0, 0, 0, dlsm_amd.OUTPUT_FILE_CAP]),
                           ([150, 150, 0, 0, 0], files[:-1], out_built)):  # the records stop before n_files
        blocks, got_recs, b = dlsm_amd.compaction_filters(keys, merged, fl, ob)
        assert b == (0, 0, dlsm_amd.FILTERS_INPUT_FLAGGED) and len(blocks) == 0
    for bpk, fl in ((0, files), (513, files), (10, np.zeros((dlsm_amd.OUTPUT_MAX_FILES + 1, 9), dtype=np.uint64))):
        with pytest.raises(dlsm_amd.DlsmError) as e:
            dlsm_amd.compaction_filters(keys, [150, 150, 0, 0, 0], fl, out_built, bits_per_key=bpk)
        assert e.value.status == -1  # DLSM_E_ARG


def test_plan_program(tmp_path):
    exe, cuts = tmp_path / "compaction_filters_plan_test", tmp_path / "cuts.txt"
    cuts.write_text("".join("%d %d %s\n" % (bpk, len(sizes), " ".join(map(str, sizes))) for _, sizes, bpk in CASES.values()))
    subprocess.run(["g++", "-O2"] + FLAGS + [SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(cuts)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK %d cuts" % len(CASES)), out.stdout[-4000:] + out.stderr[-4000:]
