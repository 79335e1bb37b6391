"""dlsm_memtable_sort, the host form of the memtable sort, against
dlsm_amd/compaction.py's pure Python order over the batches of
memtable_sort_cases.py, and the sort's host planning through
tests/cpp/memtable_sort_plan_test.cc.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from compaction_merge_cases import expected, packed
from memtable_sort_cases import CASES, SHORT, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "memtable_sort_plan_test.cc")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]


def host(pairs, policy=0, snapshot=0, **caps):
    kb, ko, kl = packed([p[0] for p in pairs])
    vb, vo, vl = packed([p[1] for p in pairs])
    return dlsm_amd.memtable_sort((Keys(kb, len(pairs), kl, ko), vb, vo, vl), policy, snapshot, **caps)


@pytest.mark.parametrize("name", list(CASES))
def test_host_form_matches_the_python_order(name):
    case, want = CASES[name], expected(CASES[name])
    caps = dict(zip(("keys_cap", "values_cap", "pair_cap"), want["caps"]))
    got = host(case["runs"][0], case.get("policy", 0), case.get("snapshot", 0), **caps)
    assert list(got[5]) == want["merged"]
    for g, w in zip(got[:5], ("keys", "key_off", "values", "value_off", "src")):
        assert np.array_equal(g, want[w]), w


def test_host_form_short_key_and_arguments():
    got = host(SHORT, 1, 100)
    assert got[5] == (len(SHORT), 0, 0, 0, dlsm_amd.MERGE_SHORT_KEY)
    with pytest.raises(dlsm_amd.DlsmError):
        host(SHORT[:3], policy=2)


def test_plan_program(tmp_path):
    exe = tmp_path / "memtable_sort_plan_test"
    subprocess.run(["g++", "-O2"] + FLAGS + [SRC, "-o", str(exe)], check=True)
    sizes = [0, 1, 3, 4, 5, T - 1, T, T + 1, 2 * T + 5, 3 * T + 7, 5 * T + 1, 8 * T]
    out = subprocess.run([str(exe)] + [str(n) for n in sizes], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK %d sizes" % len(sizes)), out.stdout[-4000:] + out.stderr[-4000:]
