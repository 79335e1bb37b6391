"""dlsm_compaction_merge, the host form: the merge passes, the drop rule and the
packing of compaction_merge.h run on the CPU, against dlsm_amd/compaction.py --
a pure Python merge that never calls the code under test."""
import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from compaction_merge_cases import BAD, CASES, expected, packed


def host_runs(runs):
    out = []
    for run in runs:
        kb, ko, kl = packed([p[0] for p in run])
        vb, vo, vl = packed([p[1] for p in run])
        out.append((Keys(kb, len(run), kl, ko), vb, vo, vl))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_host_merge_against_the_python_merge(name):
    case, want = CASES[name], expected(CASES[name])
    caps = dict(zip(("keys_cap", "values_cap", "pair_cap"), want["caps"]))
    got = dlsm_amd.compaction_merge(host_runs(case["runs"]), case.get("policy", 0), case.get("snapshot", 0), **caps)
    assert list(got[5]) == want["merged"]
    for g, w in zip(got[:5], ("keys", "key_off", "values", "value_off", "src")):
        assert np.array_equal(g, want[w]), w


@pytest.mark.parametrize("name", list(BAD))
def test_host_merge_flags_malformed_runs(name):
    runs, spoil, flag = BAD[name]
    runs = [list(r) for r in runs]
    spoil(runs)
    m = dlsm_amd.compaction_merge(host_runs(runs), 1, 100)[5]
    assert (m[0], m[4]) == (sum(map(len, runs)), flag)


def test_host_merge_rejects_bad_arguments():
    run = host_runs(CASES["type-2-restarts"]["runs"])
    with pytest.raises(ValueError):
        dlsm_amd.compaction_merge(run * 33)
    with pytest.raises(dlsm_amd.DlsmError) as e:
        dlsm_amd.compaction_merge(run, policy=2)
    assert e.value.status == -1
