"""dlsm_memtable_sort_dev: one batch in arrival order on the device into a
sorted run in the table build's input form, against dlsm_amd/compaction.py -- a
pure Python sort that never calls the code under test.  Every comparison is
``array_equal``; every output carries sentinels: 64 bytes behind each total and
each cap, 8 entries behind the offsets, ``src`` and ``merged``."""
import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from dlsm_amd import compaction as cp
from compaction_merge_cases import expected, packed
from memtable_sort_cases import CASES, SHORT, T, fixed

pytestmark = pytest.mark.gpu

SENT, END_SENT = 0xCD, 0x5A5A5A5A5A5A5A5A


def dev(a):
    import torch

    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).cuda()


def sort(gpu, pairs, policy, snapshot, caps, room):
    """Runs the sort on sentinel-filled outputs of `room` (keys, values, pairs);
    returns them as numpy arrays: keys, key_off, values, value_off, src, merged."""
    import torch

    kb, ko, kl = packed([p[0] for p in pairs])
    vb, vo, vl = packed([p[1] for p in pairs])
    batch = (Keys(dev(kb), len(pairs), kl, dev(ko)), dev(vb), dev(vo), vl)
    keys = torch.full((max(room[0], caps[0]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    values = torch.full((max(room[1], caps[1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    ko, vo, src = (dev(np.full(max(room[2], caps[2]) + 9, END_SENT, dtype=np.uint64)) for _ in range(3))
    merged = dev(np.full(5 + 8, END_SENT, dtype=np.uint64))
    gpu.memtable_sort_dev(batch, keys, ko, values, vo, merged, src=src, policy=policy, smallest_snapshot=snapshot,
                          keys_cap=caps[0], values_cap=caps[1], pair_cap=caps[2])
    gpu.sync()
    return [x.cpu().numpy() if x.dtype == torch.uint8 else x.cpu().numpy().view(np.uint64)
            for x in (keys, ko, values, vo, src, merged)]


def run_case(gpu, case):
    want = expected(case)
    got = sort(gpu, case["runs"][0], case.get("policy", 0), case.get("snapshot", 0), want["caps"],
               want["merged"][2:4] + [want["merged"][1]])
    assert got[5][:5].tolist() == want["merged"] and (got[5][5:] == END_SENT).all()
    for g, w in zip(got[:5], ("keys", "key_off", "values", "value_off", "src")):
        m = len(want[w])
        assert np.array_equal(g[:m], want[w]), w
        assert (g[m:] == (SENT if g.dtype == np.uint8 else END_SENT)).all(), w  # nothing at or past a cap or a total
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_sort_against_the_python_order(gpu, name):
    run_case(gpu, CASES[name])


def test_short_key_writes_only_merged(gpu):
    got = sort(gpu, SHORT, 1, 100, [1 << 16, 1 << 16, len(SHORT)], [0, 0, 0])
    assert (got[5][0], got[5][4]) == (len(SHORT), dlsm_amd.MERGE_SHORT_KEY) and (got[5][5:] == END_SENT).all()
    for g in got[:5]:
        assert (g == (SENT if g.dtype == np.uint8 else END_SENT)).all()


def test_sorted_batch_builds_the_table_of_the_sorted_pairs(gpu):
    """sort(flush rule) -> table build on one stream: the region and the sealed
    index block of the host table_build over the Python-sorted pairs."""
    import torch

    case = dict(runs=[fixed(T + 1)], policy=1, snapshot=cp.MAX_SEQUENCE)
    keys, ko, values, vo, _, merged = run_case(gpu, case)
    pairs, _ = cp.merge_runs(case["runs"], 1, cp.MAX_SEQUENCE)
    n, kb, vb = (int(x) for x in merged[1:4])
    vbytes, voff, vlen = packed([p[1] for p in pairs])
    want = dlsm_amd.table_build(Keys.pack([p[0] for p in pairs]), vbytes, value_off=voff, value_len=vlen)
    d_cap, i_cap = dlsm_amd.table_build_bound(n, kb, vb)
    data, index = (torch.zeros(c + 16, dtype=torch.uint8, device="cuda") for c in (d_cap, i_cap))
    ce, built = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    gpu.table_build_dev(Keys(dev(keys[:kb]), n, 0, dev(ko[:n + 1])), dev(values[:max(vb, 1)]), data, index, ce, built,
                        value_off=dev(vo[:n + 1]))
    gpu.sync()
    b = built.cpu().numpy()
    assert tuple(int(x) for x in b) == want[3]
    assert np.array_equal(data.cpu().numpy()[:b[0]], want[0]) and np.array_equal(index.cpu().numpy()[:b[1]], want[1])
