"""dlsm_compaction_merge_dev: sorted runs on the device into one run in the
table build's input form, against dlsm_amd/compaction.py -- a pure Python merge
that never calls the code under test.  Every comparison is ``array_equal``;
every output carries sentinels: 64 bytes behind each total and each cap, 8
entries behind the offsets, ``src`` and ``merged``."""
import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from compaction_merge_cases import BAD, CASES, T, expected, ik, listed, packed

pytestmark = pytest.mark.gpu

SENT, END_SENT = 0xCD, 0x5A5A5A5A5A5A5A5A
FOUND, DELETED = 1, 2


def dev(a):
    import torch

    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).cuda()


def merge(gpu, runs, policy, snapshot, caps, room):
    """Runs the merge on sentinel-filled outputs of `room` (keys, values, pairs);
    returns them as numpy arrays: keys, key_off, values, value_off, src, merged."""
    import torch

    drs = []
    for run in runs:
        kb, ko, kl = packed([p[0] for p in run])
        vb, vo, vl = packed([p[1] for p in run])
        drs.append((Keys(dev(kb), len(run), kl, dev(ko)), dev(vb), dev(vo), vl))
    keys = torch.full((max(room[0], caps[0]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    values = torch.full((max(room[1], caps[1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    ko, vo, src = (dev(np.full(max(room[2], caps[2]) + 9, END_SENT, dtype=np.uint64)) for _ in range(3))
    merged = dev(np.full(5 + 8, END_SENT, dtype=np.uint64))
    gpu.compaction_merge_dev(drs, keys, ko, values, vo, merged, src=src, policy=policy, smallest_snapshot=snapshot,
                             keys_cap=caps[0], values_cap=caps[1], pair_cap=caps[2])
    gpu.sync()
    return [x.cpu().numpy() if x.dtype == torch.uint8 else x.cpu().numpy().view(np.uint64)
            for x in (keys, ko, values, vo, src, merged)]


def run_case(gpu, case):
    want = expected(case)
    got = merge(gpu, case["runs"], case.get("policy", 0), case.get("snapshot", 0), want["caps"], want["merged"][2:4] + [want["merged"][1]])
    assert got[5][:5].tolist() == want["merged"] and (got[5][5:] == END_SENT).all()
    for g, w in zip(got[:5], ("keys", "key_off", "values", "value_off", "src")):
        m = len(want[w])
        assert np.array_equal(g[:m], want[w]), w
        assert (g[m:] == (SENT if g.dtype == np.uint8 else END_SENT)).all(), w  # nothing at or past a cap or a total
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_merge_against_the_python_merge(gpu, name):
    run_case(gpu, CASES[name])


@pytest.mark.parametrize("name", list(BAD))
def test_malformed_runs_write_only_merged(gpu, name):
    runs, spoil, flag = BAD[name]
    runs = [list(r) for r in runs]
    spoil(runs)
    n = sum(map(len, runs))
    got = merge(gpu, runs, 1, 100, [1 << 16, 1 << 16, n], [0, 0, 0])
    assert (got[5][0], got[5][4]) == (n, flag) and (got[5][5:] == END_SENT).all()
    for g in got[:5]:
        assert (g == (SENT if g.dtype == np.uint8 else END_SENT)).all()


def test_drop_equals_keep_all_filtered_by_the_select(gpu):
    """DROP_HIDDEN's pairs are KEEP_ALL's pairs under internal_keys_select_dev's
    compaction mask."""
    import torch

    case = dict(CASES["R5-1"], policy=0)
    keys, ko, _, _, src, merged = run_case(gpu, case)
    n = int(merged[1])
    keep = torch.zeros(n, dtype=torch.uint8, device="cuda")
    gpu.internal_keys_select_dev(Keys(dev(keys[:int(merged[2])]), n, 0, dev(ko[:n + 1])), dlsm_amd.SELECT_COMPACTION, 103, keep)
    gpu.sync()
    dropped = run_case(gpu, dict(case, policy=1, snapshot=103))
    assert np.array_equal(src[:n][keep.cpu().numpy() != 0], dropped[4][:int(dropped[5][1])])


def test_merged_runs_build_a_table_that_answers_gets(gpu):
    """Three overlapping runs -> merge(DROP_HIDDEN) -> table build -> open (which
    validates strict order) -> index seek + value read of every user key: the
    newest run's value, or DELETED."""
    import torch

    users = [b"user%05d" % j + b"x" * (j % 23) for j in range(T + 40)]
    runs = listed(*[[(u, 10 + r, (j + r) % 5 != 0) for j, u in enumerate(users) if j % (r + 2) != 1] for r in range(3)])
    newest = {}
    for run in runs:  # a later run holds the higher sequence
        newest.update({k[:-8]: ((FOUND, v) if k[-8] == 1 else (DELETED, b"")) for k, v in run})
    keys, ko, values, vo, _, merged = run_case(gpu, dict(runs=runs, policy=1, snapshot=1 << 40))
    n, kb, vb = (int(x) for x in merged[1:4])
    assert n == len(newest)
    d_cap, i_cap = dlsm_amd.table_build_bound(n, kb, vb)
    data, index = (torch.zeros(c + 16, dtype=torch.uint8, device="cuda") for c in (d_cap, i_cap))
    ce, built = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    gpu.table_build_dev(Keys(dev(keys[:kb]), n, 0, dev(ko[:n + 1])), dev(values[:max(vb, 1)]), data, index, ce, built,
                        value_off=dev(vo[:n + 1]))
    gpu.sync()
    b = built.cpu().numpy()
    assert b[3] == 0
    ti = gpu.tableindex([index[:b[1]]], on_device=True)
    td = gpu.tabledata([[data[:b[0]]]], on_device=True)
    k = Keys.pack(list(newest))
    m = len(newest)
    gk = Keys(dev(k.data), m, 0, dev(k.offsets))
    st = torch.zeros(m, dtype=torch.uint8, device="cuda")
    hd = torch.zeros((m, 16), dtype=torch.uint8, device="cuda")
    gd = torch.arange(m, dtype=torch.int32, device="cuda")
    gpu.index_seek_dev(ti, gk, (1 << 56) - 1, dev(np.array([0, m], dtype=np.uint64)), gd, task_state=st, task_handle=hd)
    out_off = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    out = torch.zeros(sum(len(w[1]) for w in newest.values()) + 16, dtype=torch.uint8, device="cuda")
    gpu.kv_read_dev(td, gk, st, hd, out_off, out, gets=gd)
    gpu.sync()
    assert st.cpu().numpy().tolist() == [w[0] for w in newest.values()]
    assert out.cpu().numpy()[:-16].tobytes() == b"".join(w[1] for w in newest.values())
    ti.close()
    td.close()


def test_fault_injection_reaches_both_forms(gpu):
    case = CASES["type-2-restarts"]
    gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 4)
    try:
        host = lambda: gpu.compaction_merge([(Keys.pack([ik(b"k", 1)]), np.zeros(1, dtype=np.uint8), None, 0)])  # noqa: E731
        for call in (lambda: run_case(gpu, case), host):
            with pytest.raises(dlsm_amd.DlsmError) as e:
                call()
            assert e.value.status == -4
    finally:
        gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 0)
    run_case(gpu, case)
