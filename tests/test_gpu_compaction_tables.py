"""dlsm_compaction_merge_tables_dev: a compaction's inputs read straight out of
opened tables on the device, against compaction.merge_runs over
compaction.table_pairs -- pure Python that walks each table the way the
reference iterator does.  Every comparison is ``array_equal``; every output
carries sentinels: 64 bytes behind each total and each cap, 8 entries behind the
offsets, ``src`` and ``merged``."""
import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from dlsm_amd.index_block import build_index_block
from compaction_tables_cases import BAD, CASES, host_args, total, two_files, want

pytestmark = pytest.mark.gpu

SENT, END_SENT = 0xCD, 0x5A5A5A5A5A5A5A5A


def opened(gpu, c):
    blocks, files, runs = host_args(c)
    return gpu.tableindex(blocks), gpu.tabledata(files), runs


def merge(gpu, ti, td, runs, policy, snapshot, caps, room):
    """The merge on sentinel-filled outputs of `room` (keys, values, pairs), as
    numpy arrays: keys, key_off, values, value_off, src, merged."""
    import torch

    keys, values = (torch.full((max(r, c) + 64,), SENT, dtype=torch.uint8, device="cuda") for r, c in zip(room[:2], caps))
    ko, vo, src = (torch.from_numpy(np.full(max(room[2], caps[2]) + 9, END_SENT, dtype=np.uint64).view(np.int64)).cuda()
                   for _ in range(3))
    merged = torch.from_numpy(np.full(5 + 8, END_SENT, dtype=np.uint64).view(np.int64)).cuda()
    gpu.compaction_merge_tables_dev(ti, td, runs, keys, ko, values, vo, merged, src=src, policy=policy,
                                    smallest_snapshot=snapshot, keys_cap=caps[0], values_cap=caps[1], pair_cap=caps[2])
    gpu.sync()
    return [x.cpu().numpy() if x.dtype == torch.uint8 else x.cpu().numpy().view(np.uint64)
            for x in (keys, ko, values, vo, src, merged)]


def check(got, w):
    assert got[5][:5].tolist() == w["merged"] and (got[5][5:] == END_SENT).all()
    for g, k in zip(got[:5], ("keys", "key_off", "values", "value_off", "src")):
        m = len(w[k])
        assert np.array_equal(g[:m], w[k]), k
        assert (g[m:] == (SENT if g.dtype == np.uint8 else END_SENT)).all(), k  # nothing at or past a cap or a total


def run_case(gpu, c):
    w = want(c)
    ti, td, runs = opened(gpu, c)
    got = merge(gpu, ti, td, runs, c.get("policy", 0), c.get("snapshot", 0), w["caps"], w["merged"][2:4] + [w["merged"][1]])
    ti.close()
    td.close()
    check(got, w)
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_tables_merge_against_the_python_walk_and_merge(gpu, name):
    run_case(gpu, CASES[name])


@pytest.mark.parametrize("name", list(BAD))
def test_malformed_tables_write_only_merged(gpu, name):
    make, flag = BAD[name]
    c = make()
    ti, td, runs = opened(gpu, c)
    got = merge(gpu, ti, td, runs, 1, 100, [1 << 12, 1 << 12, 64], [0, 0, 0])
    assert (got[5][0], got[5][4]) == (total(c), flag) and (got[5][5:] == END_SENT).all()
    for g in got[:5]:
        assert (g == (SENT if g.dtype == np.uint8 else END_SENT)).all()


def test_tables_merge_rejects_bad_arguments(gpu):
    """(More than UINT32_MAX entries is the planner's rule for both forms: the
    host form's test reaches it with a header alone.)"""
    blocks, files, _ = host_args(two_files())
    empty = build_index_block([], [])
    for runs, b, f in (([], blocks, files), ([[0]] * 65, blocks, files),  # n_runs outside 1..64
                       ([[0]], blocks, files + [None]),                   # the file counts differ
                       ([[0, 2]], blocks, files),                         # a file >= n_files
                       ([[0, 1]], [blocks[0], None], files),              # no index held
                       ([[0, 1]], blocks, [files[0], None]),              # no data held
                       ([[0] * 1024], [empty], [None])):                  # more than 1,023 files listed
        ti, td = gpu.tableindex(b), gpu.tabledata(f)
        with pytest.raises(dlsm_amd.DlsmError) as e:
            merge(gpu, ti, td, runs, 0, 0, [64, 64, 8], [0, 0, 0])
        assert e.value.status == -1, runs[:1]


def test_merged_tables_build_a_table_that_merges_to_itself(gpu):
    """tables -> merge_tables_dev(DROP_HIDDEN) -> table_build_dev -> open ->
    merge_tables_dev(KEEP_ALL) of that one table: the first call's pairs."""
    import torch

    first = run_case(gpu, CASES["file-sizes"])
    n, kb, vb = (int(x) for x in first[5][1:4])
    d_cap, i_cap = dlsm_amd.table_build_bound(n, kb, vb)
    data, index = (torch.zeros(c + 16, dtype=torch.uint8, device="cuda") for c in (d_cap, i_cap))
    ce, built = torch.zeros(64, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).cuda()  # noqa: E731
    gpu.table_build_dev(Keys(dev(first[0][:kb]), n, 0, dev(first[1][:n + 1])), dev(first[2][:max(vb, 1)]), data, index, ce,
                        built, value_off=dev(first[3][:n + 1]), chunk_bytes=1 << 16)
    gpu.sync()
    b, ends = built.cpu().numpy(), [0] + ce.cpu().numpy().tolist()
    assert b[3] == 0 and 1 < b[2] <= 64
    ti = gpu.tableindex([index[:b[1]]], on_device=True)
    td = gpu.tabledata([[data[ends[j]:ends[j + 1]] for j in range(b[2])]], on_device=True)
    again = merge(gpu, ti, td, [[0]], 0, 0, [kb, vb, n], [kb, vb, n])
    assert again[5][:5].tolist() == [n, n, kb, vb, 0]
    for g, f in zip(again[:4], first[:4]):
        assert np.array_equal(g, f)
    assert np.array_equal(again[4][:n], np.arange(n, dtype=np.uint64))


def test_fault_injection_reaches_both_forms(gpu):
    c = two_files()
    ti, td, runs = opened(gpu, c)
    gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 4)
    try:
        for call in (lambda: merge(gpu, ti, td, runs, 0, 0, [512, 512, 16], [0, 0, 0]),
                     lambda: gpu.compaction_merge_tables(*host_args(c), keys_cap=512, values_cap=512, pair_cap=16)):
            with pytest.raises(dlsm_amd.DlsmError) as e:
                call()
            assert e.value.status == -4
    finally:
        gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 0)
    run_case(gpu, c)
