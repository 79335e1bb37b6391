"""dlsm_range_scan, the host form: batched Seek + Next over sealed index blocks
and data chunks (range_scan.h's rules on the CPU), against compaction.scan_runs
over compaction.table_pairs -- pure Python that walks each table the way the
reference iterator does and then runs an explicit DBIter loop.  Every
comparison is ``array_equal``; every output carries sentinels: 64 bytes behind
each total and each cap, 8 entries behind the offsets, the counts and
``scanned``, 4 behind the handles."""
import ctypes as C

import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from dlsm_amd.index_block import build_index_block
from range_scan_cases import CASES, OUTPUTS, host_args, keys_of, mismatch, two_files, want

SENT, CNT_SENT, END_SENT = 0xCD, 0xCDCDCDCD, 0x5A5A5A5A5A5A5A5A
SENTINEL = {np.dtype(np.uint8): SENT, np.dtype(np.uint32): CNT_SENT, np.dtype(np.uint64): END_SENT}


def scan(c, caps, room=(0, 0, 0), ctx=None):
    """dlsm_range_scan of c on sentinel-filled arrays of `room` (keys, values,
    pairs) or the caps, whichever is larger, by output name."""
    blocks, files, runs = host_args(c)
    n, pa, la, ca, begin, _held = dlsm_amd._host_tables(blocks, files, "range_scan")
    tr, _keep = dlsm_amd._table_runs(runs)
    data, off = keys_of(c["starts"])
    q, limit = len(c["starts"]), c["limit"]
    pairs = max(room[2], caps[2])
    o = dict(count=np.full(q + 8, CNT_SENT, dtype=np.uint32), pair_begin=np.full(q + 1 + 8, END_SENT, dtype=np.uint64),
             handle=np.full(2 * (q * limit + 4), END_SENT, dtype=np.uint64),
             keys=np.full(max(room[0], caps[0]) + 64, SENT, dtype=np.uint8), key_off=np.full(pairs + 9, END_SENT, dtype=np.uint64),
             values=np.full(max(room[1], caps[1]) + 64, SENT, dtype=np.uint8),
             value_off=np.full(pairs + 9, END_SENT, dtype=np.uint64), scanned=np.full(5 + 8, END_SENT, dtype=np.uint64))
    so = dlsm_amd._scan_out(q, limit, o["count"], o["pair_begin"], o["handle"], o["keys"], caps[0], o["key_off"], o["values"],
                            caps[1], o["value_off"], caps[2], o["scanned"])
    ks = Keys(data, q, 0, off).c()
    dlsm_amd.check(dlsm_amd.lib().dlsm_range_scan(ctx.h if ctx is not None else None, pa, la, ca,
                                                  begin.ctypes.data_as(C.POINTER(C.c_uint32)), n, tr, len(runs), C.byref(ks),
                                                  c["snapshot"], limit, C.byref(so)), "range_scan")
    return o


def untouched(a, start=0):
    return (a[start:] == SENTINEL[a.dtype]).all()


def run_case(c, ctx=None):
    w = want(c)
    got = scan(c, w["caps"], list(w["scanned"][2:4]) + [w["scanned"][1]], ctx)
    assert got["scanned"][:5].tolist() == list(w["scanned"]) and untouched(got["scanned"], 5)
    for k in OUTPUTS:
        x = w[k].reshape(-1)
        assert np.array_equal(got[k][:len(x)], x), k
        assert untouched(got[k], len(x)), k  # nothing at or past a cap or a total


@pytest.mark.parametrize("name", list(CASES))
def test_host_scan_against_the_python_iterator(name):
    run_case(CASES[name])


def test_host_scan_of_mismatched_tables_writes_only_scanned():
    got = scan(mismatch(), [1 << 12, 1 << 12, 64])
    s = got.pop("scanned")
    assert (s[0], s[4]) == (1, dlsm_amd.SCAN_TABLE_MISMATCH) and untouched(s, 5)
    for k, g in got.items():
        assert untouched(g), k


def test_the_wrapper_returns_the_same_arrays_cut_at_the_caps():
    c, w = CASES["cap-pairs"], want(CASES["cap-pairs"])
    data, off = keys_of(c["starts"])
    got = dlsm_amd.range_scan(*host_args(c), Keys(data, len(off) - 1, 0, off), c["snapshot"], c["limit"],
                              **dict(zip(("keys_cap", "values_cap", "pair_cap"), w["caps"])))
    assert got["scanned"] == w["scanned"]
    for k in OUTPUTS:
        assert np.array_equal(got[k], w[k]), k


def test_host_scan_rejects_bad_arguments():
    c = dict(two_files(), starts=[b""], snapshot=0, limit=4)
    blocks, files, _ = host_args(c)
    empty = build_index_block([], [])
    caps = [64, 64, 8]
    for change in (dict(runs=[]), dict(runs=[[0]] * 65),                         # n_runs outside 1..64
                   dict(runs=[[0, 2]]),                                          # a file >= n_files
                   dict(tables=[(blocks[0], files[0]), (None, files[1])]),       # no index held
                   dict(tables=[(blocks[0], files[0]), (blocks[1], None)]),      # no data held
                   dict(tables=[(empty, None)], runs=[[0] * 1024]),              # more than 1,023 files listed
                   dict(limit=0), dict(limit=dlsm_amd.SCAN_MAX_LIMIT + 1),       # limit outside 1..cap
                   dict(snapshot=1 << 56)):                                      # above kMaxSequenceNumber
        with pytest.raises(dlsm_amd.DlsmError) as e:
            scan(dict(c, **change), caps)
        assert e.value.status == -1, change
    for g in scan(dict(c, starts=[]), caps).values():  # Q == 0 touches nothing
        assert untouched(g)
