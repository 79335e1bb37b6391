"""The table index (dlsm_tableindex_create_blocks) and the batched index seek
(dlsm_index_seek_dev): Table::InternalGet's index step for the tasks of a read
plan.

The reference's Block and BlockBuilder cannot be compiled outside an RDMA host,
so the yardstick is pure Python and never calls the code under test: per file a
sorted list of (user_key, 2**64 - 1 - trailer), ``bisect_left`` for (user_key,
2**64 - 1 - (snapshot << 8 | 1)), then the state rules of table.cc:469-510.
Python's ``bytes`` order is BytewiseComparator's.  Every comparison is
``array_equal``; the outputs carry 8 sentinel entries behind them.
S is the implementation's fence interval, B its tasks per workgroup step.
"""
import bisect
import ctypes as C_
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import KV_HANDLE, Keys
from dlsm_amd import index_block as ib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXU64 = 2**64 - 1
MAXSEQ = (1 << 56) - 1
NOTFOUND, FOUND, DELETED, CORRUPT = 0, 1, 2, 3
TS_SENT, TH_SENT = 0xEE, 0xAB


class Table:
    """One table's pairs: rows of (user_key, seq, type, offset, size)."""

    def __init__(self, rows):
        rows = sorted(rows, key=lambda r: (r[0], MAXU64 - ((r[1] << 8) | r[2])))
        self.keys = [(r[0], MAXU64 - ((r[1] << 8) | r[2])) for r in rows]
        assert all(a < b for a, b in zip(self.keys, self.keys[1:])), "duplicate internal key"
        self.handles = [(r[3], r[4]) for r in rows]
        self.internal = [ib.internal_key(r[0], r[1], r[2]) for r in rows]

    def block(self):
        return ib.build_index_block(self.internal, self.handles)

    def seek(self, user_key, snapshot):
        """The yardstick: (state, offset, size)."""
        i = bisect.bisect_left(self.keys, (user_key, MAXU64 - ((snapshot << 8) | 1)))
        if i == len(self.keys):
            return NOTFOUND, 0, 0
        uk, inv = self.keys[i]
        t = (MAXU64 - inv) & 0xFF
        if t > 1:
            state = CORRUPT
        elif uk != user_key:
            return NOTFOUND, 0, 0
        else:
            state = FOUND if t == 1 else DELETED
        return (state,) + self.handles[i]


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def dev_keys(user_keys, fixed=None, suffix=0):
    """The batch on the device: variable-length (offsets) or fixed-stride."""
    if fixed is None:
        k = Keys.pack(list(user_keys))
        return Keys(dev(k.data), k.n, 0, dev(k.offsets), suffix)
    assert all(len(k) == fixed for k in user_keys)
    data = np.frombuffer(b"".join(user_keys) + b"\0" * 16, dtype=np.uint8)
    return Keys(dev(data), len(user_keys), fixed, None, suffix)


def seek(gpu, ti, keys, snapshot, begin, gets, cap, outputs=(True, True, True, True)):
    """Runs the seek on sentinel-filled outputs 8 entries longer than they need
    be; returns (task_state, task_handle, get_state, get_handle) as numpy."""
    import torch

    n = keys.n
    ts = torch.full((cap + 8,), TS_SENT, dtype=torch.uint8, device="cuda")
    th = torch.full((cap + 8, 16), TH_SENT, dtype=torch.uint8, device="cuda")
    gs = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    gh = torch.zeros((n + 8, 16), dtype=torch.uint8, device="cuda")
    gs[n:] = TS_SENT
    gh[n:] = TH_SENT
    gets_d = torch.full((max(len(gets), cap) + 8,), -1, dtype=torch.int32, device="cuda")
    gets_d[:len(gets)] = dev(np.asarray(gets, dtype=np.uint32))
    gpu.index_seek_dev(ti, keys, snapshot, dev(np.asarray(begin, dtype=np.uint64)), gets_d, cap=cap,
                       task_state=ts if outputs[0] else None, task_handle=th if outputs[1] else None,
                       get_state=gs if outputs[2] else None, get_handle=gh if outputs[3] else None)
    gpu.sync()
    return (ts.cpu().numpy(), th.cpu().numpy().reshape(-1).view(KV_HANDLE),
            gs.cpu().numpy(), gh.cpu().numpy().reshape(-1).view(KV_HANDLE))


def expected(tables, user_keys, snapshot, begin, gets, cap, first_shaped=True):
    """The four arrays the yardstick asks for, sentinels included."""
    n = len(user_keys)
    total = int(begin[-1])
    limit = min(total, cap)
    ts = np.full(cap + 8, TS_SENT, dtype=np.uint8)
    th = np.frombuffer(bytes([TH_SENT]) * (16 * (cap + 8)), dtype=KV_HANDLE).copy()
    gs = np.zeros(n + 8, dtype=np.uint8)
    gh = np.zeros(n + 8, dtype=KV_HANDLE)
    gs[n:] = TS_SENT
    gh[n:] = np.frombuffer(bytes([TH_SENT]) * 16, dtype=KV_HANDLE)[0]
    for f, tab in enumerate(tables):
        for t in range(int(begin[f]), min(int(begin[f + 1]), limit)):
            g = int(gets[t])
            st, off, size = (NOTFOUND, 0, 0) if tab is None else tab.seek(user_keys[g], snapshot)
            ts[t] = st
            th[t] = (off, size, f if st else 0)
            if st and first_shaped:
                gs[g] = st
                gh[g] = (off, size, f)
    return ts, th, gs, gh


def check(gpu, ti, tables, user_keys, keys, snapshot, begin, gets, cap=None, first_shaped=True):
    cap = int(begin[-1]) if cap is None else cap
    got = seek(gpu, ti, keys, snapshot, begin, gets, cap, (True, True, first_shaped, first_shaped))
    want = expected(tables, user_keys, snapshot, begin, gets, cap, first_shaped)
    for g, w, what in zip(got, want, ("task_state", "task_handle", "get_state", "get_handle")):
        assert np.array_equal(g, w), what
    return want


def plan_of(per_file_gets):
    """file_begin / gets of hand-made task lists (one list of Get indices per file)."""
    begin = np.zeros(len(per_file_gets) + 1, dtype=np.uint64)
    begin[1:] = np.cumsum([len(p) for p in per_file_gets])
    gets = np.array([g for p in per_file_gets for g in p], dtype=np.uint32)
    return begin, gets


@pytest.fixture(scope="module")
def S():
    s = dlsm_amd.index_fence_interval()
    assert s >= 2
    return s


@pytest.fixture(scope="module")
def B():
    b = dlsm_amd.index_seek_block()
    assert b >= 64
    return b


def uk20(v):
    return b"%020d" % v


def spaced_table(count, base=0, seq=7):
    """count entries with 20-byte user keys 2 apart (odd values lie between)."""
    return Table([(uk20(base + 2 * i + 2), seq + i, 1, 1000 * i + (i % 3), 40 + (i % 200)) for i in range(count)])


def all_targets(count, base=0):
    """below the first key, every entry's key, strictly between neighbours, above the last"""
    return [uk20(base + v) for v in range(1, 2 * count + 4)]


def test_entry_counts_and_targets(gpu, S, B):
    counts = [0, 1, 2, S - 1, S, S + 1, 2 * S + 1, 1000]
    # files without a task first and last, a file whose index is not held in the middle
    tables = [spaced_table(5)] + [spaced_table(c, base=100 * j) for j, c in enumerate(counts)]
    tables.insert(4, None)
    tables.append(spaced_table(3))
    ti = gpu.tableindex([None if t is None else t.block() for t in tables])
    assert ti.n_files == len(tables) and ti.n_entries == sum(len(t.keys) for t in tables if t is not None)
    user_keys, per_file = [], []
    for f, t in enumerate(tables):
        if f == 0 or f == len(tables) - 1:
            per_file.append([])
            continue
        tg = all_targets(5) if t is None else all_targets(len(t.keys), base=100 * (f - 1 - (f > 4)))
        per_file.append(list(range(len(user_keys), len(user_keys) + len(tg))))
        user_keys += tg
    begin, gets = plan_of(per_file)
    assert int(begin[-1]) > 4 * B  # the 1000-entry file's tasks straddle several workgroups' shares
    for snapshot in (3, MAXSEQ):  # below every sequence number, then above
        ts, _, _, _ = check(gpu, ti, tables, user_keys, dev_keys(user_keys, fixed=20), snapshot, begin, gets)
    assert (ts[:len(gets)] == NOTFOUND).any() and (ts[:len(gets)] == FOUND).any()
    ti.close()


def test_snapshots_and_states(gpu, S):
    seqs = [(10, 1), (20, 1), (30, 0), (40, 1), (50, 1)]  # one of the five is a deletion
    rows = [(b"key-b", s, t, 100 + s, 9) for s, t in seqs]
    rows += [(b"key-a", 5, 1, 1, 1), (b"key-c", 45, 2, 77, 7), (b"key-d", 60, 1, 2, 2)]  # key-c: type byte 2
    tab = Table(rows)
    ti = gpu.tableindex([tab.block()])
    snaps = [9, 10, 15, 20, 25, 30, 35, 40, 44, 45, 49, 50, 55, MAXSEQ]
    user_keys = [b"key-b", b"key-c", b"key-bb", b"key-a", b"key-d", b"key-e", b""]
    begin, gets = plan_of([list(range(len(user_keys)))])
    seen = set()
    for snap in snaps:
        ts, _, _, _ = check(gpu, ti, [tab], user_keys, dev_keys(user_keys), snap, begin, gets)
        seen |= set(ts[:len(gets)].tolist())
    assert seen == {NOTFOUND, FOUND, DELETED, CORRUPT}
    # below all of key-b's versions the seek lands on key-c (type 2): the reference reports kCorrupt
    assert tab.seek(b"key-b", 9)[0] == CORRUPT and tab.seek(b"key-c", 44)[0] == NOTFOUND
    assert tab.seek(b"key-b", 35)[0] == DELETED and tab.seek(b"key-b", 29) == (FOUND, 120, 9)
    ti.close()


def test_prefix_ties(gpu, S):
    p16 = b"0123456789abcdef"
    rows = []
    for i in range(2 * S + 5):  # more than 2S consecutive entries sharing their first 16 bytes
        rows.append((p16 + bytes([i * 3 + 1]), 5, 1, i, 1))
    for s in range(1, 3 * S):   # and as many versions of one user key
        rows.append((p16, s, s % 2, 10_000 + s, 2))
    shorts = [b"", b"a", b"ab", b"ab\0", b"ab\0\0", b"a" * 15, b"a" * 16, b"a" * 17, b"a" * 16 + b"\0",
              b"\x80", b"\x80\xff", b"\xff" * 16, b"\xff" * 17, b"\x7f" * 16]
    rows += [(k, 9, 1, 500 + j, 3) for j, k in enumerate(shorts)]
    tab = Table(rows)
    ti = gpu.tableindex([tab.block()])
    user_keys = sorted(set(k for k, *_ in rows) | {p16 + bytes([i]) for i in range(0, 256, 5)} |
                       {p16[:15], p16 + b"\0", b"ab\1", b"aa", b"\x80\0", b"\xfe", b"\xff" * 18, b"a" * 14})
    begin, gets = plan_of([list(range(len(user_keys)))])
    for snap in (MAXSEQ, 3 * S // 2, 1, 0):
        check(gpu, ti, [tab], user_keys, dev_keys(user_keys), snap, begin, gets)
    ti.close()


def test_encodings(gpu, S):
    """DecodeEntry's varint path (internal keys of 128 and 129 bytes), handle
    varints of every length up to 2^35 and sizes of 1 and 2 bytes, fixed
    28-byte internal-key lookups (suffix_len = 8) and variable-length ones."""
    offs = [v + d for v in (1 << 7, 1 << 14, 1 << 21, 1 << 28, 1 << 35) for d in (-1, 0, 1)]
    t20 = Table([(uk20(2 * i), 4, 1, o, 127 + (i % 3)) for i, o in enumerate(offs)])
    t120 = Table([(b"%0120d" % (2 * i), 4, 1, o, 128 - (i % 2)) for i, o in enumerate(offs)] +
                 [(b"%0121d" % (2 * i), 4, 1, o + 1, 200) for i, o in enumerate(offs)])
    mixed = Table([(b"%0120d" % 4, 9, 1, 1, 1), (b"x" * 119, 9, 1, 2, 2), (b"y" * 121, 9, 0, 1 << 34, 129),
                   (b"z", 9, 1, (1 << 63) + 5, 0xFFFFFFFF)])
    tables = [t20, t120, mixed]
    ti = gpu.tableindex([t.block() for t in tables])
    # fixed 28-byte internal keys, looked up as ExtractUserKey
    uks = [uk20(v) for v in range(0, 2 * len(offs) + 1)]
    begin, gets = plan_of([list(range(len(uks))), [], []])
    ik = [k + struct.pack("<Q", (99 << 8) | 1) for k in uks]
    check(gpu, ti, tables, uks, dev_keys(ik, fixed=28, suffix=8), MAXSEQ, begin, gets)
    check(gpu, ti, tables, uks, dev_keys(ik, suffix=8), MAXSEQ, begin, gets)
    long_keys = [b"%0120d" % v for v in range(0, 2 * len(offs) + 1)] + [b"%0121d" % v for v in range(0, 8)] + \
        [b"x" * 119, b"y" * 121, b"y" * 120, b"z", b"zz"]
    begin, gets = plan_of([[], list(range(len(long_keys))), list(range(len(long_keys)))])
    _, th, _, _ = check(gpu, ti, tables, long_keys, dev_keys(long_keys), MAXSEQ, begin, gets, first_shaped=False)
    assert int(th["offset"][:len(gets)].max()) == (1 << 63) + 5 and int(th["size"][:len(gets)].max()) == 0xFFFFFFFF
    ti.close()


def test_task_lists(gpu, S, B):
    tables = [spaced_table(40, base=0), spaced_table(700, base=0), None, spaced_table(9, base=0)]
    ti = gpu.tableindex([None if t is None else t.block() for t in tables])
    rng = np.random.default_rng(5)
    n = 3000
    user_keys = [uk20(int(v)) for v in rng.integers(0, 1500, n)]
    keys = dev_keys(user_keys, fixed=20)
    # arbitrary, non-ascending Get indices; file 1's tasks straddle the workgroups' shares
    per_file = [rng.permutation(n)[:50].tolist(), rng.permutation(n)[:3 * B + 17].tolist(),
                rng.permutation(n)[:20].tolist(), rng.permutation(n)[:33].tolist()]
    begin, gets = plan_of(per_file)
    total = int(begin[-1])
    for cap in (total + 100, total, total - 1, B, 1):
        check(gpu, ti, tables, user_keys, keys, MAXSEQ, begin, gets, cap=cap, first_shaped=False)
    # total 0: nothing is written
    check(gpu, ti, tables, user_keys, keys, MAXSEQ, np.zeros(5, dtype=np.uint64), gets, cap=64, first_shaped=False)
    # an ALL-shaped list: Get 7 in three files, read through the task arrays
    begin, gets = plan_of([[7, 8], [7, 9], [], [7]])
    ts, th, _, _ = check(gpu, ti, tables, user_keys, keys, MAXSEQ, begin, gets, first_shaped=False)
    # a FIRST-shaped one through the Get arrays, any subset of the outputs
    per_file = np.array_split(rng.permutation(n), 4)
    begin, gets = plan_of([p.tolist() for p in per_file])
    want = check(gpu, ti, tables, user_keys, keys, MAXSEQ, begin, gets)
    got = seek(gpu, ti, keys, MAXSEQ, begin, gets, int(begin[-1]), (False, False, True, False))
    assert np.array_equal(got[2], want[2]) and (got[0] == TS_SENT).all() and (got[3][:n] == np.zeros(1, KV_HANDLE)).all()
    # a Get index past the batch answers NOTFOUND and touches no Get array
    begin, gets = plan_of([[1, n + 5, 0xFFFFFFFF, 2], [], [], []])
    got = seek(gpu, ti, keys, MAXSEQ, begin, gets, 4)
    assert got[0][:4].tolist() == [tables[0].seek(user_keys[1], MAXSEQ)[0], 0, 0, tables[0].seek(user_keys[2], MAXSEQ)[0]]
    assert (got[2][n:] == TS_SENT).all()
    ti.close()


def corrupt_blocks(S):
    """(name, block, expected BLOCK_* code): the trailer's outcomes and one
    block per rule of the contents' validation."""
    t = spaced_table(2 * S + 3)
    good = t.block()
    c = bytearray(ib.build_index_contents(t.internal, t.handles))
    n = len(t.keys)
    r0 = len(c) - 4 * (n + 1)  # the restart array

    def edit(fn):
        d = bytearray(c)
        fn(d)
        return ib.seal(bytes(d))

    def put32(d, at, v):
        d[at:at + 4] = struct.pack("<I", v)

    e1 = struct.unpack_from("<I", c, r0 + 4)[0]  # entry 1's offset
    swapped = ib.build_index_block([t.internal[1], t.internal[0]] + t.internal[2:], t.handles)
    equal = ib.build_index_block([t.internal[0], t.internal[0]] + t.internal[2:], t.handles)
    bad_type = bytearray(good)
    bad_type[-5] = 1
    bad_type[-4:] = struct.pack("<I", dlsm_amd.crc32c_mask(dlsm_amd.crc32c(bytes(bad_type[:-4]))))
    flipped = bytearray(good)
    flipped[len(good) // 2] ^= 0x10
    out = [
        ("good", good, dlsm_amd.BLOCK_OK),
        ("short", good[:4], dlsm_amd.BLOCK_SHORT),
        ("checksum", bytes(flipped), dlsm_amd.BLOCK_CHECKSUM),
        ("type", bytes(bad_type), dlsm_amd.BLOCK_TYPE),
        ("empty table", ib.seal(struct.pack("<I", 0)), dlsm_amd.BLOCK_OK),
        ("len < 4", ib.seal(b"\0\0\0"), dlsm_amd.BLOCK_INDEX),
        ("num_restarts too large", edit(lambda d: put32(d, len(d) - 4, (len(d) - 4) // 4 + 1)), dlsm_amd.BLOCK_INDEX),
        ("num_restarts past the bytes", edit(lambda d: put32(d, len(d) - 4, (len(d) - 4) // 4)), dlsm_amd.BLOCK_INDEX),
        ("restart[0] != 0", edit(lambda d: put32(d, r0, 1)), dlsm_amd.BLOCK_INDEX),
        ("restarts not ascending", edit(lambda d: put32(d, r0 + 8, e1)), dlsm_amd.BLOCK_INDEX),
        ("restart past the entries", edit(lambda d: put32(d, r0 + 4 * (n - 1), r0 + 1)), dlsm_amd.BLOCK_INDEX),
        ("shared != 0", edit(lambda d: d.__setitem__(e1, 1)), dlsm_amd.BLOCK_INDEX),
        ("non_shared < 8", ib.build_index_block([b"1234567"], [(1, 1)]), dlsm_amd.BLOCK_INDEX),
        ("entry overruns the next", edit(lambda d: d.__setitem__(e1 + 1, 29)), dlsm_amd.BLOCK_INDEX),
        ("entry ends early", edit(lambda d: d.__setitem__(e1 + 1, 27)), dlsm_amd.BLOCK_INDEX),
        ("varint header without end", edit(lambda d: d.__setitem__(slice(e1, e1 + 6), b"\x80" * 6)), dlsm_amd.BLOCK_INDEX),
        ("value not two varints", edit(lambda d: d.__setitem__(e1 + 3 + 28, d[e1 + 3 + 28] | 0x80) or
                                       d.__setitem__(e1 + 3 + 29, d[e1 + 3 + 29] | 0x80)), dlsm_amd.BLOCK_INDEX),
        ("order: swapped", swapped, dlsm_amd.BLOCK_INDEX),
        ("order: equal keys", equal, dlsm_amd.BLOCK_INDEX),
    ]
    return out


@pytest.mark.parametrize("on_device", [False, True])
def test_open_outcomes(gpu, S, on_device):
    import torch

    cases = corrupt_blocks(S)
    want = np.array([c[2] for c in cases], dtype=np.uint8)
    assert set(want.tolist()) == {0, 1, 2, 3, 5}

    def blocks(sel):
        bl = [cases[j][1] for j in sel]
        return [torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() for b in bl] if on_device else bl

    every = list(range(len(cases)))
    with pytest.raises(dlsm_amd.BlockError) as e:  # *out == NULL is asserted inside TableIndex
        gpu.tableindex(blocks(every), on_device)
    assert np.array_equal(e.value.block_status, want), [c[0] for c, g in zip(cases, e.value.block_status) if c[2] != g]
    # one bad block at a time, in a different place each time, with a NULL neighbour
    for j in every:
        if cases[j][2] == dlsm_amd.BLOCK_OK:
            continue
        order = [0, j, 4] if j % 2 else [j, 0, 4]
        with pytest.raises(dlsm_amd.BlockError) as e:
            gpu.tableindex(blocks(order) + [None], on_device)
        assert np.array_equal(e.value.block_status, np.append(want[order], 0)), cases[j][0]
    # without checksum verification the flipped byte is judged by the contents' rules alone
    good = [j for j in every if cases[j][2] == dlsm_amd.BLOCK_OK]
    ti = gpu.tableindex(blocks(good), on_device, verify_checksums=False)
    assert ti.n_entries == 2 * S + 3
    ti.close()
    bad_crc = bytearray(cases[0][1])
    bad_crc[-1] ^= 0xFF  # the stored crc, not the contents
    b = [torch.from_numpy(np.frombuffer(bytes(bad_crc), dtype=np.uint8).copy()).cuda()] if on_device else [bytes(bad_crc)]
    with pytest.raises(dlsm_amd.BlockError):
        gpu.tableindex(b, on_device)
    ti = gpu.tableindex(b, on_device, verify_checksums=False)
    assert ti.n_entries == 2 * S + 3
    ti.close()


def test_open_70001_files(gpu):
    """70,001 one-entry files open with the same four launches and one
    synchronisation as one file (the file index never lives in a grid
    dimension), and seek through the file_begin search that does not fit LDS."""
    import torch

    nf = 70_001
    blocks = [ib.build_index_block([ib.internal_key(b"%08d" % f, 3, 1)], [(f, 1 + f % 100)]) for f in range(nf)]
    at = np.zeros(nf + 1, dtype=np.int64)  # the blocks lie back to back, at any alignment
    at[1:] = np.cumsum([len(b) for b in blocks])
    flat = torch.from_numpy(np.frombuffer(b"".join(blocks), dtype=np.uint8).copy()).cuda()
    ti = gpu.tableindex([flat[at[f]:at[f + 1]] for f in range(nf)], on_device=True)
    assert ti.n_files == nf and ti.n_entries == nf
    rng = np.random.default_rng(3)
    files = np.sort(rng.choice(nf, 500, replace=False))
    files[0], files[-1] = 0, nf - 1
    user_keys = [b"%08d" % (f + (j % 3 == 0)) for j, f in enumerate(files)]
    cnt = np.zeros(nf, dtype=np.int64)
    cnt[files] = 1
    begin = np.zeros(nf + 1, dtype=np.uint64)
    begin[1:] = np.cumsum(cnt)
    gets = np.arange(len(files), dtype=np.uint32)
    ts, th, gs, gh = seek(gpu, ti, dev_keys(user_keys, fixed=8), MAXSEQ, begin, gets, len(files))
    hit = np.array([j % 3 != 0 for j in range(len(files))])
    assert np.array_equal(ts[:len(files)], hit.astype(np.uint8))
    assert np.array_equal(th["file"][:len(files)][hit], files[hit].astype(np.uint32))
    assert np.array_equal(th["offset"][:len(files)][hit], files[hit].astype(np.uint64))
    assert np.array_equal(gs[:len(files)], ts[:len(files)]) and (ts[len(files):] == TS_SENT).all()
    ti.close()


def test_round_loop_end_to_end(gpu):
    """probe -> plan(FIRST) -> seek -> advance to exhaustion on make_version's
    version, against a Python walk of the probe's own masks in slot order
    through the yardstick.  Each table holds the lookups inside its key range
    that a hash keeps, so a key lives in a level-0 file and, older, deeper."""
    import torch

    from test_gpu_read_plan import file_tables
    from test_version_probe import lookups, make_version

    files = make_version(0, with_nofilter=True)
    nf = len(files)
    n = 6000
    q = lookups(n, 33)
    uks = [q[20 * i:20 * i + 20].tobytes() for i in range(n)]
    distinct = sorted(set(uks))
    tables = []
    for f, vf in enumerate(files):
        rows = []
        for k in distinct:
            h = zlib.crc32(k) + 7919 * f
            if bytes(vf.smallest) <= k <= bytes(vf.largest) and h % 3 != 0:
                typ = 0 if h % 11 == 0 else (2 if h % 97 == 1 else 1)
                rows.append((k, 1000 - 10 * vf.level - (h % 5), typ, (h % 100_000) * 64, 30 + h % 300))
        tables.append(Table(rows))
    snap = 1 << 45
    v = gpu.version(files)
    ti = gpu.tableindex([t.block() for t in tables])
    keys = Keys(dev(q), n, 20)
    mask = torch.zeros(n, dtype=torch.int64, device="cuda")
    lf = torch.zeros((n, 5), dtype=torch.int32, device="cuda")
    gpu.version_probe_dev(v, keys, snap, mask, lf)
    gpu.sync()
    mask0 = mask.cpu().numpy().view(np.uint64).copy()
    lf0 = lf.cpu().numpy().view(np.uint32).copy()
    begin = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
    gets = torch.zeros(n, dtype=torch.int32, device="cuda")
    gs = torch.zeros(n, dtype=torch.uint8, device="cuda")
    gh = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
    rounds = 0
    while True:
        gpu.version_read_plan_dev(v, mask, lf, dlsm_amd.PLAN_FIRST, begin, gets)
        gpu.index_seek_dev(ti, keys, snap, begin, gets, get_state=gs, get_handle=gh)
        gpu.version_masks_advance_dev(mask, gs)
        if int(begin[nf].item()) == 0:  # the 8-byte "is anything left" check
            break
        rounds += 1
        assert rounds <= v.n_slots
    # the walk Version::Get makes: the probe's slots in order, the first non-zero state ends it
    l0, lv = file_tables(files)
    want_s = np.zeros(n, dtype=np.uint8)
    want_h = np.zeros(n, dtype=KV_HANDLE)
    both = 0
    for g in range(n):
        hits = []
        for s in range(v.n_slots):
            if not (int(mask0[g]) >> s) & 1:
                continue
            f = int(l0[s]) if s < len(l0) else int(lv[s - len(l0)][int(lf0[g, s - len(l0)])])
            st, off, size = tables[f].seek(uks[g], snap)
            if st:
                hits.append((s, st, off, size, f))
        if hits:
            _, st, off, size, f = hits[0]
            want_s[g] = st
            want_h[g] = (off, size, f)
            both += len(hits) > 1 and hits[0][0] < len(l0) <= hits[1][0]
    assert rounds >= 2 and both > 0 and set(want_s.tolist()) == {0, 1, 2, 3}
    assert np.array_equal(gs.cpu().numpy(), want_s)
    assert np.array_equal(gh.cpu().numpy().reshape(-1).view(KV_HANDLE), want_h)
    a, b = C_.c_uint64(), C_.c_uint64()
    assert dlsm_amd.lib().dlsm_fallback_stats(gpu.h, C_.byref(a), C_.byref(b)) == 0 and a.value == 0
    ti.close()
    v.close()


def test_adapter_table_index_gpu_leg(tmp_path):
    """dlsm_adapter::TableIndex::SeekPlan on the GPU against its own host path
    (tests/cpp/adapter_index_test.cc, the program test_index_seek_host.py runs on the CPU)."""
    from test_index_seek_host import compile_adapter_index_test

    exe = compile_adapter_index_test(tmp_path)
    out = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK adapter index gpu" in out.stdout, out.stdout + out.stderr
