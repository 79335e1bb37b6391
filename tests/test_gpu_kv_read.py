"""The value read of a seeked Get batch (dlsm_tabledata_create,
dlsm_kv_read_dev): the tail of Table::InternalGet for byte-addressable tables.

TableBuilder_BACS cannot be compiled outside an RDMA host, so the yardstick is
pure Python and never calls the code under test: per file a dict from offset to
(internal key, value), built beside the region by dlsm_amd/data_region.py's
writer, and the rules of include/dlsm_bloom.h restated over the region's bytes
(``bisect_right`` over the chunk ends is Find_Remote_MR's upper_bound).  Expected
offsets are ``np.cumsum``, expected bytes ``b"".join``; every comparison is
``array_equal``.  Every output carries sentinels: 8 entries behind the arrays,
64 bytes behind ``values`` and behind ``values_cap``.
C is the implementation's items per workgroup chunk, Sp its output bytes per
workgroup step of the copy.
"""
import bisect
import ctypes as C_
import struct
import subprocess

import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import KV_HANDLE, Keys
from dlsm_amd import data_region as dr
from dlsm_amd import index_block as ib

pytestmark = pytest.mark.gpu

NOTFOUND, FOUND, DELETED, CORRUPT = 0, 1, 2, 3
MAXSEQ = (1 << 56) - 1
ST_SENT, OFF_SENT, VAL_SENT = 0xEE, 0x5A5A5A5A5A5A5A5A, 0xCD


class FileData:
    """One file's data region: its chunks, the running chunk ends and the dict
    offset -> (internal key, value) of the pairs written."""

    def __init__(self, pairs, chunk_bytes=None):
        self.chunks, self.handles = dr.build_region(pairs, chunk_bytes)
        self.ends = np.cumsum([len(c) for c in self.chunks]).tolist()
        self.pairs = {off: (k, v) for (off, _), (k, v) in zip(self.handles, pairs)}

    def bytes_at(self, off, size):
        """The rules' chunk lookup: the size bytes at off, or None."""
        c = bisect.bisect_right(self.ends, off)
        if c == len(self.ends) or off + size > self.ends[c]:
            return None
        at = off - (self.ends[c - 1] if c else 0)
        return self.chunks[c][at:at + size]


def rule(files, state, h, user_key):
    """(state, value) of one item by the rules; value is b"" unless FOUND."""
    off, size, f = int(h[0]), int(h[1]), int(h[2])
    if state != FOUND:
        return state, b""
    if user_key is None or f >= len(files) or files[f] is None:
        return CORRUPT, b""
    p = files[f].bytes_at(off, size) if size >= 16 else None
    if p is None:
        return CORRUPT, b""
    ks, vs = struct.unpack_from("<II", p, 0)
    if ks < 8 or 8 + ks + vs != size:
        return CORRUPT, b""
    typ = p[8 + ks - 8]
    if typ > 1 or p[8:8 + ks - 8] != user_key:
        return CORRUPT, b""
    out = (DELETED, b"") if typ == 0 else (FOUND, p[8 + ks:8 + ks + vs])
    k, v = files[f].pairs[off]  # a well-formed pair is one the writer wrote
    assert p[8:8 + ks] == k and p[8 + ks:] == v
    return out


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == KV_HANDLE:
        a = a.view(np.uint8).reshape(-1, 16)
    return torch.from_numpy(a.copy()).cuda()


def dev_keys(user_keys, fixed=None, suffix=0):
    if fixed is None:
        k = Keys.pack(list(user_keys))
        return Keys(dev(k.data), k.n, 0, dev(k.offsets), suffix)
    assert all(len(k) == fixed for k in user_keys)
    return Keys(dev(np.frombuffer(b"".join(user_keys) + b"\0" * 16, dtype=np.uint8)), len(user_keys), fixed, None, suffix)


def handles_of(rows):
    h = np.zeros(len(rows), dtype=KV_HANDLE)
    for j, r in enumerate(rows):
        h[j] = r
    return h


def read(gpu, td, keys, state, handle, *, gets=None, count=None, cap=None, values_cap=None, room=0):
    """Runs the read on sentinel-filled outputs; returns (state, value_off,
    values, n_corrupt) as numpy, sentinels included.  The values buffer holds
    values_cap + 64 bytes (and at least room + 64)."""
    import torch

    cap = len(state) if cap is None else cap
    st = torch.full((max(cap, len(state)) + 8,), ST_SENT, dtype=torch.uint8, device="cuda")
    st[:len(state)] = dev(np.asarray(state, dtype=np.uint8))
    hd = torch.full((max(cap, len(handle)) + 8, 16), 0xAB, dtype=torch.uint8, device="cuda")
    if len(handle):
        hd[:len(handle)] = dev(handle)
    vo = dev(np.full(cap + 1 + 8, OFF_SENT, dtype=np.uint64))
    values_cap = room if values_cap is None else values_cap
    vb = torch.full((max(values_cap, room) + 64,), VAL_SENT, dtype=torch.uint8, device="cuda")
    nc = dev(np.full(1 + 8, OFF_SENT, dtype=np.uint64))
    gd = None
    if gets is not None:
        gd = torch.full((max(cap, len(gets)) + 8,), -1, dtype=torch.int32, device="cuda")
        gd[:len(gets)] = dev(np.asarray(gets, dtype=np.uint32))
    cd = None if count is None else dev(np.array([7, count, 9], dtype=np.uint64))[1:]
    gpu.kv_read_dev(td, keys, st, hd, vo, vb, gets=gd, count=cd, cap=cap, values_cap=values_cap, n_corrupt=nc)
    gpu.sync()
    return (st.cpu().numpy(), vo.cpu().numpy().view(np.uint64), vb.cpu().numpy(), nc.cpu().numpy().view(np.uint64))


def expected(files, user_keys, state, handle, *, gets=None, count=None, cap=None, values_cap=None, room=0):
    cap = len(state) if cap is None else cap
    m = cap if count is None else min(count, cap)
    st = np.full(max(cap, len(state)) + 8, ST_SENT, dtype=np.uint8)
    st[:len(state)] = state
    vals, bad = [], 0
    for i in range(m):
        g = i if gets is None else int(gets[i])
        s, v = rule(files, int(state[i]), handle[i], user_keys[g] if g < len(user_keys) else None)
        bad += s == CORRUPT and state[i] == FOUND
        st[i] = s
        vals.append(v)
    vo = np.full(cap + 1 + 8, OFF_SENT, dtype=np.uint64)
    vo[0] = 0
    vo[1:m + 1] = np.cumsum([len(v) for v in vals], dtype=np.uint64)
    blob = b"".join(vals)
    values_cap = room if values_cap is None else values_cap
    vb = np.full(max(values_cap, room) + 64, VAL_SENT, dtype=np.uint8)
    k = min(len(blob), values_cap)
    vb[:k] = np.frombuffer(blob[:k], dtype=np.uint8)
    nc = np.full(9, OFF_SENT, dtype=np.uint64)
    nc[0] = bad
    return st, vo, vb, nc


def check(gpu, td, files, user_keys, keys, state, handle, **kw):
    """values_cap and room default to the total: the whole blob is compared."""
    want = expected(files, user_keys, state, handle, **kw)
    if kw.get("values_cap") is None and not kw.get("room"):
        cap = len(state) if kw.get("cap") is None else kw["cap"]
        m = cap if kw.get("count") is None else min(kw["count"], cap)
        kw["room"] = int(want[1][m])
        want = expected(files, user_keys, state, handle, **kw)
    got = read(gpu, td, keys, state, handle, **kw)
    for g, w, what in zip(got, want, ("state", "value_off", "values", "n_corrupt")):
        assert np.array_equal(g, w), (what, np.nonzero(g != w)[0][:8])
    return want


def no_fallback(gpu):
    a, b = C_.c_uint64(), C_.c_uint64()
    assert dlsm_amd.lib().dlsm_fallback_stats(gpu.h, C_.byref(a), C_.byref(b)) == 0 and a.value == 0


@pytest.fixture(scope="module")
def C():
    c = dlsm_amd.kv_read_chunk()
    assert c >= 64
    return c


@pytest.fixture(scope="module")
def Sp():
    s = dlsm_amd.kv_read_span()
    assert s >= 16 and s % 16 == 0
    return s


def ukey(j, n):
    return bytes((j * 7 + i * 3 + 1) % 251 for i in range(n))


def make_pairs(lengths, rng, key_len=lambda j: 1 + j % 40, typ=lambda j: 1):
    blob = rng.integers(0, 256, int(sum(lengths)) + 1, dtype=np.uint8).tobytes()
    pairs, uks, at = [], [], 0
    for j, n in enumerate(lengths):
        uk = ukey(j, key_len(j))
        uks.append(uk)
        pairs.append((ib.internal_key(uk, 5 + j, typ(j)), blob[at:at + n]))
        at += n
    return pairs, uks


def one_file(gpu, lengths, seed, **kw):
    pairs, uks = make_pairs(lengths, np.random.default_rng(seed), **kw)
    fd = FileData(pairs)
    td = gpu.tabledata([fd.chunks])
    h = handles_of([(o, s, 0) for o, s in fd.handles])
    return fd, td, uks, h


def test_unit_path_against_byte_path(gpu, Sp):
    base = [0, 1, 15, 16, 17, 31, 32, 33, Sp - 1, Sp, Sp + 1, 3 * Sp + 5]
    lengths = []
    for _ in range(16):
        lengths += base + [1]
    if sum(lengths) % 16 == 0:
        lengths.append(3)
    fd, td, uks, h = one_file(gpu, lengths, 1)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    big = np.array(lengths) >= 16
    assert set((starts[big] % 16).tolist()) == set(range(16))           # destination residues
    src = np.array([o + 8 + len(uks[j]) + 8 for j, (o, _) in enumerate(fd.handles)])
    assert set((src[big] % 16).tolist()) == set(range(16))              # source residues
    assert sum(lengths) % 16 != 0
    state = np.full(len(lengths), FOUND, dtype=np.uint8)
    want = check(gpu, td, [fd], uks, dev_keys(uks), state, h)
    assert int(want[1][len(lengths)]) == sum(lengths)
    # two runs give identical bytes
    a = read(gpu, td, dev_keys(uks), state, h, room=sum(lengths))
    b = read(gpu, td, dev_keys(uks), state, h, room=sum(lengths))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    no_fallback(gpu)
    td.close()


def test_empty_and_tiny_values(gpu, Sp):
    lengths = [40] + [0] * 3000 + [25] + [1] * (2 * Sp) + [0, 0, 7]
    fd, td, uks, h = one_file(gpu, lengths, 2, key_len=lambda j: 1 + j % 5)
    keys = dev_keys(uks)
    state = np.full(len(lengths), FOUND, dtype=np.uint8)
    check(gpu, td, [fd], uks, keys, state, h)
    # m = 1 and m = 0 (by count, and by cap)
    check(gpu, td, [fd], uks, keys, state, h, count=1)
    check(gpu, td, [fd], uks, keys, state[:1], h[:1])
    got = check(gpu, td, [fd], uks, keys, state, h, count=0, room=64)
    assert int(got[1][0]) == 0
    got = read(gpu, td, keys, state[:0], h[:0], cap=0, room=64)
    assert (got[1] == OFF_SENT).all() and (got[2] == VAL_SENT).all()   # cap == 0 touches nothing
    # all items non-FOUND: the total is 0 and no byte is written
    for s in (NOTFOUND, DELETED, CORRUPT):
        want = check(gpu, td, [fd], uks, keys, np.full(len(lengths), s, dtype=np.uint8), h, room=64)
        assert int(want[1][len(lengths)]) == 0 and int(want[3][0]) == 0
    no_fallback(gpu)
    td.close()


def test_one_large_value(gpu, Sp):
    lengths = [3, 100, 5 * 1024 * 1024 + 11, 0, 9, 400]
    assert lengths[2] > 64 * Sp
    fd, td, uks, h = one_file(gpu, lengths, 3)
    check(gpu, td, [fd], uks, dev_keys(uks), np.full(len(lengths), FOUND, dtype=np.uint8), h)
    td.close()


def test_partial_sums(gpu, C):
    rng = np.random.default_rng(4)
    m = 3 * C + 17
    lengths = rng.integers(1, 9, m).tolist()
    fd, td, uks, h = one_file(gpu, lengths, 4, key_len=lambda j: 2 + j % 7)
    state = np.full(m, FOUND, dtype=np.uint8)
    state[rng.integers(0, m, 50)] = NOTFOUND
    check(gpu, td, [fd], uks, dev_keys(uks), state, h)
    td.close()


def test_more_than_one_chunk_per_workgroup(gpu, C):
    """m = 512 C + 3 through the vectorised writer: the partial-sum table is
    full and a workgroup takes two chunks."""
    m, klen, vlen = 512 * C + 3, 28, 5
    rng = np.random.default_rng(5)
    n = 4096
    uk = np.frombuffer(b"".join(b"%020d" % v for v in range(n)), dtype=np.uint8).reshape(n, 20)
    ik = np.concatenate([uk, np.tile(np.frombuffer(struct.pack("<Q", (9 << 8) | 1), dtype=np.uint8), (n, 1))], axis=1)
    vals = rng.integers(0, 256, (n, vlen), dtype=np.uint8)
    region, offs, sizes = dr.build_region_fixed(ik, vals)
    rows = rng.integers(0, n, m)
    rows[m // 3] = n  # one handle past the region
    h = np.zeros(m, dtype=KV_HANDLE)
    h["offset"], h["size"] = rows.astype(np.uint64) * np.uint64(8 + klen + vlen), 8 + klen + vlen
    td = gpu.tabledata([[dev(region)]], on_device=True)
    keys = Keys(dev(uk[np.minimum(rows, n - 1)].reshape(-1)), m, 20)
    state = np.full(m, FOUND, dtype=np.uint8)
    st, vo, vb, nc = read(gpu, td, keys, state, h, room=m * vlen)
    lens = np.full(m, vlen, dtype=np.uint64)
    lens[m // 3] = 0
    want_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    good = np.delete(np.arange(m), m // 3)
    assert np.array_equal(vo[:m + 1], want_off) and (vo[m + 1:] == OFF_SENT).all()
    assert np.array_equal(vb[:(m - 1) * vlen], vals[rows[good]].reshape(-1)) and (vb[(m - 1) * vlen:] == VAL_SENT).all()
    assert int(nc[0]) == 1 and st[m // 3] == CORRUPT and (np.delete(st[:m], m // 3) == FOUND).all()
    assert (st[m:] == ST_SENT).all()
    no_fallback(gpu)
    td.close()


def test_values_cap(gpu, Sp):
    lengths = [5, 100, 33, 0, 2 * Sp + 3, 64, 1]
    fd, td, uks, h = one_file(gpu, lengths, 6)
    keys = dev_keys(uks)
    total = sum(lengths)
    state = np.full(len(lengths), FOUND, dtype=np.uint8)
    for cap_b in (total - 1, 5 + 50, 5 + 100 + 33 + Sp + 7, 138 + 2 * Sp + 3, 16, 0, total, total + 40):
        want = check(gpu, td, [fd], uks, keys, state, h, values_cap=cap_b, room=total)
        assert int(want[1][len(lengths)]) == total  # value_off is exact whatever the cap
    td.close()


def test_rejection_rules(gpu):
    rng = np.random.default_rng(7)
    good, uks = make_pairs([30, 0, 12, 50, 9], rng, key_len=lambda j: 4 + j, typ=lambda j: 0 if j == 2 else 1)

    def raw(ks, vs, key, value):
        return struct.pack("<II", ks, vs) + key + value

    k9 = ib.internal_key(b"k", 3, 1)
    # hand-written pairs behind the writer's: each as (bytes, user key, handle size)
    odd = [
        (raw(7, 9, b"1234567", b"v" * 9), b"", 24),                        # key_size < 8
        (raw(9, 11, k9, b"v" * 10), b"k", 27),                             # lengths say one byte more than the size
        (raw(9, 9, k9, b"v" * 10), b"k", 27),                              # ... and one byte less
        (raw(9, 0xFFFFFFFF, k9, b""), b"k", 16),                           # 8 + 9 + 0xFFFFFFFF is 16 in 32 bits
        (raw(9, 3, ib.internal_key(b"k", 3, 2), b"abc"), b"k", 20),        # type byte 2
        (raw(9, 3, k9, b"abc"), b"j", 20),                                 # user-key mismatch
        (raw(9, 3, k9, b"abc"), b"kk", 20),                                # ... a longer key
        (raw(8, 0, ib.internal_key(b"", 3, 1), b""), b"", 16),             # the least pair: FOUND, empty
    ]
    fd = FileData(good, chunk_bytes=80)
    assert len(fd.chunks) >= 2
    tail = b"".join(o[0] for o in odd)
    base = fd.ends[-1]
    fd.chunks.append(tail)
    fd.ends.append(base + len(tail))
    rows, keys_l, at = [], [], base
    for j, (o, s) in enumerate(fd.handles):
        rows.append((o, s, 1))
        keys_l.append(uks[j])
    for b, uk, size in odd:
        rows.append((at, size, 1))
        keys_l.append(uk)
        at += len(b)
    fd.pairs[rows[-1][0]] = (ib.internal_key(b"", 3, 1), b"")
    end0 = fd.ends[0]
    first1 = fd.handles[[o >= end0 for o, _ in fd.handles].index(True)]
    rows += [
        (0, fd.handles[0][1], 2),                       # file >= n_files ... (file 2 holds no data)
        (0, fd.handles[0][1], 3),                       # file >= n_files
        (0, fd.handles[0][1], 0xFFFFFFFF),
        (fd.ends[-1], 16, 1),                           # an offset past every chunk
        (1 << 63, 20, 1),
        (end0 - 10, 10 + first1[1], 1),                 # a pair straddling a chunk end
        (fd.handles[0][0], fd.handles[0][1] + (end0 - fd.handles[0][1]) + 1, 1),
        (fd.handles[0][0], 15, 1),                      # size < 16
        (fd.handles[0][0], 0, 1),
    ]
    keys_l += [uks[0]] * 9
    files = [None, fd, None]
    td = gpu.tabledata([None, fd.chunks, []])
    assert td.n_files == 3 and td.n_chunks == len(fd.chunks)
    h = handles_of(rows)
    n = len(rows)
    state = np.full(n, FOUND, dtype=np.uint8)
    want = check(gpu, td, files, keys_l, dev_keys(keys_l), state, h)
    assert want[0][:n].tolist() == [FOUND, FOUND, DELETED, FOUND, FOUND] + [CORRUPT] * 7 + [FOUND] + [CORRUPT] * 9
    assert int(want[3][0]) == 16
    # incoming NOTFOUND, DELETED and CORRUPT items with wild handles pass through and are never dereferenced
    wild = handles_of([(0xDEAD0000_00000000 + j, 0xFFFFFFF0, (1, 7, 0xFFFFFFFF)[j % 3]) for j in range(n)])
    for s in (NOTFOUND, DELETED, CORRUPT):
        check(gpu, td, files, keys_l, dev_keys(keys_l), np.full(n, s, dtype=np.uint8), wild, room=64)
    mixed = np.where(np.arange(n) % 2 == 0, FOUND, DELETED).astype(np.uint8)
    hm = h.copy()
    hm[1::2] = wild[1::2]
    check(gpu, td, files, keys_l, dev_keys(keys_l), mixed, hm)
    no_fallback(gpu)
    td.close()


@pytest.mark.parametrize("on_device", [False, True])
def test_chunk_lookup(gpu, on_device):
    """A file of 70 unequal chunks beside a one-chunk file; pairs at the first
    and last bytes of chunks; host chunks (copied) and device chunks
    (referenced) give the same arrays (both are held to the yardstick)."""
    rng = np.random.default_rng(8)
    lengths = rng.integers(0, 60, 400).tolist()
    pairs, uks = make_pairs(lengths, rng, key_len=lambda j: 1 + j % 13)
    fd = FileData(pairs, chunk_bytes=None)
    # cut the region into 70 chunks at pair boundaries, unequal
    cuts = sorted(rng.choice(np.arange(1, len(pairs)), 69, replace=False).tolist())
    bounds = [0] + [fd.handles[c][0] for c in cuts] + [fd.ends[-1]]
    region = fd.chunks[0]
    fd.chunks = [region[a:b] for a, b in zip(bounds, bounds[1:])]
    fd.ends = bounds[1:]
    assert len(fd.chunks) == 70 and len(set(len(c) for c in fd.chunks)) > 20
    other = FileData(pairs[:5])
    files = [other, fd]
    rows = [(o, s, 1) for o, s in fd.handles] + [(o, s, 0) for o, s in other.handles]
    keys_l = uks + uks[:5]
    # the pair behind each cut starts at an offset equal to a chunk end; a handle
    # that starts there but belongs, by its size, to neither chunk is rejected
    rows += [(fd.ends[0], fd.ends[1] - fd.ends[0] + 1, 1), (fd.ends[3] - 1, 17, 1)]
    keys_l += [uks[cuts[0]], uks[0]]
    chunks = [[dev(np.frombuffer(c, dtype=np.uint8)) for c in f.chunks] for f in files] if on_device \
        else [f.chunks for f in files]
    td = gpu.tabledata(chunks, on_device)
    assert td.n_chunks == 71
    state = np.full(len(rows), FOUND, dtype=np.uint8)
    want = check(gpu, td, files, keys_l, dev_keys(keys_l), state, handles_of(rows))
    assert int(want[3][0]) == 2 and (want[0][:len(rows) - 2] == FOUND).all()
    td.close()


def test_per_task_form(gpu):
    rng = np.random.default_rng(9)
    a = FileData(make_pairs([10, 20, 30], rng, key_len=lambda j: 3)[0])
    pairs_b, uks = make_pairs([11, 21, 31], rng, key_len=lambda j: 3)
    b = FileData(pairs_b)
    files = [a, b]
    td = gpu.tabledata([a.chunks, b.chunks])
    keys = dev_keys(uks)
    # Get 1 in two files; a gets entry >= keys.n
    gets = [1, 0, 1, 2, 3, 0xFFFFFFFF, 2]
    rows = [a.handles[1] + (0,), a.handles[0] + (0,), b.handles[1] + (1,), b.handles[2] + (1,), a.handles[0] + (0,),
            a.handles[0] + (0,), a.handles[2] + (0,)]
    h = handles_of(rows)
    state = np.full(len(rows), FOUND, dtype=np.uint8)
    want = check(gpu, td, files, uks, keys, state, h, gets=gets)
    assert want[0][:7].tolist() == [FOUND] * 4 + [CORRUPT, CORRUPT, FOUND]
    # count_dev below and above cap
    for count, cap in ((3, 7), (7, 7), (100, 7), (100, 4), (0, 7), (5, 6)):
        check(gpu, td, files, uks, keys, state, h, gets=gets, count=count, cap=cap)
    td.close()


def test_key_shapes(gpu):
    rng = np.random.default_rng(10)
    n = 300
    uks = [b"%020d" % (3 * j) for j in range(n)]
    vals = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in rng.integers(0, 90, n)]
    fd = FileData([(ib.internal_key(k, 9, 1), v) for k, v in zip(uks, vals)])
    td = gpu.tabledata([fd.chunks])
    h = handles_of([(o, s, 0) for o, s in fd.handles])
    state = np.full(n, FOUND, dtype=np.uint8)
    iks = [k + struct.pack("<Q", (77 << 8) | 1) for k in uks]
    check(gpu, td, [fd], uks, dev_keys(uks, fixed=20), state, h)             # 20-byte fixed keys
    check(gpu, td, [fd], uks, dev_keys(iks, fixed=28, suffix=8), state, h)   # 28-byte keys, suffix_len = 8
    check(gpu, td, [fd], uks, dev_keys(uks), state, h)                       # variable-length keys
    check(gpu, td, [fd], uks, dev_keys(iks, suffix=8), state, h)
    # the Get's key one byte short of the pair's
    short = [k[:-1] for k in uks]
    want = check(gpu, td, [fd], short, dev_keys(short), state, h)
    assert (want[0][:n] == CORRUPT).all()
    td.close()


def make_end_to_end():
    """4 level-0 files plus two levels with overwrites and deletes, 20,000
    Gets, and the dict model's answers: (files, index blocks, data, user keys,
    snapshot, states, values)."""
    from dlsm_amd import VersionFile

    rng = np.random.default_rng(12)
    universe = 3000
    K = lambda v: b"%020d" % v  # noqa: E731
    model = {}      # user key -> list of (seq, type, value)
    specs = []      # (level, number, lo, hi, first seq): deeper = older
    seq = 1
    for level, number, lo, hi in ((2, 30, 0, 1500), (2, 31, 1500, 3000), (1, 20, 0, 1000), (1, 21, 1000, 3000),
                                  (0, 10, 200, 2500), (0, 11, 0, 1200), (0, 13, 900, 3000), (0, 12, 400, 2000)):
        specs.append((level, number, lo, hi, seq))
        seq += 10_000
    # level-0 files are searched newest (highest number) first: give them sequence numbers in that order
    l0 = sorted([s for s in specs if s[0] == 0], key=lambda s: s[1])
    base = max(s[4] for s in specs if s[0] != 0) + 10_000
    specs = [s for s in specs if s[0] != 0] + [(s[0], s[1], s[2], s[3], base + 10_000 * j) for j, s in enumerate(l0)]
    files, tables, datas = [], [], []
    for level, number, lo, hi, s0 in specs:
        rows = []
        picked = np.sort(rng.choice(np.arange(lo, hi), (hi - lo) // 2, replace=False))
        s = s0
        for v in picked:
            for _ in range(1 + (v % 7 == 0)):       # some keys twice in one file: an overwrite
                s += 1
                typ = 0 if rng.integers(0, 6) == 0 else 1
                val = rng.integers(0, 256, int(rng.integers(0, 120)), dtype=np.uint8).tobytes() if typ else b""
                rows.append((K(v), s, typ, val))
        rows.sort(key=lambda r: (r[0], -r[1]))
        fd = FileData([(ib.internal_key(r[0], r[1], r[2]), r[3]) for r in rows])
        for r in rows:
            model.setdefault(r[0], []).append((r[1], r[2], r[3]))
        datas.append(fd)
        tables.append(ib.build_index_block([ib.internal_key(r[0], r[1], r[2]) for r in rows], fd.handles))
        files.append(VersionFile(level, number, rows[0][0], rows[-1][0], (rows[-1][1] << 8) | rows[-1][2], None))
    snap = base + 10_000 * 3 + 400  # inside the newest level-0 file's sequence numbers
    n = 20_000
    qv = rng.integers(0, universe + 50, n)
    uks = [K(int(v)) for v in qv]
    want_s = np.zeros(n, dtype=np.uint8)
    want_v = []
    for g, k in enumerate(uks):
        vis = [e for e in model.get(k, []) if e[0] <= snap]
        if not vis:
            want_v.append(b"")
            continue
        _, typ, val = max(vis)
        want_s[g] = FOUND if typ else DELETED
        want_v.append(val if typ else b"")
    assert set(want_s.tolist()) == {NOTFOUND, FOUND, DELETED}
    return files, tables, datas, uks, snap, want_s, want_v


def test_end_to_end(gpu):
    """4 level-0 files plus two levels, overwrites and deletes; 20,000 Gets
    through probe -> plan(FIRST) -> seek -> advance to exhaustion, then one
    kv_read_dev, against a dict model of Version::Get: the newest entry at or
    below the snapshot; a deletion means no value."""
    import torch

    files, tables, datas, uks, snap, want_s, want_v = make_end_to_end()
    n = len(uks)
    nf = len(files)
    v = gpu.version(files)
    ti = gpu.tableindex(tables)
    td = gpu.tabledata([d.chunks for d in datas])
    keys = dev_keys(uks, fixed=20)
    mask = torch.zeros(n, dtype=torch.int64, device="cuda")
    lf = torch.zeros((n, 5), dtype=torch.int32, device="cuda")
    gpu.version_probe_dev(v, keys, snap, mask, lf)
    begin = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
    gets = torch.zeros(n, dtype=torch.int32, device="cuda")
    gs = torch.zeros(n, dtype=torch.uint8, device="cuda")
    gh = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
    rounds = 0
    while True:
        gpu.version_read_plan_dev(v, mask, lf, dlsm_amd.PLAN_FIRST, begin, gets)
        gpu.index_seek_dev(ti, keys, snap, begin, gets, get_state=gs, get_handle=gh)
        gpu.version_masks_advance_dev(mask, gs)
        if int(begin[nf].item()) == 0:
            break
        rounds += 1
        assert rounds <= v.n_slots
    total = sum(len(x) for x in want_v)
    vo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    vb = torch.full((total + 64,), VAL_SENT, dtype=torch.uint8, device="cuda")
    nc = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    gpu.kv_read_dev(td, keys, gs, gh, vo, vb, values_cap=total, n_corrupt=nc)
    gpu.sync()
    assert rounds >= 2 and int(nc.item()) == 0
    assert np.array_equal(gs.cpu().numpy(), want_s)
    assert np.array_equal(vo.cpu().numpy(), np.concatenate([[0], np.cumsum([len(x) for x in want_v])]))
    got = vb.cpu().numpy()
    assert np.array_equal(got[:total], np.frombuffer(b"".join(want_v), dtype=np.uint8)) and (got[total:] == VAL_SENT).all()
    no_fallback(gpu)
    td.close()
    ti.close()
    v.close()


def test_host_memory_form(gpu):
    lengths = [5, 0, 70_000, 33, 1]
    rng = np.random.default_rng(13)
    pairs, uks = make_pairs(lengths, rng)
    fd = FileData(pairs)
    td = gpu.tabledata([fd.chunks])
    h = handles_of([(o, s, 0) for o, s in fd.handles])
    h["size"][3] += 1
    state = np.array([FOUND, FOUND, FOUND, FOUND, DELETED], dtype=np.uint8)
    want = expected([fd], uks, state, h, room=sum(lengths))
    k = Keys.pack(uks)
    for vc in (sum(lengths), 100, 0):
        st = state.copy()
        vo, vb, bad = gpu.kv_read(td, k, st, h, values_cap=vc)
        total = int(want[1][5])
        assert np.array_equal(st, want[0][:5]) and np.array_equal(vo, want[1][:6]) and bad == 1
        assert np.array_equal(vb, want[2][:min(total, vc)])
    # the binding's guards: arrays of the wrong dtype or shorter than state are refused before the library reads them
    for bad_args in ((state.astype(np.int32), h, None), (state.copy(), h[:4], None), (state.copy(), h.view(np.uint8), None),
                     (state.copy(), h, np.zeros(5, dtype=np.int64)), (state.copy(), h, np.zeros(4, dtype=np.uint32))):
        with pytest.raises(ValueError):
            gpu.kv_read(td, k, bad_args[0], bad_args[1], gets=bad_args[2], values_cap=8)
    td.close()


def test_launch_times_and_grid(gpu):
    """dlsm_kv_read_stats: the three launches' device times of the last call,
    and a copy grid of two workgroups per compute unit of the device."""
    import torch

    fd, td, uks, h = one_file(gpu, [300] * 2000, 15)
    read(gpu, td, dev_keys(uks), np.full(2000, FOUND, dtype=np.uint8), h, room=600_000)
    ms, wgs = gpu.kv_read_stats()
    assert len(ms) == 3 and all(0 < x < 1000 for x in ms), ms
    assert wgs == 2 * torch.cuda.get_device_properties(0).multi_processor_count
    td.close()


def test_arguments_and_fault_injection(gpu):
    import torch

    lengths = [20, 30]
    fd, td, uks, h = one_file(gpu, lengths, 14)
    keys = dev_keys(uks)
    state = np.full(2, FOUND, dtype=np.uint8)
    st, hd = dev(state), dev(h)
    vo = dev(np.full(3, OFF_SENT, dtype=np.uint64))
    vb = torch.full((128,), VAL_SENT, dtype=torch.uint8, device="cuda")
    with pytest.raises(dlsm_amd.DlsmError):   # a misaligned values_dev
        gpu.kv_read_dev(td, keys, st, hd, vo, vb[1:], values_cap=64)
    with pytest.raises(ValueError):           # missing arrays: the binding's guard (the ABI's: test_kv_read_host.py)
        gpu.kv_read_dev(td, keys, st, hd, None, vb, cap=2, values_cap=64)
    gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 3)
    try:
        with pytest.raises(dlsm_amd.DlsmError) as e:
            gpu.kv_read_dev(td, keys, st, hd, vo, vb)
        assert e.value.status == -3
        with pytest.raises(dlsm_amd.DlsmError):
            gpu.tabledata([fd.chunks])
        with pytest.raises(dlsm_amd.DlsmError):
            gpu.kv_read(td, Keys.pack(uks), state.copy(), h, values_cap=64)
    finally:
        gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 0)
    gpu.sync()
    assert (vo.cpu().numpy().view(np.uint64) == OFF_SENT).all() and (vb.cpu().numpy() == VAL_SENT).all()
    gpu.kv_read_dev(td, keys, st, hd, vo, vb)
    gpu.sync()
    assert vo.cpu().numpy().tolist() == [0, 20, 50]
    td.close()


def test_adapter_table_data_gpu_leg(tmp_path):
    """dlsm_adapter::TableData::ReadBatch on the GPU against its own host path
    (tests/cpp/adapter_kv_test.cc, the program test_kv_read_host.py runs on the CPU)."""
    from test_kv_read_host import compile_adapter_kv_test

    exe = compile_adapter_kv_test(tmp_path)
    out = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK adapter kv gpu" in out.stdout, out.stdout + out.stderr
