"""Shard route of a Get batch (dlsm_shard_route_dev): Get_Target_Shard
(db/db_impl_sharding.h:41-55) for every Get of a device batch, each shard's
Gets as one contiguous run that starts at a multiple of 4, the Get indices
ascending, and the keys copied along.

The yardstick restates the contract in Python: ``bisect.bisect_right`` over
Python ``bytes`` (memcmp over the common length, then the shorter first: the
order of Slice::compare) gives the bin, a stable ``argsort`` the runs, and the
padded offsets are a running sum rounded up to 4.  It never calls the code
under test, so every comparison is exact equality over whole buffers, which
are pre-filled with a sentinel: the gaps and everything past the last run must
still hold it.  C is the implementation's Gets per workgroup-chunk; the sizes
around it are where the kernels change path.  DBImpl_Sharding needs the RDMA
Env and cannot run here, so the cases are hand-derived from the cited lines.
"""
import bisect
import ctypes as C_
import random
import subprocess

import numpy as np
import pytest

import oracle
from test_gpu_read_plan import yardstick as plan_yardstick
from test_shard_route_host import compile_adapter_shard_test
from test_version_probe import K, lookups, make_version

pytestmark = pytest.mark.gpu

SENT32 = 0xDEADBEEF
SENT8 = 0xA5


def layout(bins, n_shards):
    """(shard_off, shard_cnt, the Get indices run after run) of the bins."""
    bins = np.asarray(bins, dtype=np.int64)
    cnt = np.bincount(bins, minlength=n_shards + 1).astype(np.uint64)
    off = np.zeros(n_shards + 1, dtype=np.uint64)
    end = 0
    for s in range(n_shards + 1):
        off[s] = (end + 3) & ~3
        end = int(off[s]) + int(cnt[s])
    return off, cnt, np.argsort(bins, kind="stable").astype(np.uint32)


def bins_of(bounds, users):
    assert all(a < b for a, b in zip(bounds, bounds[1:]))
    return np.array([bisect.bisect_right(bounds, k) for k in users], dtype=np.int64)


def expected(bins, n_shards, cap, rows=None):
    """The whole gets buffer (cap + 8 slots) and, with rows ([n, key_len]
    uint8), the whole keys_out buffer."""
    off, cnt, order = layout(bins, n_shards)
    gets = np.full(cap + 8, SENT32, dtype=np.uint32)
    pos = np.concatenate([np.arange(int(off[s]), int(off[s]) + int(cnt[s])) for s in range(n_shards + 1)]
                         + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    gets[pos] = order
    assert int(off[-1]) + int(cnt[-1]) <= cap
    out = None
    if rows is not None:
        out = np.full((cap + 8, rows.shape[1]), SENT8, dtype=np.uint8)
        out[pos] = rows[order]
    return off, cnt, gets, out


def run_route(gpu, m, keys, with_keys=True):
    """Routes device keys; returns (off, cnt, gets[cap + 8], keys_out[(cap + 8), key_len] or None)."""
    import torch

    import dlsm_amd

    cap = dlsm_amd.shard_route_cap(keys.n, m.n_shards)
    off = torch.full((m.n_shards + 1,), -1, dtype=torch.int64, device="cuda")
    cnt = torch.full((m.n_shards + 1,), -1, dtype=torch.int64, device="cuda")
    gets = torch.full((cap + 8,), SENT32 - (1 << 32), dtype=torch.int32, device="cuda")
    out = torch.full(((cap + 8) * keys.key_len,), SENT8, dtype=torch.uint8, device="cuda") if with_keys else None
    gpu.shard_route_dev(m, keys, off, cnt, gets, out, cap=cap)
    gpu.sync()
    return (off.cpu().numpy().view(np.uint64), cnt.cpu().numpy().view(np.uint64), gets.cpu().numpy().view(np.uint32),
            out.cpu().numpy().reshape(cap + 8, keys.key_len) if with_keys else None, cap)


def check_fixed(gpu, bounds, rows, suffix=0, bins=None, data_d=None):
    """rows: [n, key_len] uint8 host keys.  Routes them with and without
    keys_out and compares every buffer with the yardstick."""
    import torch

    import dlsm_amd

    n, kl = rows.shape
    if bins is None:
        bins = bins_of(bounds, [r.tobytes()[:kl - suffix] for r in rows])
    if data_d is None:
        data_d = torch.from_numpy(np.ascontiguousarray(rows).reshape(-1).copy()).cuda()
    keys = dlsm_amd.Keys(data_d, n, kl, None, suffix)
    m = gpu.shardmap(bounds)
    try:
        for with_keys in (True, False):
            off, cnt, gets, out, cap = run_route(gpu, m, keys, with_keys)
            w_off, w_cnt, w_gets, w_out = expected(bins, len(bounds), cap, rows if with_keys else None)
            assert np.array_equal(cnt, w_cnt)
            assert np.array_equal(off, w_off) and np.all(off % 4 == 0)
            assert np.array_equal(gets, w_gets)
            if with_keys:
                assert np.array_equal(out, w_out)
    finally:
        m.close()
    return bins


def check_var(gpu, bounds, keys_list):
    """Variable-length keys: the indices only."""
    import torch

    import dlsm_amd

    data, offs = oracle.pack_var(keys_list)
    keys = dlsm_amd.Keys(torch.from_numpy(data).cuda(), len(keys_list), 0,
                         torch.from_numpy(offs.view(np.int64)).cuda())
    m = gpu.shardmap(bounds)
    try:
        off, cnt, gets, _, cap = run_route(gpu, m, keys, with_keys=False)
        w_off, w_cnt, w_gets, _ = expected(bins_of(bounds, keys_list), len(bounds), cap)
        assert np.array_equal(cnt, w_cnt) and np.array_equal(off, w_off) and np.array_equal(gets, w_gets)
        # keys_out with offsets is refused, and nothing is written
        out = torch.full((cap * 8,), SENT8, dtype=torch.uint8, device="cuda")
        with pytest.raises(dlsm_amd.DlsmError) as e:
            gpu.shard_route_dev(m, keys, torch.zeros(len(bounds) + 1, dtype=torch.int64, device="cuda"),
                                torch.zeros(len(bounds) + 1, dtype=torch.int64, device="cuda"),
                                torch.zeros(cap, dtype=torch.int32, device="cuda"), out, cap=cap)
        assert e.value.status == -1
    finally:
        m.close()


@pytest.fixture(autouse=True)
def no_host_fallback(gpu):
    """Nothing in these tests is answered by a host fallback."""
    import dlsm_amd

    L = dlsm_amd.lib()
    a, b = C_.c_uint64(0), C_.c_uint64(0)
    assert L.dlsm_fallback_stats(gpu.h, C_.byref(a), None) == 0
    yield
    assert L.dlsm_fallback_stats(gpu.h, C_.byref(b), None) == 0
    assert a.value == b.value == 0


@pytest.fixture(scope="module")
def chunk():
    import dlsm_amd

    c = dlsm_amd.shard_route_chunk()
    assert c >= 64 and c % 64 == 0
    return c


SPAN = 1_000_000
SHARDS = (1, 2, 16, 511)


def split_bounds(ns):
    """ns equal shards of [0, SPAN): shard s ends at the db_bench key of (s + 1) * SPAN // ns."""
    return [(s + 1) * SPAN // ns for s in range(ns)]


@pytest.fixture(scope="module")
def batch(chunk):
    """3C + 3 db_bench-shaped 20-byte lookups over [0, 1.1 SPAN) -- a tenth lie
    past the last bound -- with every 97th replaced by a shard bound of the 16-
    or 511-way split (the tie path of fixed keys), their rows, and per shard
    count the yardstick's bins.  Read-only."""
    n = 3 * chunk + 3
    rng = np.random.default_rng(17)
    v = rng.integers(0, SPAN + SPAN // 10, n).astype(np.uint64)
    ties = np.array(split_bounds(16) + split_bounds(511), dtype=np.uint64)
    v[::97] = ties[rng.integers(0, len(ties), len(v[::97]))]
    v[0], v[1] = 0, SPAN
    rows = oracle.keys_from_values(v).reshape(n, 20)
    users = [r.tobytes() for r in rows]
    bins = {}
    for ns in SHARDS:
        bounds = [K(b) for b in split_bounds(ns)]
        bins[ns] = bins_of(bounds, users)
        bins[ns].setflags(write=False)
        # the values order as the keys do: a second statement of the same bins
        assert np.array_equal(bins[ns], np.searchsorted(np.array(split_bounds(ns), dtype=np.uint64), v, side="right"))
    v.setflags(write=False)
    rows.setflags(write=False)
    return dict(n=n, v=v, rows=rows, bins=bins)


@pytest.mark.parametrize("ns", SHARDS)
@pytest.mark.parametrize("size", ["0", "1", "63", "64", "65", "C-1", "C", "C+1", "3*C+3"])
def test_sizes_and_shard_counts(gpu, chunk, batch, size, ns):
    n = eval(size, {"C": chunk})
    bounds = [K(b) for b in split_bounds(ns)]
    check_fixed(gpu, bounds, batch["rows"][:n], bins=batch["bins"][ns][:n])


def test_distributions(gpu, chunk):
    ns = 16
    edges = [0] + split_bounds(ns)
    bounds = [K(b) for b in edges[1:]]
    rng = np.random.default_rng(5)
    n = chunk + 65

    def rows_in(shards):
        s = rng.choice(shards, n)
        v = np.array([rng.integers(edges[q], edges[q + 1]) for q in s], dtype=np.uint64)
        return oracle.keys_from_values(v).reshape(n, 20)

    b = check_fixed(gpu, bounds, rows_in([5]))                    # all Gets in one shard
    assert np.all(b == 5)
    past = oracle.keys_from_values(rng.integers(SPAN, 2 * SPAN, n).astype(np.uint64)).reshape(n, 20)
    b = check_fixed(gpu, bounds, past)                            # all Gets past the last bound
    assert np.all(b == ns)
    b = check_fixed(gpu, bounds, rows_in([0, 7, 15]))             # empty shards between full ones
    assert set(b.tolist()) == {0, 7, 15}
    one = np.array([edges[q] + 3 for q in rng.permutation(ns)], dtype=np.uint64)
    b = check_fixed(gpu, bounds, oracle.keys_from_values(one).reshape(ns, 20))  # one Get per shard
    assert sorted(b.tolist()) == list(range(ns))


def test_internal_keys_bin_by_user_key(gpu, chunk, batch):
    """28-byte internal keys, suffix_len 8: the bin comes from the user key and
    the 8-byte trailer travels with it (trailers of 0xff bytes would move keys
    that equal a bound if they were compared)."""
    n = chunk + 65
    rng = np.random.default_rng(9)
    rows = np.concatenate([batch["rows"][:n], rng.integers(0xF0, 0x100, (n, 8)).astype(np.uint8)], axis=1)
    bounds = [K(b) for b in split_bounds(16)]
    bins = check_fixed(gpu, bounds, rows, suffix=8)
    assert np.array_equal(bins, batch["bins"][16][:n])


@pytest.mark.parametrize("key_len", [16, 33, 36])
def test_other_fixed_lengths(gpu, chunk, key_len):
    """16 bytes (whole 16-byte prefix, nothing after it), 33 bytes (the byte
    path) and 36 bytes (whole dwords, too long for the staged path)."""
    n = chunk + 65
    rng = np.random.default_rng(key_len)
    v = rng.integers(0, SPAN + SPAN // 10, n).astype(np.uint64)
    v[::50] = np.array(split_bounds(16), dtype=np.uint64)[rng.integers(0, 16, len(v[::50]))]
    rows = oracle.keys_from_values(v, key_len).reshape(n, key_len)
    bounds = [oracle.keys_from_values(np.array([b], dtype=np.uint64), key_len).tobytes() for b in split_bounds(16)]
    bins = check_fixed(gpu, bounds, rows)
    assert np.array_equal(bins, np.searchsorted(np.array(split_bounds(16), dtype=np.uint64), v, side="right"))


def test_input_base_not_16_byte_aligned(gpu, chunk, batch):
    import torch

    n = chunk + 65
    rows = batch["rows"][:n]
    buf = torch.zeros(n * 20 + 4, dtype=torch.uint8, device="cuda")
    buf[4:] = torch.from_numpy(np.ascontiguousarray(rows).reshape(-1).copy()).cuda()
    view = buf[4:]
    assert view.data_ptr() % 16 == 4
    check_fixed(gpu, [K(b) for b in split_bounds(16)], rows, bins=batch["bins"][16][:n], data_d=view)


def crowded(want, seed):
    """Random bounds that crowd a few 16-byte prefixes (the CPU test's recipe)."""
    rng = random.Random(seed)
    pre = [bytes(16), b"0000000000000042", b"\x80" * 15 + b"\xff", b"\xff" * 16]
    out = set()
    while len(out) < want:
        k = rng.choice(pre)
        if rng.randrange(8) == 0:
            k = k[:rng.randrange(17)]
        else:
            k += bytes(rng.choice(b"\x00a\x80\xff") for _ in range(rng.randrange(7)))
        out.add(k)
    return sorted(out)


def adversarial_bounds():
    P = b"p" * 16
    return [
        [P, P + b"\0", P + b"\0\0", P + b"a", P + b"ab", P + b"\x80", P + b"\xff"],   # share 16 bytes, differ after
        [b"", b"k", b"k" * 15, b"k" * 16, b"k" * 17, b"k" * 40],                     # 0, 1, 15, 16, 17, 40 bytes
        [b"\0", b"\0\0", b"\0\1", b"a\0", b"a\0\0", b"a\0b", b"\x7f", b"\x80", b"\x80\0", b"\xff", b"\xff\xff"],
        [b"m"],
        [b"g" * 20, b"t" * 20],
        crowded(255, 7),
        crowded(511, 11),
    ]


def adversarial_lookups(bounds):
    keys = []
    for b in bounds:
        keys += [b, b + b"\0", b + b"\xff"]
        if b:
            keys += [b[:-1], b[:-1] + bytes([(b[-1] + 1) & 255])]
        keys += [b[:7], b[:15]]                                  # shorter than 16 bytes
        if len(b) >= 16:
            keys += [b[:16], b[:16] + b"\x01", b[:16] + b"\xfe\xfe"]  # share the bound's 16-byte prefix
    keys += [b"", bounds[-1] + b"\xff\xff", b"\xff" * 41]
    return keys


@pytest.mark.parametrize("which", range(7))
def test_tie_path(gpu, which):
    bounds = adversarial_bounds()[which]
    check_var(gpu, bounds, adversarial_lookups(bounds))


def test_variable_length_keys(gpu, chunk):
    """0 to 40 bytes over a small alphabet, so that many keys are prefixes of
    bounds and of each other; more than one chunk."""
    rng = random.Random(3)
    mk = lambda: bytes(rng.choice(b"\x00ab\xff") for _ in range(rng.randrange(41)))  # noqa: E731
    bounds = sorted({mk() for _ in range(40)} - {b""})
    keys = [mk() for _ in range(chunk + 65)]
    keys[::31] = [rng.choice(bounds) for _ in keys[::31]]
    check_var(gpu, bounds, keys)


def test_past_the_workgroup_cap(gpu, chunk):
    """More chunks than workgroups (512): several chunks per workgroup.  The
    yardstick is np.searchsorted over the 64-bit values (db_bench keys order as
    their values do); the keys' copies are compared on the device."""
    import torch

    import dlsm_amd

    ns = 16
    n = 512 * chunk + chunk + 77
    rng = np.random.default_rng(23)
    v = rng.integers(0, SPAN + SPAN // 10, n).astype(np.uint64)
    edges = np.array(split_bounds(ns), dtype=np.uint64)
    bins = np.searchsorted(edges, v, side="right")
    keys_d = torch.from_numpy(oracle.keys_from_values(v)).cuda()
    m = gpu.shardmap([K(b) for b in split_bounds(ns)])
    try:
        cap = dlsm_amd.shard_route_cap(n, ns)
        off = torch.full((ns + 1,), -1, dtype=torch.int64, device="cuda")
        cnt = torch.full((ns + 1,), -1, dtype=torch.int64, device="cuda")
        gets = torch.full((cap + 8,), SENT32 - (1 << 32), dtype=torch.int32, device="cuda")
        out = torch.full(((cap + 8) * 20,), SENT8, dtype=torch.uint8, device="cuda")
        gpu.shard_route_dev(m, dlsm_amd.Keys(keys_d, n, 20), off, cnt, gets, out, cap=cap)
        gpu.sync()
        w_off, w_cnt, w_gets, _ = expected(bins, ns, cap)
        assert np.array_equal(off.cpu().numpy().view(np.uint64), w_off)
        assert np.array_equal(cnt.cpu().numpy().view(np.uint64), w_cnt)
        assert np.array_equal(gets.cpu().numpy().view(np.uint32), w_gets)
        w = torch.from_numpy(w_gets.astype(np.int64)).cuda()
        run = w != SENT32
        rows = out.view(cap + 8, 20)
        assert torch.equal(rows[run], keys_d.view(n, 20)[w[run]])
        assert bool((rows[~run] == SENT8).all())
    finally:
        m.close()


def test_two_runs_are_identical(gpu, chunk, batch):
    import torch

    import dlsm_amd

    n = batch["n"]
    keys = dlsm_amd.Keys(torch.from_numpy(batch["rows"].reshape(-1).copy()).cuda(), n, 20)
    m = gpu.shardmap([K(b) for b in split_bounds(511)])
    try:
        a = run_route(gpu, m, keys)
        b = run_route(gpu, m, keys)
        for x, y in zip(a[:4], b[:4]):
            assert np.array_equal(x, y)
    finally:
        m.close()


def test_fault_injection_and_argument_checks(gpu, chunk, batch):
    import torch

    import dlsm_amd

    L = dlsm_amd.lib()
    n, ns = chunk + 1, 16
    keys_t = torch.from_numpy(batch["rows"][:n].reshape(-1).copy()).cuda()
    ks = dlsm_amd.Keys(keys_t, n, 20).c()
    m = gpu.shardmap([K(b) for b in split_bounds(ns)])
    try:
        cap = dlsm_amd.shard_route_cap(n, ns)
        off = torch.full((ns + 1,), -1, dtype=torch.int64, device="cuda")
        cnt = torch.full((ns + 1,), -1, dtype=torch.int64, device="cuda")
        gets = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
        out = torch.full((cap * 20,), SENT8, dtype=torch.uint8, device="cuda")

        def call(cap_=cap, off_=off, map_=m.h, keys_=ks):
            return L.dlsm_shard_route_dev(gpu.h, map_, C_.byref(keys_), off_.data_ptr() if off_ is not None else None,
                                          cnt.data_ptr(), gets.data_ptr(), out.data_ptr(), cap_)

        big = dlsm_amd.dlsm_keyset(ks.bytes, None, 20, 0, 1 << 32)
        gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 4)
        try:
            assert call() == -4
            assert call(cap_=cap - 1) == -1       # argument checks come first
            assert call(off_=None) == -1
            assert call(map_=None) == -1
            assert call(keys_=big) == -1          # n > UINT32_MAX
        finally:
            gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 0)
        assert call(cap_=cap - 1) == -1
        gpu.sync()
        assert np.all(gets.cpu().numpy() == -1) and np.all(out.cpu().numpy() == SENT8)
        assert np.all(off.cpu().numpy() == -1) and np.all(cnt.cpu().numpy() == -1)
        assert m.n_shards == ns
        k = C_.c_int(0)
        assert L.dlsm_shardmap_size(m.h, C_.byref(k)) == 0 and k.value == ns
        # bounds out of order, with a live context
        with pytest.raises(dlsm_amd.DlsmError) as e:
            gpu.shardmap([b"b", b"a"])
        assert e.value.status == -1
        with pytest.raises(dlsm_amd.DlsmError):
            gpu.shardmap([])
        # an empty first bound is legal: shard 0 then holds nothing
        rows = batch["rows"][:100]
        bins = check_fixed(gpu, [b"", K(SPAN // 2)], rows)
        assert 0 not in bins.tolist() and 1 in bins.tolist()
    finally:
        m.close()


def test_adapter_route_equals_its_host_fallback(tmp_path):
    exe = compile_adapter_shard_test(tmp_path)
    out = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "OK adapter shard gpu" in out.stdout, out.stdout + out.stderr


def test_composition_with_probe_and_plan(gpu, chunk):
    """Three shards over disjoint key ranges, each with its own version.  Route
    3C + 3 lookups, then per shard: probe keys_out's run against the shard's
    version, equal to the oracle's answer on the lookups the yardstick gave that
    shard; a FIRST plan's Get indices, mapped through gets, name the caller's
    Gets."""
    import torch

    import dlsm_amd

    edges = [400_000, 800_000, 1_200_000]
    bounds = [K(b) for b in edges]
    n = 3 * chunk + 3
    q = lookups(n, 33)
    rows = q.reshape(n, 20)
    bins = bins_of(bounds, [r.tobytes() for r in rows])
    assert set(bins.tolist()) == {0, 1, 2, 3}  # lookups() ends with 2,000,000: past the last bound
    snap = 1 << 45
    versions = [make_version(10 + s) for s in range(3)]
    m = gpu.shardmap(bounds)
    vs = [gpu.version(f) for f in versions]
    try:
        keys = dlsm_amd.Keys(torch.from_numpy(q.copy()).cuda(), n, 20)
        cap = dlsm_amd.shard_route_cap(n, 3)
        off_d = torch.zeros(4, dtype=torch.int64, device="cuda")
        cnt_d = torch.zeros(4, dtype=torch.int64, device="cuda")
        gets_d = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
        out_d = torch.zeros(cap * 20, dtype=torch.uint8, device="cuda")
        gpu.shard_route_dev(m, keys, off_d, cnt_d, gets_d, out_d)
        gpu.sync()
        off, cnt = off_d.cpu().numpy(), cnt_d.cpu().numpy()
        gets = gets_d.cpu().numpy().view(np.uint32)
        for s in range(3):
            mine = np.nonzero(bins == s)[0]          # the yardstick's Gets of shard s, ascending
            ns = len(mine)
            assert ns > 0 and cnt[s] == ns
            run = out_d[int(off[s]) * 20:(int(off[s]) + ns) * 20]
            assert run.data_ptr() % 16 == 0          # an aligned keyset: the probe's staged loaders take it
            slot = torch.zeros(ns, dtype=torch.int64, device="cuda")
            lf = torch.zeros((ns, 5), dtype=torch.int32, device="cuda")
            gpu.version_probe_dev(vs[s], dlsm_amd.Keys(run, ns, 20), snap, slot, lf)
            begin = torch.zeros(len(versions[s]) + 1, dtype=torch.int64, device="cuda")
            pg = torch.full((ns,), -1, dtype=torch.int32, device="cuda")
            gpu.version_read_plan_dev(vs[s], slot, lf, dlsm_amd.PLAN_FIRST, begin, pg)
            gpu.sync()
            w_mask, w_lf = oracle.version_probe(versions[s], np.ascontiguousarray(rows[mine]).reshape(-1), ns, snap)
            assert np.array_equal(slot.cpu().numpy().view(np.uint64), np.asarray(w_mask, dtype=np.uint64))
            assert np.array_equal(lf.cpu().numpy().view(np.uint32), w_lf)
            w_begin, w_pg = plan_yardstick(versions[s], w_mask, w_lf, 0)
            total = int(w_begin[-1])
            assert total > 0
            assert np.array_equal(begin.cpu().numpy().view(np.uint64), w_begin)
            local = pg.cpu().numpy().view(np.uint32)[:total]
            assert np.array_equal(local, w_pg)
            # local Get g of shard s is the caller's Get gets[shard_off[s] + g]
            assert np.array_equal(gets[int(off[s]) + local.astype(np.int64)], mine[w_pg.astype(np.int64)])
    finally:
        for v in vs:
            v.close()
        m.close()
