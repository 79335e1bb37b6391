"""Read plan of a probed batch (dlsm_version_read_plan_dev): the version probe's
slot masks and level picks grouped by file, as compressed sparse rows over the
caller's file indices, and dlsm_version_masks_advance_dev, which ends a read
round.

The yardstick (``yardstick`` below) restates the contract in numpy: it expands
(mask, level_file) into (Get, file) pairs Get by Get, slot by slot, and sorts
them with a stable sort by file.  It never calls the code under test, so every
comparison is ``array_equal``.  C is the implementation's Gets per
workgroup-chunk; the sizes around it are where the kernels change path.
"""
import ctypes as C_

import numpy as np
import pytest

import oracle
from dlsm_amd import VersionFile
from test_version_probe import K, lookups, make_version

pytestmark = pytest.mark.gpu

FIRST, ALL = 0, 1
SENTINEL = 0xDEADBEEF
NOPICK = 0xFFFFFFFF


def file_tables(files):
    """(level-0 files newest first, per level 1..5 its files in the caller's
    order), each as caller indices -- dlsm_version_create's search order."""
    l0 = [j for j, f in enumerate(files) if f.level == 0]
    l0.sort(key=lambda j: -files[j].number)  # stable: equal numbers keep the caller's order
    lv = [np.array([j for j, f in enumerate(files) if f.level == level], dtype=np.int64) for level in range(1, 6)]
    return np.array(l0, dtype=np.int64), lv


def expand(files, mask, lf, mode):
    """(get, file, slot) of every task, Get by Get, slot by slot."""
    l0, lv = file_tables(files)
    n_l0 = len(l0)
    mask = np.asarray(mask, dtype=np.uint64)
    if mode == FIRST:
        mask = mask & (~mask + np.uint64(1))  # the lowest set bit
    gets, fids, slots = [], [], []
    for s in range(n_l0 + 5):
        g = np.nonzero((mask >> np.uint64(s)) & np.uint64(1))[0]
        if g.size == 0:
            continue
        f = np.full(g.size, l0[s]) if s < n_l0 else lv[s - n_l0][lf[g, s - n_l0].astype(np.int64)]
        gets.append(g)
        fids.append(f)
        slots.append(np.full(g.size, s))
    if not gets:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    gets, fids, slots = np.concatenate(gets), np.concatenate(fids), np.concatenate(slots)
    o = np.lexsort((slots, gets))
    return gets[o], fids[o], slots[o]


def yardstick(files, mask, lf, mode):
    gets, fids, _ = expand(files, mask, lf, mode)
    o = np.argsort(fids, kind="stable")
    begin = np.zeros(len(files) + 1, dtype=np.uint64)
    begin[1:] = np.cumsum(np.bincount(fids, minlength=len(files)))
    return begin, gets[o].astype(np.uint32)


def to_dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint64:
        return torch.from_numpy(a.view(np.int64)).cuda()
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a).cuda()


def plan(gpu, v, n_files, mask_d, lf_d, mode, cap):
    """Runs the plan on device tensors; returns (file_begin, gets[cap + 8], dropped):
    gets is pre-filled with the sentinel, 8 entries longer than cap."""
    import torch

    begin = torch.full((n_files + 1,), -1, dtype=torch.int64, device="cuda")
    gets = torch.full((cap + 8,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    dropped = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    gpu.version_read_plan_dev(v, mask_d, lf_d, mode, begin, gets, dropped, cap=cap)
    gpu.sync()
    return (begin.cpu().numpy().view(np.uint64), gets.cpu().numpy().view(np.uint32),
            int(dropped.cpu().numpy().view(np.uint64)[0]))


def check_plan(gpu, v, files, mask, lf, mode, mask_d=None, lf_d=None):
    want_begin, want_gets = yardstick(files, mask, lf, mode)
    mask_d = to_dev(mask) if mask_d is None else mask_d
    lf_d = to_dev(lf) if lf_d is None else lf_d
    cap = len(mask) if mode == FIRST else max(1, len(want_gets))
    begin, gets, dropped = plan(gpu, v, len(files), mask_d, lf_d, mode, cap)
    assert np.array_equal(begin, want_begin)
    assert np.array_equal(gets[:len(want_gets)], want_gets)
    assert np.all(gets[len(want_gets):] == SENTINEL)
    assert dropped == 0
    return want_begin, want_gets


@pytest.fixture(scope="module")
def chunk():
    import dlsm_amd

    c = dlsm_amd.read_plan_chunk()
    assert c >= 128 and c % 128 == 0
    return c


@pytest.fixture(scope="module")
def probed(gpu, chunk):
    """make_version(0) (31 files, one without a filter), 3C + 3 lookups and the
    oracle's answers; a prefix of the lookups has a prefix of the answers."""
    files = make_version(0)
    assert len(files) == 31 and sum(f.filter is None for f in files) == 1
    n = 3 * chunk + 3
    q = lookups(n, 21)
    snap = 1 << 45
    mask, lf = oracle.version_probe(files, q, n, snap)
    mask.setflags(write=False)
    lf.setflags(write=False)
    v = gpu.version(files)
    yield dict(files=files, n=n, q=q, snap=snap, mask=mask, lf=lf, v=v)
    v.close()


def synth_version(gpu, n_l0, counts, seed):
    """A version without filters: n_l0 level-0 files and counts[level-1] files on
    level 1..5, listed in a shuffled caller order (each level's files keep their
    key order among themselves, as dlsm_version_create asks)."""
    rng = np.random.default_rng(seed)
    t = (1 << 8) | 1
    labels = np.array([0] * n_l0 + [lv + 1 for lv, c in enumerate(counts) for _ in range(c)])
    rng.shuffle(labels)
    nxt = [0] * 6
    numbers = rng.permutation(n_l0) + 100
    vals = np.arange(0, 10 * (max(counts) + 1) + 6, dtype=np.uint64)
    keys = oracle.keys_from_values(vals).reshape(-1, 20)
    files = []
    for lab in labels:
        q = nxt[lab]
        nxt[lab] += 1
        if lab == 0:
            files.append(VersionFile(0, int(numbers[q]), keys[0].tobytes(), keys[-1].tobytes(), t))
        else:
            files.append(VersionFile(int(lab), 1000 + q, keys[10 * q].tobytes(), keys[10 * q + 5].tobytes(), t))
    return files, gpu.version(files)


def synth_answers(n_l0, counts, n, seed, density=0.4):
    """Random consistent masks and picks: a level's bit only with a pick inside
    the level, UINT32_MAX picks where the level has no candidate."""
    rng = np.random.default_rng(seed)
    mask = np.zeros(n, dtype=np.uint64)
    lf = np.full((n, 5), NOPICK, dtype=np.uint32)
    for s in range(n_l0):
        mask |= (rng.random(n) < density).astype(np.uint64) << np.uint64(s)
    for lv, c in enumerate(counts):
        if c == 0:
            continue
        cand = rng.random(n) < 0.8
        lf[cand, lv] = rng.integers(0, c, int(cand.sum()), dtype=np.uint32)
        mask |= (cand & (rng.random(n) < density)).astype(np.uint64) << np.uint64(n_l0 + lv)
    return mask, lf


SHAPES = {  # name -> (n_l0, files on levels 1..5)
    "bins-1": (4, (300, 150, 0, 50, 7)),
    "bins+1": (4, (300, 150, 0, 52, 7)),
    "70001": (1, (60_000, 9_000, 0, 990, 10)),
}


@pytest.fixture(scope="module")
def synth(gpu):
    made = {}

    def get(name):
        if name not in made:
            n_l0, counts = SHAPES[name]
            assert n_l0 + sum(counts) == {"bins-1": 511, "bins+1": 513, "70001": 70_001}[name]
            made[name] = (n_l0, counts) + synth_version(gpu, n_l0, counts, len(made) + 3)
        return made[name]

    yield get
    for _, _, _, v in made.values():
        v.close()


# ---- 1. end to end --------------------------------------------------------------
@pytest.mark.parametrize("mode", [FIRST, ALL])
@pytest.mark.parametrize("size", ["1", "63", "64", "65", "C-1", "C", "C+1", "3C+3"])
def test_plan_end_to_end(gpu, probed, chunk, size, mode):
    n = {"1": 1, "63": 63, "64": 64, "65": 65, "C-1": chunk - 1, "C": chunk, "C+1": chunk + 1,
         "3C+3": 3 * chunk + 3}[size]
    mask, lf = probed["mask"][:n], probed["lf"][:n]
    _, gets = check_plan(gpu, probed["v"], probed["files"], mask, lf, mode)
    if n >= 63:
        assert len(gets) > 0


@pytest.mark.parametrize("mode", [FIRST, ALL])
def test_plan_on_the_gpu_probe_output(gpu, probed, mode):
    """Probe and plan back to back on the device: the plan reads the probe's own
    output buffers (which equal the oracle's)."""
    import torch

    import dlsm_amd

    n = probed["n"]
    mask_d = torch.zeros(n, dtype=torch.int64, device="cuda")
    lf_d = torch.zeros((n, 5), dtype=torch.int32, device="cuda")
    gpu.version_probe_dev(probed["v"], dlsm_amd.Keys(torch.from_numpy(probed["q"]).cuda(), n, 20), probed["snap"],
                          mask_d, lf_d)
    check_plan(gpu, probed["v"], probed["files"], probed["mask"], probed["lf"], mode, mask_d, lf_d)
    assert np.array_equal(mask_d.cpu().numpy().view(np.uint64), probed["mask"])


# ---- 2. synthetic masks ----------------------------------------------------------
def test_plan_all_64_slots(gpu):
    """59 level-0 files + 5 one-file levels: every Get has all 64 slots set."""
    files, v = synth_version(gpu, 59, (1, 1, 1, 1, 1), 11)
    assert v.n_slots == 64
    n = 257
    mask = np.full(n, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    lf = np.zeros((n, 5), dtype=np.uint32)
    begin, gets = check_plan(gpu, v, files, mask, lf, ALL)
    assert len(gets) == 64 * n and np.all(np.diff(begin.astype(np.int64)) == n)
    check_plan(gpu, v, files, mask, lf, FIRST)
    v.close()


@pytest.mark.parametrize("mode", [FIRST, ALL])
@pytest.mark.parametrize("name", ["bins-1", "bins+1", "70001"])
def test_plan_synthetic(gpu, synth, chunk, name, mode):
    """511 files take one digit pass; 513 and 70,001 take two (the intermediate
    pairs, the stable second pass and the bounds search)."""
    n_l0, counts, files, v = synth(name)
    n = 3 * chunk + 3
    mask, lf = synth_answers(n_l0, counts, n, 5)
    begin, gets = check_plan(gpu, v, files, mask, lf, mode)
    assert len(gets) > n // 2
    assert np.count_nonzero(np.diff(begin.astype(np.int64))) > min(len(files), 400) // 2  # many files in use


# ---- 3. skew ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", [FIRST, ALL])
@pytest.mark.parametrize("name", ["bins-1", "bins+1"])
def test_plan_every_get_on_one_file(gpu, synth, chunk, name, mode):
    n_l0, counts, files, v = synth(name)
    n = 3 * chunk + 3
    assert n > 65535  # the one bin's count passes any 16-bit counter
    mask = np.full(n, 1 << n_l0, dtype=np.uint64)  # level 1's slot
    lf = np.full((n, 5), NOPICK, dtype=np.uint32)
    lf[:, 0] = 7
    begin, gets = check_plan(gpu, v, files, mask, lf, mode)
    assert np.array_equal(gets, np.arange(n, dtype=np.uint32))
    assert begin[-1] == n and np.count_nonzero(np.diff(begin.astype(np.int64))) == 1


@pytest.mark.parametrize("mode", [FIRST, ALL])
@pytest.mark.parametrize("name", ["bins-1", "70001"])
def test_plan_empty_and_last_get_only(gpu, synth, chunk, name, mode):
    n_l0, counts, files, v = synth(name)
    n = 3 * chunk + 3
    mask = np.zeros(n, dtype=np.uint64)
    lf = np.full((n, 5), NOPICK, dtype=np.uint32)
    begin, gets = check_plan(gpu, v, files, mask, lf, mode)  # checks that gets still holds the sentinel
    assert begin[-1] == 0 and not begin.any() and len(gets) == 0
    mask[-1] = (1 << 0) | (1 << (n_l0 + 1))  # level-0 file 0 and a level-2 file
    lf[-1, 1] = counts[1] - 1
    begin, gets = check_plan(gpu, v, files, mask, lf, mode)
    assert begin[-1] == (1 if mode == FIRST else 2) and np.all(gets == n - 1)


# ---- 4. capacity ------------------------------------------------------------------
@pytest.mark.parametrize("which", ["total-1", "total/2", "0"])
def test_plan_capacity(gpu, probed, which):
    files, mask, lf = probed["files"], probed["mask"], probed["lf"]
    want_begin, want_gets = yardstick(files, mask, lf, ALL)
    total = len(want_gets)
    assert total > 1000
    cap = {"total-1": total - 1, "total/2": total // 2, "0": 0}[which]
    begin, gets, dropped = plan(gpu, probed["v"], len(files), to_dev(mask), to_dev(lf), ALL, cap)
    assert np.array_equal(begin, want_begin) and begin[-1] == total  # exact whatever cap is
    assert np.array_equal(gets[:cap], want_gets[:cap])
    assert np.all(gets[cap:] == SENTINEL)
    assert dropped == 0


# ---- 5. rounds --------------------------------------------------------------------
def run_rounds(gpu, probed, n, hit_after_first=None):
    """plan(FIRST) + advance until a plan's total is 0; per round the (get, file) pairs."""
    import torch

    files = probed["files"]
    mask_d = to_dev(probed["mask"][:n].copy())
    lf_d = to_dev(probed["lf"][:n])
    zero = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rounds = []
    for r in range(65):
        begin, gets, dropped = plan(gpu, probed["v"], len(files), mask_d, lf_d, FIRST, n)
        total = int(begin[-1])
        assert dropped == 0
        if total == 0:
            break
        fids = np.repeat(np.arange(len(files)), np.diff(begin.astype(np.int64)))
        rounds.append((gets[:total].astype(np.int64), fids))
        hit = zero if (r > 0 or hit_after_first is None) else to_dev(hit_after_first)
        gpu.version_masks_advance_dev(mask_d, hit)
    else:
        pytest.fail("the rounds did not end")
    gpu.sync()
    assert not mask_d.cpu().numpy().any()
    return rounds


def test_plan_rounds(gpu, probed, chunk):
    n = chunk + 1
    files, mask, lf = probed["files"], probed["mask"][:n], probed["lf"][:n]
    g_all, f_all, _ = expand(files, mask, lf, ALL)
    rounds = run_rounds(gpu, probed, n)
    pop = np.array([bin(int(m)).count("1") for m in mask])
    assert len(rounds) == pop.max() and len(rounds) > 1
    # round r of Get i is its r-th set slot: the ALL expansion is Get by Get, slot by slot
    rank = np.arange(len(g_all)) - np.searchsorted(g_all, g_all, side="left")
    for r, (g, f) in enumerate(rounds):
        o = np.argsort(g, kind="stable")
        sel = rank == r
        assert np.array_equal(g[o], g_all[sel]) and np.array_equal(f[o], f_all[sel]), r
    # the union of the rounds is the ALL plan
    want_begin, want_gets = yardstick(files, mask, lf, ALL)
    g = np.concatenate([g for g, _ in rounds])
    f = np.concatenate([f for _, f in rounds])
    o = np.lexsort((g, f))
    assert np.array_equal(g[o].astype(np.uint32), want_gets)
    assert np.array_equal(np.searchsorted(f[o], np.arange(len(files) + 1)).astype(np.uint64), want_begin)


def test_plan_rounds_stop_at_a_hit(gpu, probed, chunk):
    n = chunk + 1
    hit = (np.random.default_rng(8).random(n) < 0.5).astype(np.uint8)
    rounds = run_rounds(gpu, probed, n, hit_after_first=hit)
    later = np.concatenate([g for g, _ in rounds[1:]])
    assert len(later) > 0 and not hit[later].any()
    # the Gets without a hit still visit every one of their files
    g_all, _, _ = expand(probed["files"], probed["mask"][:n], probed["lf"][:n], ALL)
    rest = g_all[hit[g_all] == 0]
    got = np.concatenate([g[hit[g] == 0] for g, _ in rounds])
    assert np.array_equal(np.sort(got), rest)


# ---- 6. arguments -----------------------------------------------------------------
def test_plan_arguments(gpu, probed):
    import torch

    import dlsm_amd

    L = dlsm_amd.lib()
    fb0 = C_.c_uint64(0)
    assert L.dlsm_fallback_stats(gpu.h, C_.byref(fb0), None) == 0
    v, n_files = probed["v"], len(probed["files"])
    n = 100
    mask_d, lf_d = to_dev(probed["mask"][:n]), to_dev(probed["lf"][:n])
    begin = torch.zeros(n_files + 1, dtype=torch.int64, device="cuda")
    gets = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    m, p, b, g = (int(x.data_ptr()) for x in (mask_d, lf_d, begin, gets))

    def call(mask=m, pick=p, n_=n, mode=FIRST, begin_=b, gets_=g, cap=n):
        return L.dlsm_version_read_plan_dev(gpu.h, v.h, mask, pick, n_, mode, begin_, gets_, cap, None)

    assert call() == 0
    assert call(n_=1 << 32) == -1
    assert call(mode=7) == -1 and call(mode=-1) == -1
    assert call(begin_=None) == -1 and call(gets_=None) == -1
    assert call(pick=None) == -1  # the version has files on levels 1-5
    assert L.dlsm_version_read_plan_dev(None, v.h, m, p, n, FIRST, b, g, n, None) == -1
    assert L.dlsm_version_read_plan_dev(gpu.h, None, m, p, n, FIRST, b, g, n, None) == -1
    # n == 0: an all-zero file_begin
    begin.fill_(-1)
    assert call(mask=None, pick=None, n_=0, cap=0, gets_=None) == 0
    gpu.sync()
    assert not begin.cpu().numpy().any()
    # a version with level-0 files only takes a NULL level_file
    t = (1 << 8) | 1
    l0 = [VersionFile(0, 5 + j, K(0), K(100), t) for j in range(3)]
    v0 = gpu.version(l0)
    mk = np.array([0b101, 0, 0b010, 0b111], dtype=np.uint64)
    want_begin, want_gets = yardstick(l0, mk, np.zeros((4, 5), dtype=np.uint32), ALL)
    b0 = torch.zeros(4, dtype=torch.int64, device="cuda")
    g0 = torch.zeros(12, dtype=torch.int32, device="cuda")
    gpu.version_read_plan_dev(v0, to_dev(mk), None, ALL, b0, g0)
    gpu.sync()
    assert np.array_equal(b0.cpu().numpy().view(np.uint64), want_begin)
    assert np.array_equal(g0.cpu().numpy().view(np.uint32)[:len(want_gets)], want_gets)
    v0.close()
    # fault injection answers before anything else runs
    gets.fill_(-1)
    gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 4)
    try:
        assert call() == -4
        assert call(mode=7) == -1  # argument checks come first
        with pytest.raises(dlsm_amd.DlsmError) as e:
            gpu.version_masks_advance_dev(mask_d, torch.zeros(n, dtype=torch.uint8, device="cuda"))
        assert e.value.status == -4
    finally:
        gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 0)
    gpu.sync()
    assert np.all(gets.cpu().numpy() == -1)
    assert np.array_equal(mask_d.cpu().numpy().view(np.uint64), probed["mask"][:n])
    # nothing here was answered by a host fallback
    fb1 = C_.c_uint64(1)
    assert L.dlsm_fallback_stats(gpu.h, C_.byref(fb1), None) == 0
    assert fb1.value == fb0.value
