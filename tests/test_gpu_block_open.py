"""Sealed filter blocks, read side (block_ingest.hip): ReadFilterBlock's
checks (table/format.cc:380-444) on the GPU for n ragged blocks in two
launches, and filter sets / versions opened straight from the blocks.

A block is `[contents][type 0][Fixed32(Mask(crc32c(contents || type)))]`; the
oracle seals arbitrary bytes (``orc.filter_block``).  The kernel cuts the crc'd
stream (contents + type byte) into 16-byte pieces from its start, 256 pieces
per pass (4 KiB), 8 passes per part (32 KiB), and front-pads to whole parts, so
the lengths below sit around 16, 4,096 and 32,768 stream bytes and reach two,
three and five parts; the < 16 bytes behind the last piece are appended by the
finish kernel.  A single-byte change is always caught by crc32c, so every
corruption case asserts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, SHORT, CHECKSUM, TYPE, FILTER = 0, 1, 2, 3, 4
PASS, PART = 4096, 32768  # stream bytes per pass / part of ingest_parts_kernel


def _content_lengths():
    ns = set(range(0, 301))
    for base in (1 << 10, 16 << 10, 64 << 10, 128 << 10, PASS, PART, 2 * PART):
        for d in (-1, 0, 1, 5, 6, 15, 16, 17):
            ns.add(base + d)
        for d in (-18, -17, -16, -2):  # the stream is one byte longer than the contents
            ns.add(base + d)
    return sorted(ns)


@pytest.fixture(scope="module")
def sealed(orc):
    """Random contents of every length under test, sealed by the oracle."""
    rng = np.random.default_rng(42)
    return {n: orc.filter_block(rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for n in _content_lengths()}


def _device_blocks(blocks, shift=0):
    """The blocks in one device buffer, each `shift` bytes past a 256-byte
    boundary; returns views (uint8 tensors) that keep the buffer alive."""
    import torch

    offs, total = [], 0
    for b in blocks:
        offs.append(total + shift)
        total += (len(b) + shift + 255) // 256 * 256
    host = np.zeros(total + 256, dtype=np.uint8)
    for b, o in zip(blocks, offs):
        host[o: o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 256 == 0
    return [dev[o: o + len(b)] for b, o in zip(blocks, offs)]


def _flip(block, idx):
    b = bytearray(block)
    b[idx] ^= 0x5A
    return bytes(b)


def _corruptions(n):
    """Byte indices of a block of n content bytes to flip, one at a time."""
    stream = n + 1
    body = stream // 16 * 16  # the 16-byte pieces end here
    idx = {n, n + 1, n + 2, n + 3, n + 4}  # the type byte and each crc byte
    if n:
        idx.add(0)
    if body:
        idx.add(body - 1)
    if body < stream:
        idx.add(body)  # a byte of the tail (the type byte when the tail is 1 byte)
    for b in range(body - PART, 0, -PART):  # part boundaries of the front-padded stream
        idx |= {b - 1, b}
    for b in range(body - PASS, 0, -8 * PASS):  # and one pass boundary per part
        idx |= {b - 1, b}
    return sorted(idx)


def test_lengths_host_and_device(gpu, sealed):
    ns = _content_lengths()
    blocks = [sealed[n] for n in ns]
    got = gpu.blocks_check(blocks)
    assert got.dtype == np.uint8 and got.tolist() == [OK] * len(ns), [n for n, s in zip(ns, got) if s]
    dev = _device_blocks(blocks)
    got = gpu.blocks_check(dev, on_device=True)
    assert got.tolist() == [OK] * len(ns), [n for n, s in zip(ns, got) if s]
    assert gpu.blocks_check([]).size == 0


def test_short_blocks(gpu, sealed):
    blocks = [sealed[7][:m] for m in range(5)] + [sealed[7]]
    for verify in (True, False):
        assert gpu.blocks_check(blocks, verify_checksums=verify).tolist() == [SHORT] * 5 + [OK]
        assert gpu.blocks_check(_device_blocks(blocks), on_device=True,
                                verify_checksums=verify).tolist() == [SHORT] * 5 + [OK]


CORRUPT_NS = [0, 1, 14, 15, 16, 17, 30, 31, 32, 300, PASS - 2, PASS - 1, PASS, PASS + 15, PART - 17, PART - 2,
              PART - 1, PART, PART + 1, PART + 16, 2 * PART - 1, 2 * PART + 17, (64 << 10) + 5, (128 << 10) + 6]


@pytest.mark.parametrize("on_device", [False, True])
def test_single_byte_corruption(gpu, sealed, on_device):
    blocks, want_v, want_nv = [], [], []
    for n in CORRUPT_NS:
        for i in _corruptions(n):
            blocks.append(_flip(sealed[n], i))
            want_v.append(CHECKSUM)
            want_nv.append(TYPE if i == n else OK)
        blocks.append(sealed[n])  # an intact neighbour
        want_v.append(OK)
        want_nv.append(OK)
    src = _device_blocks(blocks) if on_device else blocks
    got = gpu.blocks_check(src, on_device=on_device, verify_checksums=True)
    assert got.tolist() == want_v
    got = gpu.blocks_check(src, on_device=on_device, verify_checksums=False)
    assert got.tolist() == want_nv


@pytest.mark.parametrize("shift", [1, 3, 8, 15])
def test_unaligned_device_blocks(gpu, sealed, shift):
    ns = [0, 1, 15, 16, 17, 47, 300, PASS - 1, PASS + 1, PART - 1, PART, PART + 16, (64 << 10) + 5]
    blocks, want = [], []
    for n in ns:
        blocks += [sealed[n], _flip(sealed[n], n // 2), _flip(sealed[n], n)]
        want += [OK, CHECKSUM, CHECKSUM]
    dev = _device_blocks(blocks, shift)
    assert all(d.data_ptr() % 16 == shift for d in dev)
    assert gpu.blocks_check(dev, on_device=True).tolist() == want
    assert gpu.blocks_check(_device_blocks(blocks), on_device=True).tolist() == want


# ---- filter sets and versions opened from blocks ---------------------------

SET_SHAPES = [(n, bpk) for bpk in (10, 16) for n in (1, 7, 5_000, 20_000, 153_846)]


@pytest.fixture(scope="module")
def filters(orc):
    keys = [orc.dbbench_keys(3 + j, 5, n) for j, (n, _) in enumerate(SET_SHAPES)]
    filt = [orc.full_build(k, n, bpk=bpk) for k, (n, bpk) in zip(keys, SET_SHAPES)]
    nq = 200_003
    q = orc.keys_from_values(orc.mt_values(77, 5 * 153_846, nq))
    return {"keys": keys, "filters": filt, "blocks": [orc.filter_block(f) for f in filt], "q": q, "nq": nq,
            "want": orc.full_probe(filt, q, nq, nthreads=4)}


def test_filterset_parity(gpu, orc, filters):
    import torch

    import dlsm_amd

    q = dlsm_amd.Keys(filters["q"], filters["nq"], 20)
    blocks = filters["blocks"]
    ref = gpu.filterset(filters["filters"])
    want = gpu.full_probe(ref, q)
    assert np.array_equal(want, filters["want"])
    ref.close()
    # straight from the sealed build's device slots
    built = []
    for bpk in (10, 16):
        idx = [j for j, s in enumerate(SET_SHAPES) if s[1] == bpk]
        tabs = [dlsm_amd.Keys(torch.from_numpy(filters["keys"][j]).cuda(), SET_SHAPES[j][0], 20) for j in idx]
        outs = [torch.zeros(len(blocks[j]) + 32, dtype=torch.uint8, device="cuda") for j in idx]
        lens = torch.zeros(len(idx), dtype=torch.uint64, device="cuda")
        gpu.full_build_block_dev(tabs, outs, lens, bpk)
        gpu.sync()
        for o, n, j in zip(outs, lens.cpu().numpy(), idx):
            assert int(n) == len(blocks[j])
            built.append(o[: int(n)])
    for src, dev in ((blocks, False), (_device_blocks(blocks), True), (built, True)):
        fs = gpu.filterset(src, on_device=dev, sealed=True)
        assert fs.n_filters == len(blocks)
        assert np.array_equal(gpu.full_probe(fs, q), want)
        fs.close()
    fs = gpu.filterset(_device_blocks(blocks, 3), on_device=True, sealed=True, verify_checksums=False)
    assert np.array_equal(gpu.full_probe(fs, q), want)
    fs.close()


def test_filterset_rejects_bad_blocks(gpu, orc, filters):
    import dlsm_amd

    blocks = list(filters["blocks"][:5])
    empty = orc.filter_block(orc.full_build(np.zeros(20, np.uint8), 0))
    assert len(empty) == 10
    bad = blocks[:]
    bad[1] = _flip(bad[1], 10)            # contents
    bad[3] = _flip(bad[3], len(bad[3]) - 5)  # type byte
    bad.append(empty)                     # the 0-key filter: sealed correctly, unusable
    bad.append(empty[:3])
    for dev in (False, True):
        src = _device_blocks(bad) if dev else bad
        with pytest.raises(dlsm_amd.DlsmError) as e:
            gpu.filterset(src, on_device=dev, sealed=True)
        assert isinstance(e.value, dlsm_amd.BlockError) and e.value.status == -3
        assert e.value.block_status.tolist() == [OK, CHECKSUM, OK, CHECKSUM, OK, FILTER, SHORT]
        with pytest.raises(dlsm_amd.BlockError) as e:
            gpu.filterset(src, on_device=dev, sealed=True, verify_checksums=False)
        assert e.value.block_status.tolist() == [OK, OK, OK, TYPE, OK, FILTER, SHORT]
    # the context still builds and probes
    q = dlsm_amd.Keys(filters["q"], filters["nq"], 20)
    k = filters["keys"][2]
    got = gpu.full_build_block([dlsm_amd.Keys(k, 5_000, 20)], 10)
    assert got[0] == blocks[2]
    fs = gpu.filterset(blocks, sealed=True)
    assert np.array_equal(gpu.full_probe(fs, q), orc.full_probe(filters["filters"][:5], filters["q"], filters["nq"]))
    fs.close()


def _seal_files(orc, files, on_device):
    import torch

    from dlsm_amd import VersionFile

    out = []
    for f in files:
        blk = None if f.filter is None else orc.filter_block(f.filter)
        if blk is not None and on_device:
            blk = torch.frombuffer(bytearray(blk), dtype=torch.uint8).cuda()
        out.append(VersionFile(f.level, f.number, f.smallest, f.largest, f.largest_trailer, blk))
    return out


@pytest.fixture(scope="module")
def version0(orc):
    from test_version_probe import lookups, make_version

    files = make_version(0)
    n = 200_003
    q = lookups(n, 9)
    want = {s: orc.version_probe(files, q, n, s) for s in (1 << 45, 1 << 20)}
    return files, q, n, want


@pytest.mark.parametrize("snapshot", [1 << 45, 1 << 20])
@pytest.mark.parametrize("on_device", [False, True])
def test_version_parity(gpu, orc, version0, snapshot, on_device):
    import torch

    import dlsm_amd

    files, q, n, want = version0
    assert any(f.filter is None for f in files)
    v = gpu.version(_seal_files(orc, files, on_device), on_device=on_device, sealed=True)
    assert v.n_l0 == 4 and v.n_slots == 9
    mask = torch.zeros(n, dtype=torch.uint64, device="cuda")
    lf = torch.zeros((n, 5), dtype=torch.int32, device="cuda")
    gpu.version_probe_dev(v, dlsm_amd.Keys(torch.from_numpy(q).cuda(), n, 20), snapshot, mask, lf)
    gpu.sync()
    assert np.array_equal(mask.cpu().numpy().view(np.uint64), want[snapshot][0])
    assert np.array_equal(lf.cpu().numpy().view(np.uint32), want[snapshot][1])
    v.close()


@pytest.mark.parametrize("on_device", [False, True])
def test_version_rejects_bad_blocks(gpu, orc, version0, on_device):
    import torch

    import dlsm_amd
    from dlsm_amd import VersionFile

    files, q, n, want = version0
    sealed_files = _seal_files(orc, files, False)
    bad = {2: CHECKSUM, 9: CHECKSUM, 20: TYPE}  # a level-0 file (search order differs from the caller's) and two deeper
    broken = []
    for j, f in enumerate(sealed_files):
        blk = f.filter
        if j in bad:
            blk = _flip(blk, 17 if bad[j] == CHECKSUM else len(blk) - 5)
        if blk is not None and on_device:
            blk = torch.frombuffer(bytearray(blk), dtype=torch.uint8).cuda()
        broken.append(VersionFile(f.level, f.number, f.smallest, f.largest, f.largest_trailer, blk))
    with pytest.raises(dlsm_amd.DlsmError) as e:
        gpu.version(broken, on_device=on_device, sealed=True)
    assert isinstance(e.value, dlsm_amd.BlockError)
    assert e.value.block_status.tolist() == [CHECKSUM if j in bad else OK for j in range(len(files))]
    with pytest.raises(dlsm_amd.BlockError) as e:
        gpu.version(broken, on_device=on_device, sealed=True, verify_checksums=False)
    assert e.value.block_status.tolist() == [TYPE if bad.get(j) == TYPE else OK for j in range(len(files))]
    # the context opens and probes the intact version afterwards
    v = gpu.version(sealed_files, sealed=True)
    mask = torch.zeros(n, dtype=torch.uint64, device="cuda")
    gpu.version_probe_dev(v, dlsm_amd.Keys(torch.from_numpy(q).cuda(), n, 20), 1 << 45, mask)
    gpu.sync()
    assert np.array_equal(mask.cpu().numpy().view(np.uint64), want[1 << 45][0])
    v.close()


def test_version_of_70000_files(gpu, orc):
    """More blocks than a grid's y dimension holds (65,535): 70,000 one-line
    filters (74-byte blocks) and one larger level-0 file, device resident."""
    import torch

    import dlsm_amd
    from dlsm_amd import VersionFile
    from test_version_probe import K, build_filter

    nf = 70_000
    filt = [build_filter(np.array([10 * q, 10 * q + 3])) for q in range(nf)]
    filt.append(build_filter(np.arange(0, 10 * nf, 7)))
    meta = [(1, 10 + q, K(10 * q), K(10 * q + 5), ((q + 1) << 8) | 1) for q in range(nf)]
    meta.append((0, 5, K(0), K(10 * nf), (1 << 40 << 8) | 1))
    blocks = [orc.filter_block(f) for f in filt]
    assert len(blocks[0]) == 74
    dev = _device_blocks(blocks)
    n = 20_000
    q = orc.keys_from_values(np.random.default_rng(3).integers(0, 10 * nf + 100, n).astype(np.uint64))
    snap = (1 << 56) - 1
    want, want_lf = orc.version_probe([VersionFile(*m, f) for m, f in zip(meta, filt)], q, n, snapshot=snap)
    v = gpu.version([VersionFile(*m, d) for m, d in zip(meta, dev)], on_device=True, sealed=True)
    mask = torch.zeros(n, dtype=torch.uint64, device="cuda")
    lf = torch.zeros((n, 5), dtype=torch.int32, device="cuda")
    gpu.version_probe_dev(v, dlsm_amd.Keys(torch.from_numpy(q).cuda(), n, 20), snap, mask, lf)
    gpu.sync()
    assert np.array_equal(mask.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(lf.cpu().numpy().view(np.uint32), want_lf)
    v.close()
    got = gpu.blocks_check(dev, on_device=True)
    assert got.size == nf + 1 and not got.any()


@pytest.mark.parametrize("n", [0, 1, 20_000, 153_846])
def test_hashed_sealed_build(gpu, orc, n):
    import torch

    import dlsm_amd

    k = orc.dbbench_keys(3, 5, n) if n else np.zeros(20, np.uint8)
    want = orc.filter_block(orc.full_build(k, n))
    h = dlsm_amd.hash_batch(dlsm_amd.Keys(k, n, 20))
    hd = torch.from_numpy(np.ascontiguousarray(h)).cuda()
    for path in (0, 1, 2):
        out = torch.full((len(want) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(1, dtype=torch.uint64, device="cuda")
        gpu.set_path(path)
        try:
            gpu.full_build_block_hashed_dev([hd], [out], lens, 10)
            gpu.sync()
        finally:
            gpu.set_path(0)
        raw = out.cpu().numpy()
        assert int(lens.cpu().numpy()[0]) == len(want), path
        assert raw[: len(want)].tobytes() == want, path
        assert (raw[len(want):] == 0xEE).all(), path
    assert gpu.full_build_block_hashed([h], 10) == [want]
