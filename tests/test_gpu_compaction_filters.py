"""dlsm_compaction_filters_dev: the sealed filter block of every file of a cut run
on the device, against the oracle's full filter over every file's user keys
(compaction_filters_cases.expected).  Every comparison is ``array_equal`` over
the whole buffer: the outputs are sentinel-filled, so the pads between the
blocks, the bytes behind the total and behind a cap must come back untouched."""
import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from dlsm_amd import compaction as cp
from compaction_filters_cases import CASES, expected, file_records, pack
from compaction_merge_cases import ik, val
from table_build_cases import VALUES

pytestmark = pytest.mark.gpu

SENT, END_SENT = 0xCD, 0x5A5A5A5A5A5A5A5A


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).cuda()


def images(blocks, recs, built, filters_cap, file_cap):
    """What the two output buffers must hold under the caps, sentinels elsewhere."""
    filters = np.full(max(built[1], filters_cap) + 64, SENT, dtype=np.uint8)
    out = np.full((max(built[0], file_cap) + 2, 4), END_SENT, dtype=np.uint64)
    for f, (blk, r) in enumerate(zip(blocks, recs)):
        if r[0] + r[1] <= filters_cap:  # a block that does not lie wholly below the cap is not written
            filters[r[0]:r[0] + r[1]] = np.frombuffer(blk, dtype=np.uint8)
        out[f] = r
    return filters, out


def run(gpu, name, merged=None, out_built=None, filters_cap=None, file_cap=None, pair_cap_extra=5):
    """The device form over a case's cut run on sentinel-filled outputs;
    returns the outputs (numpy), what they must be, and `built`."""
    iks, sizes, bpk = CASES[name]
    blocks, recs, built = expected(name)
    n = len(iks)
    kb, ko, kl = pack(iks + [iks[-1]] * pair_cap_extra)
    files, ob = file_records(sizes)
    filters_cap = built[1] if filters_cap is None else filters_cap
    file_cap = len(sizes) if file_cap is None else file_cap
    flagged = merged is not None or out_built is not None or file_cap < len(sizes)
    want = images([], [], built, filters_cap, file_cap) if flagged else images(blocks, recs, built, filters_cap, file_cap)
    bufs = [dev(w) for w in images([], [], built, filters_cap, file_cap)]
    b = dev(np.full(3 + 8, END_SENT, dtype=np.uint64))
    gpu.compaction_filters_dev(Keys(dev(kb), n + pair_cap_extra, kl, None if ko is None else dev(ko)),
                               dev(np.array(merged or [n + 7, n, 1, 2, 0], dtype=np.uint64)), dev(files),
                               dev(ob if out_built is None else np.array(out_built, dtype=np.uint64)), *bufs, b,
                               bits_per_key=bpk, file_cap=file_cap, filters_cap=filters_cap)
    gpu.sync()
    b = b.cpu().numpy().view(np.uint64)
    assert (b[3:] == END_SENT).all()
    return [bufs[0].cpu().numpy(), bufs[1].cpu().numpy().view(np.uint64)], want, b[:3].tolist()


@pytest.mark.parametrize("name", list(CASES))
def test_byte_parity_with_the_oracle(gpu, name):
    got, want, b = run(gpu, name)
    assert b == list(expected(name)[2])
    assert np.array_equal(got[1], want[1]), "recs"
    assert np.array_equal(got[0], want[0]), "filters"


def test_the_slices_case_has_a_short_last_slice(gpu):
    run(gpu, "slices-var")
    lines, lg = expected("slices-var")[1][0][3], gpu.compaction_filters_stats()[1]
    assert lines > 3 << lg and lines % (1 << lg) != 0


@pytest.mark.parametrize("name", ["straddle", "chunk-edges"])
@pytest.mark.parametrize("less", ["one", "half"])
def test_filters_cap_keeps_totals_exact_and_nothing_past_it(gpu, name, less):
    built = expected(name)[2]
    got, want, b = run(gpu, name, filters_cap=built[1] - 1 if less == "one" else built[1] // 2)
    assert b == [built[0], built[1], dlsm_amd.FILTERS_CAP]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


@pytest.mark.parametrize("how", [dict(merged=[150, 150, 0, 0, 4]), dict(merged=[160, 156, 0, 0, 0]), dict(file_cap=37),
                                 dict(out_built=[38, 0, 0, 0, dlsm_amd.OUTPUT_FILE_CAP])],
                         ids=["flagged", "n_out-past-pair_cap", "file_cap-below-n_files", "built-flagged"])
def test_flagged_input_writes_only_built(gpu, how):
    got, want, b = run(gpu, "straddle", **how)  # pair_cap is 155
    assert b == [0, 0, dlsm_amd.FILTERS_INPUT_FLAGGED]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


def test_merge_output_filters_open_probe_on_one_stream(gpu, orc):
    """Two overlapping runs are merged (hidden pairs dropped, so n_out is known
    to the device only), cut, built and their filter blocks written with no
    read in between; then one read of the records, every block against the
    oracle, the blocks opened where they lie with their checksums verified, and
    every key of the run probed in its own file's filter."""
    import torch

    runs = [[(ik(b"%08d" % x, 9 - r, True), val(r, x, VALUES["mix"])) for x in range(r, 9000, 1 + r)] for r in range(2)]
    n_in = sum(len(r) for r in runs)
    pk = lambda items: pack(items)[:2]  # noqa: E731
    hk, hko, hv, hvo, _, hm = dlsm_amd.compaction_merge([(Keys.pack([k for k, _ in r]), *pk([v for _, v in r]), 0) for r in runs],
                                                        1, 100)
    assert hm[1] < n_in and hm[4] == 0
    dr = []
    for r in runs:
        k, (vb, vo) = Keys.pack([k for k, _ in r]), pk([v for _, v in r])
        dr.append((Keys(dev(k.data), len(r), 0, dev(k.offsets)), dev(vb), dev(vo), 0))
    u8 = lambda n: torch.full((n,), SENT, dtype=torch.uint8, device="cuda")  # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")  # noqa: E731
    keys, values, ko, vo, merged = u8(len(hk) + 4096), u8(len(hv) + 4096), i64(n_in + 1), i64(n_in + 1), i64(5)
    caps = dlsm_amd.compaction_output_bound(n_in, len(hk) + 4096, len(hv) + 4096, 40000, 4096)
    data, index, ends, files, built = u8(caps[0]), u8(caps[1]), i64(caps[2]), i64(9 * caps[3]), i64(5)
    filters, recs, fbuilt = u8(dlsm_amd.compaction_filters_bound(n_in, caps[3])), i64(4 * caps[3]), i64(3)
    gpu.compaction_merge_dev(dr, keys, ko, values, vo, merged, policy=1, smallest_snapshot=100)
    gpu.compaction_output_dev(Keys(keys, n_in, 0, ko), values, merged, data, index, ends, files, built, value_off=vo,
                              max_file_bytes=40000, chunk_bytes=4096)
    gpu.compaction_filters_dev(Keys(keys, n_in, 0, ko), merged, files, built, filters, recs, fbuilt)
    gpu.sync()
    fb = fbuilt.cpu().numpy().view(np.uint64).tolist()
    nf = int(built.cpu().numpy()[0])
    assert fb[0] == nf and 3 < nf <= 64 and fb[2] == 0
    frec = files.cpu().numpy().view(np.uint64).reshape(-1, 9)[:nf]
    rec = recs.cpu().numpy().view(np.uint64).reshape(-1, 4)[:nf]
    host_filters = filters.cpu().numpy()
    users = [bytes(hk[int(hko[i]):int(hko[i + 1]) - 8]) for i in range(hm[1])]
    base = 0
    for (first, n), r in zip(frec[:, :2].tolist(), rec.tolist()):
        kd, offs = orc.pack_var(users[first:first + n])
        want = orc.filter_block(orc.full_build(kd, n, offsets=offs))
        assert r[:2] == [base, len(want)] and host_filters[base:base + len(want)].tobytes() == want
        base += len(want) + 15 & ~15
    assert fb[1] == base and (host_filters[base:] == SENT).all()
    (fs,) = cp.open_filters(gpu, filters, rec)
    mask = u8(hm[1] * fs.mask_bytes)
    gpu.full_probe_dev(fs, Keys(keys, hm[1], 0, ko, suffix_len=8), mask)
    gpu.sync()
    bits = np.unpackbits(mask.cpu().numpy().reshape(hm[1], fs.mask_bytes), axis=1, bitorder="little")
    own = np.repeat(np.arange(nf), frec[:, 1].astype(np.int64))
    assert bits[np.arange(hm[1]), own].all()
    fs.close()


def test_bad_arguments_and_fault_injection(gpu):
    import torch

    z = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    q = torch.zeros(9 * (dlsm_amd.OUTPUT_MAX_FILES + 1), dtype=torch.int64, device="cuda")
    for filters, kw in ((z, {"file_cap": dlsm_amd.OUTPUT_MAX_FILES + 1}), (z[1:], {"file_cap": 1}),
                        (z, {"file_cap": 1, "bits_per_key": 0})):  # too many files; filters not 16-byte aligned; bits per key
        with pytest.raises(dlsm_amd.DlsmError) as e:
            gpu.compaction_filters_dev(Keys(z, 4, 28), q, q, q, filters, q, q, **kw)
        assert e.value.status == -1  # DLSM_E_ARG
    gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 4)
    try:
        iks, sizes, _ = CASES["straddle"]
        kb, ko, kl = pack(iks)
        for form in (lambda: run(gpu, "straddle"),
                     lambda: gpu.compaction_filters(Keys(kb, len(iks), kl, ko), [150, 150, 0, 0, 0], *file_records(sizes))):
            with pytest.raises(dlsm_amd.DlsmError) as e:
                form()
            assert e.value.status == -4
    finally:
        gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 0)
    run(gpu, "straddle")
