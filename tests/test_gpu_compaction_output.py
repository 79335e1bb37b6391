"""dlsm_compaction_output_dev: a merged run on the device cut into size-capped
tables, against a Python walk of the cut rule and the host table build of every
file's pairs (compaction_output_cases.expected).  Every comparison is
``array_equal`` over the whole buffer: the outputs are sentinel-filled, so the
pads between the files, the bytes behind every total and behind every cap must
come back untouched."""
import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from dlsm_amd import compaction as cp
from compaction_merge_cases import ik, val
from compaction_output_cases import CASES, expected, pack
from table_build_cases import VALUES

pytestmark = pytest.mark.gpu

SENT, END_SENT = 0xCD, 0x5A5A5A5A5A5A5A5A
CAPS = ("data_cap", "index_cap", "chunk_cap", "file_cap")


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).cuda()


def images(tables, recs, built, caps):
    """What the four output buffers must hold under the caps, sentinels elsewhere."""
    data = np.full(max(built[1], caps[0]) + 64, SENT, dtype=np.uint8)
    index = np.full(max(built[2], caps[1]) + 64, SENT, dtype=np.uint8)
    ends = np.full(max(built[3], caps[2]) + 8, END_SENT, dtype=np.uint64)
    files = np.full((max(built[0], caps[3]) + 2, 9), END_SENT, dtype=np.uint64)
    for f, ((d, e, x), r) in enumerate(zip(tables, recs)):
        m = max(0, min(len(d), caps[0] - r[2]))
        data[r[2]:r[2] + m] = np.frombuffer(d, dtype=np.uint8)[:m]
        x = x if r[4] + len(x) <= caps[1] else x[:-5]  # the trailer only where the whole block fits
        m = max(0, min(len(x), caps[1] - r[4]))
        index[r[4]:r[4] + m] = np.frombuffer(x, dtype=np.uint8)[:m]
        m = max(0, min(len(e), caps[2] - r[6]))
        ends[r[6]:r[6] + m] = e[:m]
        if f < caps[3]:
            files[f] = r
    return data, index, ends, files


def run(gpu, name, merged=None, pair_cap_extra=5, **caps):
    """The device form over a case's run on sentinel-filled outputs; returns
    the outputs (numpy) and what they must be."""
    _, _, _, mfb, cb = CASES[name]
    iks, vals, tables, recs, built = expected(name)
    n = len(iks)
    extra = [iks[-1]] * pair_cap_extra if n else []
    kb, ko, kl = pack(iks + extra)
    vb, vo, vl = pack(vals + [vals[-1] for _ in extra])
    cap = [caps.get(c, built[i]) for c, i in zip(CAPS, (1, 2, 3, 0))]
    want = images(tables, recs, built, cap)
    bufs = [dev(w) for w in images([], [], built, cap)]
    out = dev(np.full(5 + 8, END_SENT, dtype=np.uint64))
    m = dev(np.array(merged or [n + 7, n, 1, 2, 0], dtype=np.uint64))
    gpu.compaction_output_dev(Keys(dev(kb), n + len(extra), kl, None if ko is None else dev(ko)), dev(vb), m, *bufs, out,
                              value_off=None if vo is None else dev(vo), value_len=vl, max_file_bytes=mfb, chunk_bytes=cb,
                              **dict(zip(CAPS, cap)))
    gpu.sync()
    got = [b.cpu().numpy() for b in bufs]
    got = [got[0], got[1], got[2].view(np.uint64), got[3].view(np.uint64)]
    b = out.cpu().numpy().view(np.uint64)
    assert (b[5:] == END_SENT).all()
    return got, want, b[:5].tolist(), built


@pytest.mark.parametrize("name", list(CASES))
def test_byte_parity_with_the_walk_and_the_table_build(gpu, name):
    got, want, b, built = run(gpu, name)
    assert b == list(built)
    for g, w, what in zip(got, want, ("data", "index", "chunk_end", "files")):
        assert np.array_equal(g, w), what


@pytest.mark.parametrize("name", ["varint-chunks", "every-pair-var", "fixed"])
@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("less", ["one", "half"])
def test_caps_keep_totals_exact_and_nothing_past_them(gpu, name, which, less):
    built = expected(name)[4]
    need = built[(1, 2, 3, 0)[which]]
    got, want, b, _ = run(gpu, name, **{CAPS[which]: need - 1 if less == "one" else need // 2})
    assert b == list(built[:4]) + [built[4] | (1, 2, 4, dlsm_amd.OUTPUT_FILE_CAP)[which]]
    for g, w, what in zip(got, want, ("data", "index", "chunk_end", "files")):
        assert np.array_equal(g, w), what


@pytest.mark.parametrize("merged", [[25, 25, 0, 0, 4], [40, 31, 0, 0, 0]], ids=["flagged", "n_out-past-pair_cap"])
def test_flagged_input_writes_only_built(gpu, merged):
    got, _, b, built = run(gpu, "exact", merged=merged)  # pair_cap is 30
    assert b[4] == dlsm_amd.OUTPUT_INPUT_FLAGGED
    for g, w in zip(got, images([], [], built, [built[i] for i in (1, 2, 3, 0)])):
        assert np.array_equal(g, w)


def test_merge_output_open_merge_on_one_stream(gpu):
    """Two overlapping runs are merged (hidden pairs dropped, so n_out is below
    pair_cap and known to the device only), cut and built with no read in
    between; the tables are opened where they lie and merged again."""
    import torch

    runs = [[(ik(b"%08d" % x, 9 - r, True), val(r, x, VALUES["mix"])) for x in range(r, 900, 1 + r)] for r in range(2)]
    n_in = sum(len(r) for r in runs)
    hk, hko, hv, hvo, _, hm = dlsm_amd.compaction_merge(
        [(Keys.pack([k for k, _ in r]), *pack([v for _, v in r])[:2], 0) for r in runs], 1, 100)
    assert hm[1] < n_in and hm[4] == 0
    want_tables, want_files, want_built = dlsm_amd.compaction_output(Keys(hk, hm[1], 0, hko), hv, hm, value_off=hvo,
                                                                    max_file_bytes=30000, chunk_bytes=4096)
    assert want_built[0] > 3
    dr = []
    for r in runs:
        k, (vb, vo, _) = Keys.pack([k for k, _ in r]), pack([v for _, v in r])
        dr.append((Keys(dev(k.data), len(r), 0, dev(k.offsets)), dev(vb), dev(vo), 0))
    u8 = lambda n: torch.full((n,), SENT, dtype=torch.uint8, device="cuda")  # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")  # noqa: E731
    keys, values, ko, vo, merged = u8(len(hk) + 4096), u8(len(hv) + 4096), i64(n_in + 1), i64(n_in + 1), i64(5)
    caps = dlsm_amd.compaction_output_bound(n_in, len(hk) + 4096, len(hv) + 4096, 30000, 4096)
    data, index, ends, files, built = u8(caps[0]), u8(caps[1]), i64(caps[2]), i64(9 * caps[3]), i64(5)
    gpu.compaction_merge_dev(dr, keys, ko, values, vo, merged, policy=1, smallest_snapshot=100)
    gpu.compaction_output_dev(Keys(keys, n_in, 0, ko), values, merged, data, index, ends, files, built, value_off=vo,
                              max_file_bytes=30000, chunk_bytes=4096)
    gpu.sync()
    b = built.cpu().numpy().view(np.uint64).tolist()
    assert b == list(want_built)
    recs = files.cpu().numpy().view(np.uint64).reshape(-1, 9)[:b[0]]
    assert np.array_equal(recs, want_files)
    host_ends = ends.cpu().numpy().view(np.uint64)
    for (d, e, x), (wd, we, wx) in zip(dlsm_amd.output_tables(data.cpu().numpy(), index.cpu().numpy(), host_ends, recs),
                                       want_tables):
        assert np.array_equal(d, wd) and np.array_equal(e, we) and np.array_equal(x, wx)
    ti, td = cp.open_output(gpu, data, index, host_ends, recs)
    k2, v2, ko2, vo2, m2 = u8(len(hk) + 64), u8(len(hv) + 64), i64(hm[1] + 1), i64(hm[1] + 1), i64(5)
    gpu.compaction_merge_tables_dev(ti, td, [list(range(b[0]))], k2, ko2, v2, vo2, m2, policy=0)
    gpu.sync()
    assert m2.cpu().numpy().view(np.uint64).tolist() == [hm[1], hm[1], hm[2], hm[3], 0]
    assert np.array_equal(k2.cpu().numpy()[:hm[2]], hk) and np.array_equal(v2.cpu().numpy()[:hm[3]], hv)
    assert np.array_equal(ko2.cpu().numpy().view(np.uint64), hko) and np.array_equal(vo2.cpu().numpy().view(np.uint64), hvo)
    ti.close()
    td.close()


def test_bad_arguments_and_fault_injection(gpu):
    import torch

    z = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    q = torch.zeros(9 * (dlsm_amd.OUTPUT_MAX_FILES + 1), dtype=torch.int64, device="cuda")
    for data, kw in ((z, {"file_cap": dlsm_amd.OUTPUT_MAX_FILES + 1}), (z[1:], {})):  # too many files; data not 16-byte aligned
        with pytest.raises(dlsm_amd.DlsmError) as e:
            gpu.compaction_output_dev(Keys(z, 4, 28), z, q, data, z, q, q, q, value_len=28, **kw)
        assert e.value.status == -1  # DLSM_E_ARG
    gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 4)
    try:
        for form in (lambda: run(gpu, "exact"),
                     lambda: gpu.compaction_output(Keys(np.zeros(112, dtype=np.uint8), 4, 28), np.zeros(4, dtype=np.uint8),
                                                   [4, 4, 0, 0, 0], value_len=1)):
            with pytest.raises(dlsm_amd.DlsmError) as e:
                form()
            assert e.value.status == -4
    finally:
        gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 0)
    run(gpu, "exact")
