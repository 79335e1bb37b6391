"""dlsm_table_build_dev: a table's data region, chunk ends and sealed index
block from pairs on the device, against dlsm_amd/data_region.py and
dlsm_amd/index_block.py -- pure Python writers that never call the code under
test.  Every comparison is ``array_equal``; every output carries sentinels: 64
bytes behind each total and behind each cap, 8 entries behind ``chunk_end``.
C is the implementation's pairs per workgroup chunk, Sp its output bytes per
workgroup step of the region write.
"""
import numpy as np
import pytest

import dlsm_amd
from dlsm_amd import Keys
from dlsm_amd import data_region as dr
from dlsm_amd import index_block as ib
from table_build_cases import KEYS, VALUES, make

pytestmark = pytest.mark.gpu

C, Sp = dlsm_amd.table_build_chunk(), dlsm_amd.table_build_span()
SENT, END_SENT = 0xCD, 0x5A5A5A5A5A5A5A5A
FOUND, DELETED, NOTFOUND = 1, 2, 0
def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).cuda()


def packed(items):
    """The device form of keys or values: no byte behind the last one; one length
    (the key_len / value_len form) wherever the lengths are uniform, else offsets."""
    data = dev(np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8))
    if len(set(map(len, items))) == 1:
        return data, None, len(items[0])
    return data, dev(np.concatenate([[0], np.cumsum([len(x) for x in items])]).astype(np.uint64)), 0


def build(gpu, iks, vals, chunk_bytes=0, data_cap=None, index_cap=None, chunk_cap=None):
    """Runs the build on sentinel-filled outputs; checks everything against the
    Python writers and returns the device outputs."""
    import torch

    n = len(iks)
    chunks, handles = dr.build_region(list(zip(iks, vals)), chunk_bytes or None)
    region, block = b"".join(chunks), ib.build_index_block(iks, handles)
    ends = np.cumsum([len(c) for c in chunks]).astype(np.uint64)
    kb, ko, kl = packed(iks)
    keys = Keys(kb, n, kl, ko)
    vb, vo, vl = packed(vals)
    caps = [len(region) if data_cap is None else data_cap, len(block) if index_cap is None else index_cap,
            len(ends) if chunk_cap is None else chunk_cap]
    data = torch.full((max(len(region), caps[0]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    index = torch.full((max(len(block), caps[1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    ce = dev(np.full(max(len(ends), caps[2]) + 8, END_SENT, dtype=np.uint64))
    built = dev(np.full(4 + 8, END_SENT, dtype=np.uint64))
    gpu.table_build_dev(keys, vb, data, index, ce, built, value_off=vo, value_len=vl, chunk_bytes=chunk_bytes,
                        data_cap=caps[0], index_cap=caps[1], chunk_cap=caps[2])
    gpu.sync()
    b = built.cpu().numpy().view(np.uint64)
    over = [len(region) > caps[0], len(block) > caps[1], len(ends) > caps[2]]
    oversize = bool(chunk_bytes) and any(s > chunk_bytes for _, s in handles)
    assert b[:4].tolist() == [len(region), len(block), len(ends), over[0] + 2 * over[1] + 4 * over[2] + 64 * oversize]
    assert (b[4:] == END_SENT).all()
    for got, want, cap in ((data, region, caps[0]), (index, block[:-5] if over[1] else block, caps[1])):
        got, m = got.cpu().numpy(), min(len(want), cap)
        assert np.array_equal(got[:m], np.frombuffer(want, dtype=np.uint8)[:m])
        assert (got[m:] == SENT).all()  # nothing at or past a cap or a total; no trailer unless the block fits
    got, m = ce.cpu().numpy().view(np.uint64), min(len(ends), caps[2])
    assert np.array_equal(got[:m], ends[:m]) and (got[m:] == END_SENT).all()
    return data, index, ce, b


def edge(what, delta):
    """Pairs whose region (or entry area) ends delta bytes from a multiple of Sp."""
    if what == "region":  # 64-byte pairs; the last value absorbs delta
        return make(Sp // 64, KEYS["k28"], lambda j: 28 + (delta if j == Sp // 64 - 1 else 0))
    iks, vals = make(Sp // 32 + 64, KEYS["k28"], VALUES["v0"])
    _, handles = dr.build_region(list(zip(iks, vals)))
    end = np.cumsum([3 + 28 + len(ib.encode_handle(*h)) for h in handles])
    n = int(np.searchsorted(end, Sp - 50))  # entries [0, n) end 50 .. 85 bytes short: the last key absorbs the rest
    iks[n - 1] = iks[n - 1][:20] + b"p" * int(Sp + delta - end[n - 1]) + iks[n - 1][20:]
    assert len(ib.build_index_contents(iks[:n], handles[:n])) - 4 * (n + 1) == Sp + delta
    return iks[:n], vals[:n]


CASES = [(f"n{n}-{k}", lambda n=n, k=k: (make(n, KEYS[k], VALUES["mix"]), {}))
         for n in (0, 1, 2, C - 1, C, C + 1, 2 * C + 3) for k in KEYS]
CASES += [(f"{v}", lambda v=v: (make(C + 1, KEYS["var"], VALUES[v]), {})) for v in VALUES]
CASES += [(f"{k}-{v}", lambda k=k, v=v: (make(C + 1, KEYS[k], VALUES[v]), {})) for k in ("k28", "k8") for v in VALUES]
CASES += [("past-2^21", lambda: (make(6 * C, KEYS["k28"], VALUES["v400"]), {})),
          ("window-overflow", lambda: (make(4 * C + 3, KEYS["k8"], VALUES["v1"]), {}))]
CASES += [(f"{w}-edge{d:+d}", lambda w=w, d=d: (edge(w, d), {})) for w in ("region", "entries") for d in (-3, 0, 3)]
CASES += [(f"chunk-{name}", lambda f=f: (lambda p: (p, {"chunk_bytes": f(*p)}))(make(C + 1, KEYS["var"], VALUES["mix"])))
          for name, f in (("exact", lambda i, v: len(b"".join(i[:40] + v[:40])) + 320),
                          ("minus1", lambda i, v: len(b"".join(i[:40] + v[:40])) + 319),
                          ("oversize", lambda i, v: 15), ("1000", lambda i, v: 1000))]
CASES += [(f"cap-{name}", lambda kw=kw: (make(C + 1, KEYS["var"], VALUES["mix"]), dict(kw, chunk_bytes=1000)))
          for name, kw in (("data-mid", {"data_cap": Sp + 23}), ("data-0", {"data_cap": 0}), ("index-mid", {"index_cap": 8192 + 7}),
                           ("index-0", {"index_cap": 0}), ("index-trailer", {"index_cap": -2}), ("chunk-mid", {"chunk_cap": 5}),
                           ("chunk-0", {"chunk_cap": 0}))]


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=[c[0] for c in CASES])
def test_build_against_the_python_writers(gpu, case):
    (iks, vals), kw = case()
    if kw.get("index_cap") == -2:  # the contents fit, the trailer does not
        kw["index_cap"] = len(ib.build_index_block(iks, dr.build_region(list(zip(iks, vals)))[1])) - 2
    build(gpu, iks, vals, **kw)


def test_built_tables_open_and_answer_gets(gpu):
    """Two files built on the device, opened without leaving it, then index
    seek -> value read for present, deleted and absent keys."""
    import torch

    files, keep = [], []
    for f, (n, cb) in enumerate(((C + 5, 0), (300, 4096))):
        iks, vals = make(n, lambda j: 28 + j % 50, VALUES["mix"], seed=f)
        iks = [bytes([65 + f]) + k for k in iks]
        data, index, ce, b = build(gpu, iks, vals, chunk_bytes=cb)
        ends = [0] + ce.cpu().numpy().view(np.uint64)[:b[2]].tolist()
        keep.append((index[:b[1]], [data[s:e] for s, e in zip(ends, ends[1:])]))
        files.append((iks, vals))
    ti = gpu.tableindex([k[0] for k in keep], on_device=True)
    td = gpu.tabledata([k[1] for k in keep], on_device=True)
    gets, want = [], []  # (file, user key) -> (state, value)
    for f, (iks, vals) in enumerate(files):
        for j in range(0, len(iks), 7):
            gets.append((f, iks[j][:-8]))
            want.append((FOUND, vals[j]) if iks[j][-8] == 1 else (DELETED, b""))
        gets.append((f, bytes([65 + f]) + b"absent"))
        want.append((NOTFOUND, b""))
    m = len(gets)
    k = Keys.pack([g[1] for g in gets])
    keys = Keys(dev(k.data), m, 0, dev(k.offsets))
    fb = np.searchsorted([g[0] for g in gets], [0, 1, 2]).astype(np.uint64)  # the Gets are grouped by file
    st = torch.zeros(m, dtype=torch.uint8, device="cuda")
    hd = torch.zeros((m, 16), dtype=torch.uint8, device="cuda")
    gd = torch.arange(m, dtype=torch.int32, device="cuda")
    gpu.index_seek_dev(ti, keys, (1 << 56) - 1, dev(fb), gd, task_state=st, task_handle=hd)
    vo = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    vb = torch.zeros(sum(len(w[1]) for w in want) + 16, dtype=torch.uint8, device="cuda")
    gpu.kv_read_dev(td, keys, st, hd, vo, vb, gets=gd)
    gpu.sync()
    assert st.cpu().numpy().tolist() == [w[0] for w in want]
    assert vo.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(w[1]) for w in want])]).tolist()
    assert vb.cpu().numpy()[:-16].tobytes() == b"".join(w[1] for w in want)
    ti.close()
    td.close()


def test_fault_injection_reaches_both_forms(gpu):
    iks, vals = make(5, KEYS["k28"], VALUES["v17"])
    gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 4)
    try:
        host = lambda: gpu.table_build(Keys.pack(iks), np.zeros(101, dtype=np.uint8), value_len=17)  # noqa: E731
        for call in (lambda: build(gpu, iks, vals), host):
            with pytest.raises(dlsm_amd.DlsmError) as e:
                call()
            assert e.value.status == -4
    finally:
        gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 0)
    build(gpu, iks, vals)
