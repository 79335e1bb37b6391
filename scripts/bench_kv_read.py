"""The value read of a seeked Get batch (dlsm_kv_read_dev): 10 M FOUND Gets whose
handles are uniform over a data region built on the GPU with torch, as
TableBuilder_BACS::Add lays pairs out (dlsm_amd/data_region.py's fixed-size
writer restated in torch, compared here with it on a small table).

Legs: values of 400 B (db_bench --value_size=400: pairs of 436 B with 28-byte
internal keys), values of 100 B, and a mixed leg of lengths uniform in
[0, 800].  Timed with device events on one stream:
  call     dlsm_kv_read_dev, best and median of --reps, and each of its three
           launches (size, offsets, copy) from the events the library records
           around them (dlsm_kv_read_stats), medians over the same calls
  gather   for the fixed-size legs, torch's ``region.view(-1, pair)[rows, 36:]``
           of rows it is given for free (no handle, no header, no key compare)
  floor    2 x value bytes over the copy rate dlsm_stream_kernel kind 1 reaches
           in the same process
The bytes are compared with the gather (fixed legs) or with a
torch restatement over the first --check Gets (mixed leg) before timing.
Prints one JSON line; --out writes it.

    python scripts/bench_kv_read.py [--gets 10000000] [--reps 10] [--out profiles/kv_read.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEY = 28  # internal key bytes


def region_torch(values, vals, seq, dev):
    """The data region of a table holding db_bench keys of `values` (int64 on
    dev) with the fixed-size values `vals` (uint8[n, vlen]): uint8[n, 36 + vlen]."""
    import torch

    from dlsm_amd import workload as W

    n, vlen = vals.shape
    out = torch.empty((n, 8 + KEY + vlen), dtype=torch.uint8, device=dev)
    head = KEY.to_bytes(4, "little") + vlen.to_bytes(4, "little")
    out[:, :8] = torch.tensor(list(head), dtype=torch.uint8, device=dev)
    out[:, 8:28] = W.dbbench_keys_torch(values).reshape(n, 20)
    out[:, 28:36] = torch.tensor(list(((seq << 8) | 1).to_bytes(8, "little")), dtype=torch.uint8, device=dev)
    out[:, 36:] = vals
    return out


def handles_torch(offset, size, dev):
    """dlsm_kv_handle{offset, size, file 0} as int64[n, 2]."""
    import torch

    h = torch.empty((offset.numel(), 2), dtype=torch.int64, device=dev)
    h[:, 0] = offset
    h[:, 1] = size
    return h


def timed(stream, fn, reps, ctx=None):
    """Best and median of reps calls between device events; with ctx, the
    launches' own times (dlsm_kv_read_stats) as medians over the same calls."""
    import torch

    ms, parts = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        ms.append(e0.elapsed_time(e1))
        if ctx is not None:
            parts.append(ctx.kv_read_stats()[0])
    out = {"best_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4)}
    if parts:
        for j, name in enumerate(("size_ms", "offsets_ms", "copy_ms")):
            out[name] = round(statistics.median(p[j] for p in parts), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gets", type=int, default=10_000_000)
    ap.add_argument("--rows", type=int, default=10_000_000, help="pairs of the region")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--check", type=int, default=1_000_000, help="mixed leg: Gets compared with the restatement")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dlsm_amd
    from dlsm_amd import data_region as dr
    from dlsm_amd import workload as W

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from bench_read_plan import copy_rate

    dev = torch.device("cuda", 0)
    ctx = dlsm_amd.Context(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    n, R = args.gets, args.rows
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)

    # the torch writer against data_region.py's on a small table
    sv = torch.arange(0, 3000, 3, dtype=torch.int64, device=dev)
    svals = torch.randint(0, 256, (sv.numel(), 13), dtype=torch.uint8, device=dev, generator=gen)
    small = region_torch(sv, svals, 9, dev)
    ik = np.concatenate([W.dbbench_keys_torch(sv).reshape(-1, 20).cpu().numpy(),
                         np.tile(np.frombuffer(((9 << 8) | 1).to_bytes(8, "little"), dtype=np.uint8), (sv.numel(), 1))], axis=1)
    want, _, _ = dr.build_region_fixed(ik, svals.cpu().numpy())
    assert np.array_equal(small.reshape(-1).cpu().numpy(), want), "torch writer differs from data_region.py"

    res = {"gets": n, "rows": R, "reps": args.reps, "chunk": dlsm_amd.kv_read_chunk(), "span": dlsm_amd.kv_read_span(),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count}
    rate = copy_rate(dev, stream, 2_000_000_000)
    res["copy_GBps"] = rate
    values = torch.arange(R, dtype=torch.int64, device=dev) * 3
    rows = torch.randint(0, R, (n,), dtype=torch.int64, device=dev, generator=gen)
    keys = dlsm_amd.Keys(W.dbbench_keys_torch(values[rows]).reshape(-1), n, 20)
    nc = torch.zeros(1, dtype=torch.int64, device=dev)
    vo = torch.zeros(n + 1, dtype=torch.int64, device=dev)

    for vlen in (400, 100):
        pair = 8 + KEY + vlen
        vals = torch.randint(0, 256, (R, vlen), dtype=torch.uint8, device=dev, generator=gen)
        region = region_torch(values, vals, 9, dev)
        del vals
        td = ctx.tabledata([[region.reshape(-1)]], on_device=True)
        hd = handles_torch(rows * pair, pair, dev)
        state = torch.ones(n, dtype=torch.uint8, device=dev)
        out = torch.empty(n * vlen, dtype=torch.uint8, device=dev)
        stream.synchronize()
        call = lambda: ctx.kv_read_dev(td, keys, state, hd, vo, out, n_corrupt=nc)  # noqa: E731
        call()
        gather = region.view(-1, pair)[rows, 36:]
        stream.synchronize()
        assert int(nc.item()) == 0 and bool((state == 1).all()), "a FOUND Get was rejected"
        assert int(vo[n].item()) == n * vlen and torch.equal(vo, torch.arange(n + 1, dtype=torch.int64, device=dev) * vlen)
        assert torch.equal(out.view(n, vlen), gather), "values differ from torch's gather"
        del gather
        leg = {"value_bytes": vlen, "pair_bytes": pair, "out_GB": round(n * vlen / 1e9, 3)}
        leg["call"] = timed(stream, call, args.reps, ctx)
        leg["torch_gather"] = timed(stream, lambda: region.view(-1, pair)[rows, 36:], args.reps)
        leg["floor_ms"] = round(2 * n * vlen / (rate * 1e9) * 1e3, 4)
        leg["call_over_floor"] = round(leg["call"]["best_ms"] / leg["floor_ms"], 2)
        leg["call_over_gather"] = round(leg["call"]["best_ms"] / leg["torch_gather"]["best_ms"], 2)
        leg["call_GBps"] = round(2 * n * vlen / (leg["call"]["best_ms"] * 1e-3) / 1e9, 1)
        res[f"v{vlen}"] = leg
        td.close()
        del region, out, hd

    # mixed lengths: pairs of 36 + len bytes back to back over random bytes
    lens = torch.randint(0, 801, (R,), dtype=torch.int64, device=dev, generator=gen)
    size = lens + 8 + KEY
    end = torch.cumsum(size, 0)
    at = end - size
    region = torch.randint(0, 256, (int(end[-1].item()),), dtype=torch.uint8, device=dev, generator=gen)
    kb = W.dbbench_keys_torch(values).reshape(R, 20)
    cols = torch.arange(20, device=dev)
    region[(at + 8)[:, None] + cols[None, :]] = kb
    del kb
    for j, b in enumerate(KEY.to_bytes(4, "little")):
        region[at + j] = b
    for j in range(4):
        region[at + 4 + j] = ((lens >> (8 * j)) & 255).to(torch.uint8)
    for j, b in enumerate(((9 << 8) | 1).to_bytes(8, "little")):
        region[at + 28 + j] = b
    td = ctx.tabledata([[region]], on_device=True)
    hd = handles_torch(at[rows], size[rows], dev)
    state = torch.ones(n, dtype=torch.uint8, device=dev)
    glen = lens[rows]
    total = int(glen.sum().item())
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    stream.synchronize()
    call = lambda: ctx.kv_read_dev(td, keys, state, hd, vo, out, n_corrupt=nc)  # noqa: E731
    call()
    stream.synchronize()
    want_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    want_off[1:] = torch.cumsum(glen, 0)
    assert int(nc.item()) == 0 and torch.equal(vo, want_off), "offsets differ from cumsum"
    c = min(args.check, n)
    item = torch.repeat_interleave(torch.arange(c, device=dev), glen[:c])
    pos = torch.arange(int(want_off[c].item()), device=dev)
    want = region[(at[rows[:c]] + 36)[item] + pos - want_off[:c][item]]
    assert torch.equal(out[:want.numel()], want), "values differ from the restatement"
    del item, pos, want
    leg = {"value_bytes": "uniform 0..800", "out_GB": round(total / 1e9, 3), "checked_gets": c}
    leg["call"] = timed(stream, call, args.reps, ctx)
    leg["floor_ms"] = round(2 * total / (rate * 1e9) * 1e3, 4)
    leg["call_over_floor"] = round(leg["call"]["best_ms"] / leg["floor_ms"], 2)
    leg["call_GBps"] = round(2 * total / (leg["call"]["best_ms"] * 1e-3) / 1e9, 1)
    res["mixed"] = leg
    res["copy_wgs"] = ctx.kv_read_stats()[1]
    td.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
