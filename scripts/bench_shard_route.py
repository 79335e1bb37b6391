"""Shard route of a batched Get (dlsm_shard_route_dev): 100 M db_bench-shaped
20-byte lookups, uniform over the key space, against 16 equal shards and
against 1 shard.

Per shard count it times, warm, in interleaved rounds on one stream with device
events (median, min and max over the rounds):
  route_keys    the route with keys_out (every shard's keys as one aligned run)
  route_index   the route without keys_out (Get indices only)
  torch_sort    torch given the shard ids FOR FREE (int16, computed before the
                window): a stable sort of the ids plus an index_select of the
                20-byte rows -- strictly more passes than the route makes
and reports the bytes the route moves (the byte model of shard_route.hip) and
that traffic at the copy rate dlsm_stream_kernel kind 1 reaches in the same
process: the floor.  The full-size outputs are compared with torch's stable
order.

Then the sharded Get end to end on the version of scripts/bench_read_plan.py
(db_bench's final state, 426 files): the route plus 16 version probes, shard
s probing its run of keys_out against a version of the files that overlap its
key range, against one probe of the unsplit version on the same Gets.

Prints one JSON line; --out writes it.

    python scripts/bench_shard_route.py [--lookups 100000000] [--rounds 21] [--out profiles/shard_route.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lookups", type=int, default=100_000_000)
    ap.add_argument("--space", type=int, default=100_000_000, help="key space V")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--no-e2e", action="store_true", help="skip the sharded end to end")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dlsm_amd
    from bench_read_plan import copy_rate
    from dlsm_amd import workload as W

    dev = torch.device("cuda", 0)
    ctx = dlsm_amd.Context(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    V, Q = args.space, args.lookups
    rng = np.random.default_rng(12)
    qv = torch.from_numpy(rng.integers(0, V, Q, dtype=np.int64)).to(dev)
    qbytes = W.dbbench_keys_torch(qv)
    qk = dlsm_amd.Keys(qbytes, Q, 20)
    rows = qbytes.view(Q, 20)

    res = {"what": "shard route of a batched Get (Get_Target_Shard + each shard's Gets as one aligned run), "
                   "device-resident",
           "lookups": Q, "key_len": 20, "chunk": dlsm_amd.shard_route_chunk(), "rounds": args.rounds,
           "reps": args.reps, "cus": torch.cuda.get_device_properties(0).multi_processor_count,
           "scatter_lds_staging_by_bin": "not tried: the scatter stores each key's dwords from the wave's LDS area",
           "shards": {}}
    res["copy_gb_s"] = copy_rate(dev, stream, 2_000_000_000)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def stat(xs):
        return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}

    def bound(v):
        return W.dbbench_keys_np(np.array([v], dtype=np.uint64)).tobytes()

    routed = {}
    for ns in (16, 1):
        edges = [(s + 1) * V // ns for s in range(ns)]
        m = ctx.shardmap([bound(e) for e in edges])
        cap = dlsm_amd.shard_route_cap(Q, ns)
        off = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
        cnt = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
        gets = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        out = torch.zeros(cap * 20, dtype=torch.uint8, device=dev)
        ids = torch.bucketize(qv, torch.tensor(edges, dtype=torch.int64, device=dev), right=True).to(torch.int16)

        def route_keys():
            ctx.shard_route_dev(m, qk, off, cnt, gets, out)

        def route_index():
            ctx.shard_route_dev(m, qk, off, cnt, gets, None)

        def torch_sort():
            idx = torch.sort(ids, stable=True).indices
            return idx, torch.index_select(rows, 0, idx)

        # warm-up of every shape, and the full-size check against torch's stable order
        route_index()
        route_keys()
        idx, sorted_rows = torch_sort()
        ctx.sync()
        h_off, h_cnt = off.cpu().numpy(), cnt.cpu().numpy()
        want_cnt = torch.bincount(ids.long(), minlength=ns + 1).cpu().numpy()
        ok = bool(np.array_equal(h_cnt, want_cnt)) and bool(np.all(h_off % 4 == 0))
        at = 0
        for s in range(ns + 1):
            o, c = int(h_off[s]), int(h_cnt[s])
            ok = ok and bool(torch.equal(gets[o:o + c].long(), idx[at:at + c]))
            ok = ok and bool(torch.equal(out.view(cap, 20)[o:o + c], sorted_rows[at:at + c]))
            at += c
        del idx, sorted_rows
        legs = {"route_keys": [], "route_index": [], "torch_sort": []}
        for _ in range(args.rounds):
            legs["route_keys"].append(timed(route_keys))
            legs["route_index"].append(timed(route_index))
            legs["torch_sort"].append(timed(torch_sort))
        r = {leg: stat(xs) for leg, xs in legs.items()}
        # byte model (shard_route.hip): count 20 B in + 2 B out; scatter 2 B in + 4 B out, and 20 B in + 20 B out
        # with keys_out
        for leg, per_get in (("route_keys", 68), ("route_index", 28)):
            floor = per_get * Q / (res["copy_gb_s"] * 1e9) * 1e3
            r[leg].update({"model_bytes": per_get * Q, "floor_ms": round(floor, 3),
                           "over_floor": round(r[leg]["median_ms"] / floor, 2),
                           "gb_s": round(per_get * Q / (r[leg]["median_ms"] * 1e-3) / 1e9, 1)})
        r["torch_sort_over_route_keys"] = round(r["torch_sort"]["median_ms"] / r["route_keys"]["median_ms"], 2)
        r["matches_torch_stable_order"] = ok
        res["shards"][str(ns)] = r
        routed[ns] = (m, off, cnt, gets, out, h_off, h_cnt, edges)

    if not args.no_e2e:
        ns = 16
        m, off, cnt, gets, out, h_off, h_cnt, edges = routed[ns]
        files = W.dbbench_version(ctx, dev, V)
        ver = ctx.version(files, on_device=True)
        lo_edges = [0] + edges[:-1]
        key_lo = [bound(e) for e in lo_edges]
        key_hi = [bound(e) for e in edges]
        # shard s = [lo, hi): the files with largest >= lo and smallest < hi (a file that spans several
        # shards belongs to each; the filters are shared device tensors)
        vers = []
        for s in range(ns):
            mine = [f for f in files if f.largest >= key_lo[s] and f.smallest < key_hi[s]]
            vers.append(ctx.version(mine, on_device=True))
        snap = (1 << 56) - 1
        mask = torch.zeros(Q, dtype=torch.int64, device=dev)
        lf = torch.zeros((Q, 5), dtype=torch.int32, device=dev)
        smask = torch.zeros(int(h_off[ns]) + 4, dtype=torch.int64, device=dev)
        slf = torch.zeros((int(h_off[ns]) + 4, 5), dtype=torch.int32, device=dev)
        runs = []
        for s in range(ns):
            o, c = int(h_off[s]), int(h_cnt[s])
            runs.append((vers[s], dlsm_amd.Keys(out[o * 20:(o + c) * 20], c, 20), smask[o:o + c], slf[o:o + c]))

        def unsplit():
            ctx.version_probe_dev(ver, qk, snap, mask, lf)

        def probes():
            for v, k, sm, sl in runs:
                ctx.version_probe_dev(v, k, snap, sm, sl)

        def sharded():
            ctx.shard_route_dev(m, qk, off, cnt, gets, out)
            probes()

        unsplit()
        sharded()
        ctx.sync()
        same = int((mask != 0).sum().item()) == int((smask != 0).sum().item())
        legs = {"unsplit_probe": [], "route_plus_16_probes": [], "the_16_probes": []}
        for _ in range(args.rounds):
            legs["unsplit_probe"].append(timed(unsplit))
            legs["route_plus_16_probes"].append(timed(sharded))
            legs["the_16_probes"].append(timed(probes))
        e = {leg: stat(xs) for leg, xs in legs.items()}
        e["files"] = len(files)
        e["files_per_shard"] = [v.n_files for v in vers]
        e["gets_with_a_candidate_agree"] = same
        e["sharded_over_unsplit"] = round(e["route_plus_16_probes"]["median_ms"] / e["unsplit_probe"]["median_ms"], 2)
        res["end_to_end_16_shards"] = e

    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
