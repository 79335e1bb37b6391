"""The compaction filters (dlsm_compaction_filters_dev): the sealed filter block of
every output file of a compaction, from the cut run on the device in one call.

Workload: the L0 -> L1 merge of DESIGN §7, 1.69 M pairs with 100-byte values cut
into 12 and 100 files (the records a compaction output of that shape writes:
equal pair counts per file), as fixed 28-byte internal keys (db_bench user keys)
and as variable-length ones (the same keys cut to 12..20 user bytes, behind
key_off).  Timed warm, medians of --reps:
  call      dlsm_compaction_filters_dev end to end (host clock around the call
            and the stream's drain) and each launch from the events the library
            records (dlsm_compaction_filters_stats)
  baseline  what a caller has without it: drain the stream, read the file
            records, one dlsm_bloom_full_build_block_dev over the files as jobs;
            host clock, drained
  floor     the hash pass's own bytes (keys and offsets read, hashes written)
            over the copy rate dlsm_stream_kernel kind 1 reaches in the same
            process
The call's blocks are compared with the baseline's before timing.  Prints one
JSON line; --out writes it.

    python scripts/bench_compaction_filters.py [--reps 20] [--out profiles/compaction_filters.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KEY, BPK = 28, 10
KINDS = ("hash", "plan", "partition", "slice", "finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1_690_000)
    ap.add_argument("--out")
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
    n = args.n
    res = {"reps": args.reps, "n": n, "bits_per_key": BPK, "legs": []}
    rate = copy_rate(dev, stream, 2_000_000_000)
    res["copy_GBps"] = rate
    user = W.dbbench_keys_torch(torch.arange(n, dtype=torch.int64, device=dev) * 3).reshape(n, 20).cpu().numpy()
    trailer = np.frombuffer(((9 << 8) | 1).to_bytes(8, "little"), dtype=np.uint8)
    k28 = np.concatenate([user, np.broadcast_to(trailer, (n, 8))], axis=1)
    ulen = 12 + np.arange(n) % 9  # the variable-length form: the last 12..20 digits of the user key, then the trailer
    col = np.arange(32)[None, :]
    digits = np.take_along_axis(user, np.clip(col + 20 - ulen[:, None], 0, 19), axis=1)
    rows = np.where(col < ulen[:, None], digits, trailer[np.clip(col - ulen[:, None], 0, 7)])
    var_flat = rows[col < ulen[:, None] + 8]
    var_off = np.concatenate([[0], np.cumsum(ulen + 8)]).astype(np.int64)
    forms = {"k28": (torch.from_numpy(k28.reshape(-1)).to(dev), None, n * KEY),
             "var": (torch.from_numpy(var_flat).to(dev), torch.from_numpy(var_off).to(dev), len(var_flat) + 8 * (n + 1))}
    merged = torch.tensor([n, n, 0, 0, 0], dtype=torch.int64, device=dev)
    med = statistics.median
    for form, (kflat, ko, key_bytes) in forms.items():
        for want_files in (12, 100):
            per = -(-n // want_files)
            first = np.arange(0, n, per, dtype=np.int64)
            F = len(first)
            frec = np.zeros((F, 9), dtype=np.int64)
            frec[:, 0], frec[:, 1] = first, np.minimum(per, n - first)
            files = torch.from_numpy(frec.reshape(-1)).to(dev)
            out_built = torch.tensor([F, 0, 0, 0, 0], dtype=torch.int64, device=dev)
            cap = dlsm_amd.compaction_filters_bound(n, F, BPK)
            filters, bfilters = (torch.zeros(cap + 256 * F, dtype=torch.uint8, device=dev) for _ in range(2))
            recs, built = torch.zeros(4 * F, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
            lens = torch.zeros(F, dtype=torch.int64, device=dev)
            keys = dlsm_amd.Keys(kflat, n, KEY) if ko is None else dlsm_amd.Keys(kflat, n, 0, ko)

            def call():
                ctx.compaction_filters_dev(keys, merged, files, out_built, filters, recs, built, bits_per_key=BPK,
                                           filters_cap=cap)

            def baseline():
                """Returns each job's place in bfilters."""
                ctx.sync()
                fr = files.cpu().numpy().reshape(-1, 9)
                tables, outs, at = [], [], 0
                for a, cnt in fr[:, :2].tolist():
                    slot = dlsm_amd.full_size(cnt, BPK)[0] + 5
                    tables.append(dlsm_amd.Keys(kflat[a * KEY:], cnt, KEY, None, 8) if ko is None else
                                  dlsm_amd.Keys(kflat, cnt, 0, ko[a:], 8))
                    outs.append(bfilters[at:at + slot])
                    at += (slot + 255) & ~255
                ctx.full_build_block_dev(tables, outs, lens, BPK)
                ctx.sync()
                return outs

            call()
            ctx.sync()
            b = built.cpu().numpy().tolist()
            assert b[0] == F and b[2] == 0, b
            outs, rec = baseline(), recs.cpu().numpy().reshape(-1, 4)
            for r, o, ln in zip(rec.tolist(), outs, lens.cpu().numpy().tolist()):
                assert r[1] == ln and torch.equal(filters[r[0]:r[0] + r[1]], o[:ln]), "filter blocks differ"
            wall, parts, base_ms = [], [], []
            for _ in range(args.reps):
                ctx.sync()
                t0 = time.perf_counter()
                call()
                ctx.sync()
                wall.append((time.perf_counter() - t0) * 1e3)
                parts.append(ctx.compaction_filters_stats()[0])
                t0 = time.perf_counter()
                baseline()
                base_ms.append((time.perf_counter() - t0) * 1e3)
            launch = {k: med(p[j] for p in parts) for j, k in enumerate(KINDS)}
            _, lg, wgs = ctx.compaction_filters_stats()
            res["legs"].append({"keys": form, "n_files": F, "filter_bytes": b[1], "lgR": lg, "slice_wgs": wgs,
                                "call_wall_ms": med(wall), "call_device_ms": sum(launch.values()), "launch_ms": launch,
                                "baseline_wall_ms": med(base_ms), "baseline_over_call": med(base_ms) / med(wall),
                                "hash_floor_ms": (key_bytes + 4 * n) / rate / 1e6})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
