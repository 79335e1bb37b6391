"""The compaction merge (dlsm_compaction_merge_dev): sorted runs on the device
into one run in the table build's input form.

Cases, db_bench's 24-byte internal keys (16-byte user keys), values of 100 and
400 bytes, KEEP_ALL (every byte moves), one flush = 153,846 pairs:
  l0-into-l1  one flush into ten flushes' worth of level files passed as one run (R = 2)
  8-flushes   eight overlapping flush-sized runs (R = 8)
  disjoint    two flush-sized runs with disjoint ranges (R = 2)
Timed with device events on one stream, warm, medians of --reps:
  call     dlsm_compaction_merge_dev, and its launch kinds (record, partition,
           merge, decide, offsets, gather) from the events the library records
           (dlsm_compaction_merge_stats); pass_share = (partition + merge) / sum
  floor    input keys and values read once, outputs written once, over the copy
           rate dlsm_stream_kernel kind 1 reaches in the same process
  torch    torch.sort of pre-decoded int64 keys it is handed for free, plus
           index gathers of keys and values, on the same device
  host     both arrays to the host, np.concatenate + argsort(kind="stable") +
           take, and back (host clock): the path dbbench_replay.py uses today
The merged keys and values are compared with the torch baseline's before
timing.  Prints one JSON line; --out writes it.

    python scripts/bench_compaction_merge.py [--reps 20] [--out profiles/compaction_merge.json]
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

FLUSH, KEY = 153_846, 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np
    import torch

    import dlsm_amd
    from bench_read_plan import copy_rate

    dev = torch.device("cuda", 0)
    ctx = dlsm_amd.Context(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    res = {"reps": args.reps, "tile": dlsm_amd.merge_tile(), "span": dlsm_amd.merge_span(),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "legs": []}
    rate = copy_rate(dev, stream, 2_000_000_000)
    res["copy_GBps"] = rate

    def make_run(n, lo, hi, seq):
        """n distinct sorted numbers of [lo, hi) as 16 decimal digits + trailer; also the int64 sort key."""
        num = torch.randperm(hi - lo, device=dev, generator=gen)[:n].sort().values + lo
        digits = (num[:, None] // (10 ** torch.arange(15, -1, -1, device=dev, dtype=torch.int64))[None, :]) % 10 + 48
        k = torch.empty((n, KEY), dtype=torch.uint8, device=dev)
        k[:, :16] = digits.to(torch.uint8)
        k[:, 16:] = torch.tensor(list(((seq << 8) | 1).to_bytes(8, "little")), dtype=torch.uint8, device=dev)
        return k, num * 256 + (255 - seq)  # ascending: number, then sequence descending

    span = 40 * FLUSH
    cases = {"l0-into-l1": [(FLUSH, 0, span, 2), (10 * FLUSH, 0, span, 1)],
             "8-flushes": [(FLUSH, 0, span, 8 - r) for r in range(8)],
             "disjoint": [(FLUSH, 0, span, 1), (FLUSH, span, 2 * span, 2)]}
    for name, spec in cases.items():
        made = [make_run(*s) for s in spec]
        n = sum(s[0] for s in spec)
        allk, sortkey = torch.cat([m[0] for m in made]), torch.cat([m[1] for m in made])
        for vlen in (100, 400):
            vals = [torch.randint(0, 256, (s[0], vlen), dtype=torch.uint8, device=dev, generator=gen) for s in spec]
            allv = torch.cat(vals)
            runs = [(dlsm_amd.Keys(m[0].reshape(-1), s[0], KEY), v.reshape(-1), None, vlen) for m, s, v in zip(made, spec, vals)]
            keys, values = (torch.empty(n * w, dtype=torch.uint8, device=dev) for w in (KEY, vlen))
            ko, vo = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(2))
            merged = torch.zeros(5, dtype=torch.int64, device=dev)

            def call():
                ctx.compaction_merge_dev(runs, keys, ko, values, vo, merged, policy=dlsm_amd.MERGE_KEEP_ALL)

            def torch_path():
                idx = torch.sort(sortkey, stable=True).indices
                return allk[idx], allv[idx]

            call()
            ctx.sync()
            tk, tv = torch_path()
            assert merged.cpu().tolist() == [n, n, n * KEY, n * vlen, 0], merged
            assert torch.equal(keys, tk.reshape(-1)) and torch.equal(values, tv.reshape(-1)), "the merge's bytes differ"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            total, parts, tor = [], [], []
            for _ in range(args.reps):
                e0.record(stream)
                call()
                e1.record(stream)
                ctx.sync()
                total.append(e0.elapsed_time(e1))
                parts.append(ctx.compaction_merge_stats()[0])
                e0.record(stream)
                torch_path()
                e1.record(stream)
                ctx.sync()
                tor.append(e0.elapsed_time(e1))
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                hk = np.concatenate([m[0].cpu().numpy() for m in made])
                hv = np.concatenate([v.cpu().numpy() for v in vals])
                order = np.argsort(hk.view(f"S{KEY}").reshape(-1), kind="stable")  # (fixed trailers per run: bytes order suffices)
                ok, ov = torch.from_numpy(hk[order]).to(dev), torch.from_numpy(hv[order]).to(dev)
                torch.cuda.synchronize(dev)
                host.append((time.perf_counter() - t0) * 1e3)
            launch = dict(zip(("record", "partition", "merge", "decide", "offsets", "gather"),
                              (statistics.median(p[j] for p in parts) for j in range(6))))
            call_ms = statistics.median(total)
            floor_ms = 2 * n * (KEY + vlen) / rate / 1e6
            res["legs"].append({"case": name, "runs": len(spec), "n": n, "value_len": vlen, "call_ms": call_ms,
                                "call_best_ms": min(total), "launch_ms": launch, "passes": ctx.compaction_merge_stats()[1],
                                "pass_share": (launch["partition"] + launch["merge"]) / sum(launch.values()),
                                "floor_ms": floor_ms, "call_over_floor": call_ms / floor_ms,
                                "torch_ms": statistics.median(tor), "torch_over_call": statistics.median(tor) / call_ms,
                                "host_ms": statistics.median(host), "host_over_call": statistics.median(host) / call_ms})
            del vals, allv, keys, values, tk, tv, ok, ov
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
