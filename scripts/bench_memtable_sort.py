"""The memtable sort (dlsm_memtable_sort_dev): one batch of pairs in arrival
order on the device into a sorted run in the table build's input form.

Legs, 28-byte internal keys (20-byte user keys -- db_bench's 16 digits and 4
fixed bytes -- drawn with repeats, a sequence per pair), KEEP_ALL (every byte
moves), shuffled:
  flush    153,846 pairs (one flush), values of 100 and of 400 bytes
  merge    1.69 M pairs (the compaction merge benchmark's largest input), both
  var      153,846 pairs, user keys of 17 to 23 bytes sharing their first 16
           (the comparator's byte path), values of 100 bytes
Timed with device events on one stream, warm, the forms alternating in one
process, medians of --reps with the best and the worst beside them:
  call     dlsm_memtable_sort_dev, and its launch kinds (tile sort in the record
           slot, partition, merge, decide, offsets, gather) from the events the
           library records (dlsm_compaction_merge_stats); each kind's bytes (what
           the launch must read and write, from the shapes) over the copy rate
           dlsm_stream_kernel kind 1 reaches in the same process is its floor,
           over_floor the kind's time over it (the partition reads a few records
           per tile: no floor)
  torch    what a caller has without the call: torch.sort (stable) of an int64
           of the decoded user key and trailer it is handed for free, plus index
           gathers of keys and values, on the same device
  host     dlsm_memtable_sort on the same batch in host memory (host clock,
           no transfer counted)
The call's keys, values and src are compared with the torch baseline's before
timing.  Prints one JSON line; --out writes it.

    python scripts/bench_memtable_sort.py [--reps 20] [--out profiles/memtable_sort.json]
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

FLUSH, MERGE, KEY = 153_846, 1_692_306, 28
KINDS = ("record", "partition", "merge", "decide", "offsets", "gather")


def launch_bytes(n, key_bytes, value_bytes, variable, passes):
    """Bytes each launch kind must move, from the shapes: 32-byte records, 8-byte lengths, offsets and sources."""
    return {"record": key_bytes + (16 * n if variable else 0) + 32 * n, "partition": None, "merge": 64 * n * passes,
            "decide": 32 * n + 16 * n, "offsets": 48 * n + 56 * n, "gather": 2 * (key_bytes + value_bytes) + 32 * n}


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
    gen.manual_seed(23)
    res = {"reps": args.reps, "tile": dlsm_amd.sort_tile(),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "legs": []}
    rate = copy_rate(dev, stream, 2_000_000_000)
    res["copy_GBps"] = rate

    def fixed_batch(n):
        """Shuffled user keys of 16 digits + 4 fixed bytes, with repeats, sequence j + 1 for pair j; also the int64 sort key."""
        num = torch.randint(0, 4 * n, (n,), device=dev, generator=gen)
        seq = torch.arange(1, n + 1, device=dev)
        digits = (num[:, None] // (10 ** torch.arange(15, -1, -1, device=dev, dtype=torch.int64))[None, :]) % 10 + 48
        k = torch.full((n, KEY), 120, dtype=torch.uint8, device=dev)
        k[:, :16] = digits.to(torch.uint8)
        trailer = seq << 8 | 1
        k[:, 20:] = ((trailer[:, None] >> (8 * torch.arange(8, device=dev))[None, :]) & 255).to(torch.uint8)
        return k.reshape(-1), None, num << 22 | ((1 << 22) - 1 - seq)  # ascending: number, then sequence descending

    def variable_batch(n):
        """16 shared bytes + 1 to 7 decimal digits: bytes order is the digits' order left-aligned."""
        rng = np.random.default_rng(23)
        num = rng.integers(0, 10 ** 7, n)
        iks = [b"sixteen-byte-pfx" + b"%d" % x + int((j + 1) << 8 | 1).to_bytes(8, "little") for j, x in enumerate(num)]
        off = np.concatenate([[0], np.cumsum([len(k) for k in iks])]).astype(np.int64)
        lex = np.array([sum((int(c) - 47) * 11 ** (6 - i) for i, c in enumerate(b"%d" % x)) for x in num], dtype=np.int64)
        sortkey = lex << 22 | ((1 << 22) - 1 - np.arange(1, n + 1))
        return (torch.from_numpy(np.frombuffer(b"".join(iks), dtype=np.uint8).copy()).to(dev), torch.from_numpy(off).to(dev),
                torch.from_numpy(sortkey).to(dev))

    legs = [("flush", FLUSH, 100, fixed_batch), ("flush", FLUSH, 400, fixed_batch), ("merge", MERGE, 100, fixed_batch),
            ("merge", MERGE, 400, fixed_batch), ("var", FLUSH, 100, variable_batch)]
    for name, n, vlen, make in legs:
        kbytes, koff, sortkey = make(n)
        kb, vb = kbytes.numel(), n * vlen
        vals = torch.randint(0, 256, (n, vlen), dtype=torch.uint8, device=dev, generator=gen)
        batch = (dlsm_amd.Keys(kbytes, n, 0 if koff is not None else KEY, koff), vals.reshape(-1), None, vlen)
        keys, values = (torch.empty(w, dtype=torch.uint8, device=dev) for w in (kb, vb))
        ko, vo, src = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(3))
        merged = torch.zeros(5, dtype=torch.int64, device=dev)
        klen = (koff[1:] - koff[:-1]) if koff is not None else None

        def call():
            ctx.memtable_sort_dev(batch, keys, ko, values, vo, merged, src=src, policy=dlsm_amd.MERGE_KEEP_ALL)

        def torch_path():
            idx = torch.sort(sortkey, stable=True).indices
            if koff is None:
                return idx, kbytes.reshape(n, KEY)[idx].reshape(-1), vals[idx]
            ln = klen[idx]  # a gather of variable-length keys: byte t of the output belongs to item j, at t - start[j]
            start = torch.cumsum(ln, 0) - ln
            item = torch.repeat_interleave(torch.arange(n, device=dev), ln)
            return idx, kbytes[koff[idx][item] + torch.arange(kb, device=dev) - start[item]], vals[idx]

        call()
        ctx.sync()
        ti, tk, tv = torch_path()
        assert merged.cpu().tolist() == [n, n, kb, vb, 0], merged
        assert torch.equal(keys, tk) and torch.equal(values, tv.reshape(-1)) and torch.equal(src[:n], ti), "the sort differs"
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
        hb = (dlsm_amd.Keys(kbytes.cpu().numpy(), n, 0 if koff is not None else KEY,
                            None if koff is None else koff.cpu().numpy().view(np.uint64)), vals.cpu().numpy().reshape(-1), None, vlen)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            dlsm_amd.memtable_sort(hb, dlsm_amd.MERGE_KEEP_ALL)
            host.append((time.perf_counter() - t0) * 1e3)
        passes = ctx.compaction_merge_stats()[1]
        launch = {k: statistics.median(p[j] for p in parts) for j, k in enumerate(KINDS)}
        floors = {k: None if b is None else b / rate / 1e6 for k, b in launch_bytes(n, kb, vb, koff is not None, passes).items()}
        call_ms, torch_ms = statistics.median(total), statistics.median(tor)
        res["legs"].append({"case": name, "n": n, "value_len": vlen, "key_bytes": kb, "passes": passes, "launches": 2 * passes + 4,
                            "call_ms": call_ms, "call_best_ms": min(total), "call_worst_ms": max(total), "launch_ms": launch,
                            "floor_ms": floors, "over_floor": {k: None if f is None else launch[k] / f for k, f in floors.items()},
                            "torch_ms": torch_ms, "torch_best_ms": min(tor), "torch_worst_ms": max(tor),
                            "torch_over_call": torch_ms / call_ms, "host_ms": statistics.median(host),
                            "host_over_call": statistics.median(host) / call_ms})
        del vals, keys, values, tk, tv, ti, hb
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
