"""The table build (dlsm_table_build_dev): the data region, chunk ends and sealed
index block of a flush from keys and values that are on the device.

Legs: n = 153,846 pairs (one memtable flush, db/memtable.h:7) and 1.6 M, 28-byte
internal keys of db_bench user keys, values of 100 and 400 bytes, chunk_bytes 0
and 1 MiB.  Timed with device events on one stream, warm, medians of --reps:
  call     dlsm_table_build_dev, and each of its launches (size, offsets, region
           with the chunk chain, index, seal) from the events the library
           records around them (dlsm_table_build_stats)
  floor    keys + values read and region + index block written, over the copy
           rate dlsm_stream_kernel kind 1 reaches in the same process
  host     what a device-resident table costs without the build: data_region.py's
           and index_block.py's numpy writers on the same arrays on the host
           (host clock), plus the copy of their outputs to the device
The chunk chain's cost is the region launch with chunk_bytes 1 MiB against the
same launch with one chunk.  The outputs are compared with the numpy writers
before timing.  Prints one JSON line; --out writes it.

    python scripts/bench_table_build.py [--reps 20] [--out profiles/table_build.json]
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

KEY = 28


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[153_846, 1_600_000])
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np
    import torch

    import dlsm_amd
    from bench_read_plan import copy_rate
    from dlsm_amd import data_region as dr
    from dlsm_amd import index_block as ib
    from dlsm_amd import workload as W

    dev = torch.device("cuda", 0)
    ctx = dlsm_amd.Context(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    res = {"reps": args.reps, "chunk": dlsm_amd.table_build_chunk(), "span": dlsm_amd.table_build_span(),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "legs": []}
    rate = copy_rate(dev, stream, 2_000_000_000)
    res["copy_GBps"] = rate
    trailer = torch.tensor(list(((9 << 8) | 1).to_bytes(8, "little")), dtype=torch.uint8, device=dev)
    for n in args.sizes:
        keys_t = torch.empty((n, KEY), dtype=torch.uint8, device=dev)
        keys_t[:, :20] = W.dbbench_keys_torch(torch.arange(n, dtype=torch.int64, device=dev) * 3).reshape(n, 20)
        keys_t[:, 20:] = trailer
        keys = dlsm_amd.Keys(keys_t.reshape(-1), n, KEY)
        for vlen in (100, 400):
            vals = torch.randint(0, 256, (n, vlen), dtype=torch.uint8, device=dev, generator=gen)
            need_d, need_i = dlsm_amd.table_build_bound(n, n * KEY, n * vlen)
            data = torch.empty(need_d, dtype=torch.uint8, device=dev)
            index = torch.empty(need_i, dtype=torch.uint8, device=dev)
            ce = torch.zeros(need_d // (1 << 20) * 2 + 8, dtype=torch.int64, device=dev)
            built = torch.zeros(4, dtype=torch.int64, device=dev)
            # the host baseline, and the bytes to compare with
            hk, hv = keys_t.cpu().numpy(), vals.cpu().numpy()
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                region, offs, sizes = dr.build_region_fixed(hk, hv)
                block = np.frombuffer(ib.build_index_block_fixed(hk, offs, sizes), dtype=np.uint8)
                t1 = time.perf_counter()
                rd, bd = torch.from_numpy(region).to(dev), torch.from_numpy(block).to(dev)
                torch.cuda.synchronize(dev)
                host.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
            for cb in (0, 1 << 20):
                def call():
                    ctx.table_build_dev(keys, vals.reshape(-1), data, index, ce, built, value_len=vlen, chunk_bytes=cb)
                call()
                ctx.sync()
                b = built.cpu().numpy().view(np.uint64).tolist()
                assert b[0] == region.size and b[1] == block.size and b[3] == 0, b
                assert torch.equal(data[:b[0]], rd) and torch.equal(index[:b[1]], bd), "the build's bytes differ"
                ends = ce.cpu().numpy().view(np.uint64)[:b[2]]
                pair = 8 + KEY + vlen
                assert ends[-1] == b[0] and (cb == 0 or (np.diff(ends)[:-1] == (cb // pair) * pair).all())
                total, parts = [], []
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(args.reps):
                    e0.record(stream)
                    call()
                    e1.record(stream)
                    ctx.sync()
                    total.append(e0.elapsed_time(e1))
                    parts.append(ctx.table_build_stats()[0])
                moved = n * (KEY + vlen) + b[0] + b[1]
                leg = {"n": n, "value_len": vlen, "chunk_bytes": cb, "n_chunks": b[2], "data_bytes": b[0], "index_bytes": b[1],
                       "call_ms": statistics.median(total), "call_best_ms": min(total),
                       "launch_ms": dict(zip(("size", "offsets", "region", "index", "seal"),
                                             (statistics.median(p[j] for p in parts) for j in range(5)))),
                       "floor_ms": moved / rate / 1e6,
                       "host_build_ms": statistics.median(h[0] for h in host), "host_h2d_ms": statistics.median(h[1] for h in host)}
                res["legs"].append(leg)
            del vals, data, index, rd, bd
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
