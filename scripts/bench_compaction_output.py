"""The compaction output (dlsm_compaction_output_dev): a merged run on the device
cut into size-capped tables, all built in one call.

Workload: the L0 -> L1 merge of DESIGN §7, 1.69 M pairs of 28-byte internal keys
(db_bench user keys) with 100- and 400-byte values, chunk_bytes 1 MiB, cut at the
file sizes that give about 12 and about 100 files.  The run is given as the merge
leaves it (key_off / value_off arrays: the searching region write) and, for the
region launch alone, as fixed lengths (the specialised region write).
Timed warm, medians of --reps:
  call      dlsm_compaction_output_dev end to end (host clock around the call
            and the stream's drain) and each launch kind from the events the
            library records (dlsm_compaction_output_stats)
  baseline  what a caller has without it: drain the stream, read `merged` and
            the two offset arrays, find the cuts on the host, one
            dlsm_table_build_dev per file; host clock, drained
  floor     per write pass, its own bytes (read + written) over the copy rate
            dlsm_stream_kernel kind 1 reaches in the same process
The call's bytes are compared with the baseline's before timing.  Prints one
JSON line; --out writes it.

    python scripts/bench_compaction_output.py [--reps 20] [--out profiles/compaction_output.json]
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

KEY, CHUNK = 28, 1 << 20
KINDS = ("size", "offsets", "cut", "entries", "region", "index", "seal")


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
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    n = args.n
    res = {"reps": args.reps, "n": n, "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "legs": []}
    rate = copy_rate(dev, stream, 2_000_000_000)
    res["copy_GBps"] = rate
    keys_t = torch.empty((n, KEY), dtype=torch.uint8, device=dev)
    keys_t[:, :20] = W.dbbench_keys_torch(torch.arange(n, dtype=torch.int64, device=dev) * 3).reshape(n, 20)
    keys_t[:, 20:] = torch.tensor(list(((9 << 8) | 1).to_bytes(8, "little")), dtype=torch.uint8, device=dev)
    kflat = keys_t.reshape(-1)
    ko = torch.arange(n + 1, dtype=torch.int64, device=dev) * KEY
    merged = torch.tensor([n, n, n * KEY, 0, 0], dtype=torch.int64, device=dev)
    med = statistics.median
    for vlen in (100, 400):
        vals = torch.randint(0, 256, (n * vlen,), dtype=torch.uint8, device=dev, generator=gen)
        vo = torch.arange(n + 1, dtype=torch.int64, device=dev) * vlen
        total = n * (8 + KEY + vlen)
        for want_files in (12, 100):
            mfb = total // want_files
            caps = dlsm_amd.compaction_output_bound(n, n * KEY, n * vlen, mfb, CHUNK)
            data, index = (torch.empty(c, dtype=torch.uint8, device=dev) for c in caps[:2])
            ce, files = torch.zeros(caps[2], dtype=torch.int64, device=dev), torch.zeros(9 * caps[3], dtype=torch.int64, device=dev)
            built = torch.zeros(5, dtype=torch.int64, device=dev)
            bdata, bindex = torch.empty_like(data), torch.empty_like(index)
            bce = torch.zeros(caps[2] + 2 * caps[3] + 8, dtype=torch.int64, device=dev)
            bbuilt = torch.zeros(4 * caps[3], dtype=torch.int64, device=dev)

            def call(fixed=False):
                if fixed:
                    ctx.compaction_output_dev(dlsm_amd.Keys(kflat, n, KEY), vals, merged, data, index, ce, files, built,
                                              value_len=vlen, max_file_bytes=mfb, chunk_bytes=CHUNK)
                else:
                    ctx.compaction_output_dev(dlsm_amd.Keys(kflat, n, 0, ko), vals, merged, data, index, ce, files, built,
                                              value_off=vo, max_file_bytes=mfb, chunk_bytes=CHUNK)

            def baseline():
                """Returns the (first, n, data base, index base, chunk base) it built."""
                ctx.sync()
                m = merged.cpu().numpy()
                n_out = int(m[1])
                off = ko[:n_out + 1].cpu().numpy() + vo[:n_out + 1].cpu().numpy() + 8 * np.arange(n_out + 1)
                out, at, db, xb, cb, f = [], 0, 0, 0, 0, 0
                while at < n_out:
                    e = int(np.searchsorted(off, off[at] + mfb, side="left"))
                    e = min(max(e, at + 1), n_out)
                    nbytes = int(off[e] - off[at])
                    ctx.table_build_dev(dlsm_amd.Keys(kflat, e - at, 0, ko[at:]), vals, bdata[db:], bindex[xb:], bce[cb:],
                                        bbuilt[4 * f:], value_off=vo[at:], chunk_bytes=CHUNK)
                    out.append((at, e - at, db, xb, cb))
                    # the host knows the region's length; the block's and the chunk count it bounds
                    db += (nbytes + 15) & ~15
                    xb += (dlsm_amd.table_build_bound(e - at, (e - at) * KEY, 0)[1] + 15) & ~15
                    cb += 2 * (nbytes // CHUNK) + 2
                    at, f = e, f + 1
                ctx.sync()
                return out

            call()
            ctx.sync()
            b = built.cpu().numpy().tolist()
            recs = files.cpu().numpy().reshape(-1, 9)[:b[0]]
            base = baseline()
            bb = bbuilt.cpu().numpy().reshape(-1, 4)
            assert b[4] == 0 and len(base) == b[0], (b, len(base))
            for r, (at, fn, db, xb, cb), t in zip(recs, base, bb):
                assert (r[0], r[1], r[3], r[5], r[7]) == (at, fn, t[0], t[1], t[2]), (r, t)
                assert torch.equal(data[r[2]:r[2] + r[3]], bdata[db:db + t[0]]), "region bytes differ"
                assert torch.equal(index[r[4]:r[4] + r[5]], bindex[xb:xb + t[1]]), "index bytes differ"
                assert torch.equal(ce[r[6]:r[6] + r[7]], bce[cb:cb + t[2]]), "chunk ends differ"
            snap = data.clone()
            call(fixed=True)
            ctx.sync()
            assert torch.equal(data, snap), "the fixed-length region write differs"
            wall, parts, fixed_parts, base_ms = [], [], [], []
            for _ in range(args.reps):
                ctx.sync()
                t0 = time.perf_counter()
                call()
                ctx.sync()
                wall.append((time.perf_counter() - t0) * 1e3)
                parts.append(ctx.compaction_output_stats()[0])
                call(fixed=True)
                ctx.sync()
                fixed_parts.append(ctx.compaction_output_stats()[0])
                t0 = time.perf_counter()
                baseline()
                base_ms.append((time.perf_counter() - t0) * 1e3)
            launch = {k: med(p[j] for p in parts) for j, k in enumerate(KINDS)}
            region_bytes, index_bytes = n * (KEY + vlen) + b[1], n * KEY + b[2]
            leg = {"value_len": vlen, "max_file_bytes": mfb, "n_files": b[0], "n_chunks": b[3], "data_bytes": b[1],
                   "index_bytes": b[2], "call_wall_ms": med(wall), "call_device_ms": sum(launch.values()),
                   "launch_ms": launch, "region_fixed_ms": med(p[4] for p in fixed_parts),
                   "baseline_wall_ms": med(base_ms), "baseline_over_call": med(base_ms) / med(wall),
                   "region_floor_ms": region_bytes / rate / 1e6, "index_floor_ms": index_bytes / rate / 1e6,
                   "seal_floor_ms": b[2] / rate / 1e6}
            res["legs"].append(leg)
            del data, index, bdata, bindex, snap
        del vals
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
