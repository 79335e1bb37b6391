"""Opening a version from sealed, device-resident filter blocks.

The version is the one scripts/bench_version_probe.py probes (db_bench's final
state at config 5: 4 level-0 files + 5 / 40 / 377 files on levels 1-3, about
140 MB of filters), every filter sealed as FinishFilterBlock writes it
([filter][type 0][masked crc32c]).  Two ways to a verified dlsm_version, timed
in one process, interleaved, host wall time per call (both return
synchronised):

  (a) the stripped-filter entry points: dlsm_crc32c_dev over all blocks, the
      stored crcs fetched and compared on the host, then
      dlsm_version_create(filters_are_device=1) on the shortened lengths;
  (b) dlsm_version_create_blocks.

Also reports the ingest pass's bytes (read + written) over the time between
the events around its two launches (dlsm_block_open_stats), against the copy
ceiling dlsm_stream_kernel kind 1 reaches on this box at the same byte count
and at 1 GiB.  Prints one JSON line; --out also writes it to a file.

    python scripts/bench_block_open.py [--rounds 7] [--out profiles/block_open.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def copy_ceiling(dev, stream, nbytes, reps=5):
    """Best GB/s (read + written) of the library's copy kernel over its shapes."""
    import torch

    import dlsm_amd

    fn = dlsm_amd.lib().dlsm_stream_kernel
    nbytes = nbytes // 16 * 16
    src = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    raw = ctypes.c_void_p(stream.cuda_stream)
    best = 0.0
    for variant in range(4):
        for blocks in (1024, 2048, 4096):
            a = (raw, 1, variant, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                 ctypes.c_uint64(nbytes), ctypes.c_uint32(blocks))
            if fn(*a) != 0:
                raise RuntimeError("dlsm_stream_kernel failed")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn(*a)
            e1.record(stream)
            stream.synchronize()
            best = max(best, 2 * nbytes * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    return round(best, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--space", type=int, default=100_000_000, help="key space V")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--check", type=int, default=200_000, help="lookups compared between the two versions")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dlsm_amd
    from dlsm_amd import VersionFile
    from dlsm_amd import workload as W

    dev = torch.device("cuda", 0)
    ctx = dlsm_amd.Context(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    files = W.dbbench_version(ctx, dev, args.space)
    # seal every filter on the device: [filter][0][Fixed32(Mask(crc32c(filter || 0)))]
    blocks = [torch.cat([f.filter, torch.zeros(5, dtype=torch.uint8, device=dev)]) for f in files]
    crcs = ctx.crc32c_dev([b[:-4] for b in blocks])
    trailers = np.zeros((len(blocks), 5), dtype=np.uint8)
    for j, c in enumerate(crcs):
        trailers[j, 1:] = np.frombuffer(dlsm_amd.crc32c_mask(c).to_bytes(4, "little"), dtype=np.uint8)
    td = torch.from_numpy(trailers).to(dev)
    for j, b in enumerate(blocks):
        b[-5:] = td[j]
    stream.synchronize()
    sealed = [VersionFile(f.level, f.number, f.smallest, f.largest, f.largest_trailer, b)
              for f, b in zip(files, blocks)]
    block_bytes = sum(int(b.numel()) for b in blocks)

    def path_a():
        got = ctx.crc32c_dev([b[:-4] for b in blocks])
        stored = torch.stack([b[-5:] for b in blocks]).cpu().numpy()
        for j, c in enumerate(got):
            if stored[j, 0] != 0 or int.from_bytes(stored[j, 1:].tobytes(), "little") != dlsm_amd.crc32c_mask(c):
                raise RuntimeError(f"block {j} fails its checks")
        stripped = [VersionFile(f.level, f.number, f.smallest, f.largest, f.largest_trailer, f.filter[:-5])
                    for f in sealed]
        return ctx.version(stripped, on_device=True)

    def path_b():
        return ctx.version(sealed, on_device=True, sealed=True)

    times = {"a": [], "b": []}
    ingest = []
    for r in range(args.rounds + 1):  # round 0 warms both paths up and is dropped
        for name, fn in (("a", path_a), ("b", path_b)) if r % 2 == 0 else (("b", path_b), ("a", path_a)):
            stream.synchronize()
            t0 = time.perf_counter()
            v = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if name == "b":
                rd, wr, ms = ctx.block_open_stats()
                if r:
                    ingest.append((rd + wr) / (ms * 1e-3) / 1e9)
            if r:
                times[name].append(dt)
            v.close()

    res = {"what": "verified version open from sealed device-resident filter blocks",
           "files_per_level": [4, 5, 40, 377, 0, 0], "blocks": len(blocks), "block_bytes": block_bytes,
           "rounds": args.rounds}
    for name, label in (("a", "a_crc32c_dev_host_compare_version_create"), ("b", "b_version_create_blocks")):
        res[label] = {"median_ms": round(statistics.median(times[name]), 3), "min_ms": round(min(times[name]), 3)}
    res["b_not_above_a"] = statistics.median(times["b"]) <= statistics.median(times["a"])
    rd, wr, ms = ctx.block_open_stats()
    res["ingest"] = {"bytes_read": rd, "bytes_written": wr, "launches_ms_last": round(ms, 4),
                     "GBs_median": round(statistics.median(ingest), 1), "GBs_best": round(max(ingest), 1)}
    res["copy_ceiling_GBs"] = {"same_bytes": copy_ceiling(dev, stream, block_bytes),
                               "1GiB": copy_ceiling(dev, stream, 1 << 30)}
    # the same pass without the crc (verify_checksums = 0: copy, type check and
    # parse only): what the kernel's loads and stores cost on their own
    nocrc = []
    for r in range(args.rounds + 1):
        v = ctx.version(sealed, on_device=True, sealed=True, verify_checksums=False)
        rd0, wr0, ms0 = ctx.block_open_stats()
        if r:
            nocrc.append((rd0 + wr0) / (ms0 * 1e-3) / 1e9)
        v.close()
    res["ingest_no_crc"] = {"bytes_read": rd0, "bytes_written": wr0, "launches_ms_last": round(ms0, 4),
                            "GBs_median": round(statistics.median(nocrc), 1)}
    res["ingest"]["frac_of_copy_same_bytes"] = round(res["ingest"]["GBs_median"] / res["copy_ceiling_GBs"]["same_bytes"], 3)
    res["ingest"]["frac_of_copy_1GiB"] = round(res["ingest"]["GBs_median"] / res["copy_ceiling_GBs"]["1GiB"], 3)
    if args.check:
        rng = np.random.default_rng(5)
        n = args.check
        qv = torch.from_numpy(rng.integers(0, 2 * args.space, n, dtype=np.int64)).to(dev)
        qk = dlsm_amd.Keys(W.dbbench_keys_torch(qv), n, 20)
        masks = []
        for fn in (path_a, path_b):
            v = fn()
            m = torch.zeros(n, dtype=torch.int64, device=dev)
            ctx.version_probe_dev(v, qk, (1 << 56) - 1, m)
            ctx.sync()
            masks.append(m.cpu().numpy())
            v.close()
        res["same_answers"] = bool(np.array_equal(masks[0], masks[1])) and bool(masks[0].any())
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
