#!/usr/bin/env python3
"""Time the host form of the range scan (dlsm_range_scan; no device is touched).

The set-up is scripts/bench_compaction_tables.py's shape scaled by --scale: 4
level-0 files plus 10 level files (5 runs), 28-byte internal keys, 100-byte
values; start keys uniform over the key space at a snapshot that hides the
newest level-0 file.  Prints one JSON line: scans, limit, pairs yielded and the
median wall time of --repeats calls.  There is no device form to compare with
yet."""
import argparse
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import dlsm_amd  # noqa: E402
from dlsm_amd.data_region import build_region  # noqa: E402
from dlsm_amd.index_block import build_index_block  # noqa: E402


def table(pairs):
    chunks, handles = build_region(pairs, 1 << 16)
    return build_index_block([k for k, _ in pairs], handles), chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.01, help="1.0: 1.69 M pairs")
    ap.add_argument("--scans", type=int, default=10000)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    per = max(int(153846 * a.scale), 16)
    space = 10 * per
    rng = np.random.default_rng(7)
    ikey = lambda x, seq: b"%020d" % x + struct.pack("<Q", seq << 8 | 1)  # noqa: E731
    value = bytes(100)
    files = [[(ikey(int(x), 200 + f), value) for x in np.sort(rng.choice(space, per // 4, replace=False))] for f in range(4)]
    files += [[(ikey(x, 100), value) for x in range(f * per, (f + 1) * per)] for f in range(10)]
    tables = [table(p) for p in files]
    runs = [[0], [1], [2], [3], list(range(4, 14))]
    starts = b"".join(b"%020d" % int(x) for x in rng.integers(0, space, a.scans))
    keys = dlsm_amd.Keys(np.frombuffer(starts, dtype=np.uint8).copy(), a.scans, 20)
    cap = a.scans * a.limit
    times, out = [], None
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = dlsm_amd.range_scan([t[0] for t in tables], [t[1] for t in tables], runs, keys, 202, a.limit,
                                  keys_cap=28 * cap, values_cap=100 * cap, pair_cap=cap)
        times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(pairs_in=sum(len(f) for f in files), scans=a.scans, limit=a.limit, pairs_out=out["scanned"][1],
                          flags=out["scanned"][4], host_ms=statistics.median(times))))


if __name__ == "__main__":
    main()
