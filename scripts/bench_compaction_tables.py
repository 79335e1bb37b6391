"""The compaction merge out of opened tables (dlsm_compaction_merge_tables_dev):
a compaction's inputs read straight from data regions and sealed index blocks.

The workload of bench_compaction_merge.py's l0-into-l1: one flush (153,846
pairs) merged into ten flushes' worth of level files, db_bench's 24-byte
internal keys, values of 100 and 400 bytes, KEEP_ALL (every byte moves).  Stored
as tables -- built by dlsm_table_build_dev in 8 MiB chunks and opened on the
device: 4 level-0 files of a quarter flush each and 10 flush-sized files of one
level.  Timed with device events on one stream, warm, medians of --reps, the
launch kinds from the events the library records (dlsm_compaction_merge_stats):
  packed     dlsm_compaction_merge_dev on pre-unpacked arrays of the same pairs
             as 5 runs: a lower bound for the tables call (it reads no index
             block and no header, and its caller paid for the unpacking), and
             the leg to compare across commits (--packed-only runs it alone)
  tables-5   the new call, MakeInputIterator's runs: each level-0 file, and the
             level's 10 files as one run
  tables-14  the new call, every file a run of its own
  record_floor_ms  the table record pass's bytes -- the index contents, each
             pair's header and key read once, a record and a descriptor written
             -- over the copy rate dlsm_stream_kernel kind 1 reaches
  host       dlsm_compaction_merge_tables over host copies (host clock, once)
The tables calls' keys and values are compared with the packed call's before
timing.  Prints one JSON line; --out writes it.

    python scripts/bench_compaction_tables.py [--reps 20] [--packed-only] [--out profiles/compaction_tables.json]
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

FLUSH, KEY, CHUNK = 153_846, 24, 8 << 20
KINDS = ("record", "partition", "merge", "decide", "offsets", "gather")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--packed-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
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
    res = {"reps": args.reps, "chunk": dlsm_amd.merge_chunk(), "tile": dlsm_amd.merge_tile(), "legs": []}
    rate = copy_rate(dev, stream, 2_000_000_000)
    res["copy_GBps"] = rate

    def make_file(n, lo, hi, seq):
        """n distinct sorted numbers of [lo, hi) as 16 decimal digits + trailer."""
        num = torch.randperm(hi - lo, device=dev, generator=gen)[:n].sort().values + lo
        digits = (num[:, None] // (10 ** torch.arange(15, -1, -1, device=dev, dtype=torch.int64))[None, :]) % 10 + 48
        k = torch.empty((n, KEY), dtype=torch.uint8, device=dev)
        k[:, :16] = digits.to(torch.uint8)
        k[:, 16:] = torch.tensor(list(((seq << 8) | 1).to_bytes(8, "little")), dtype=torch.uint8, device=dev)
        return k

    span = 40 * FLUSH
    spec = [(FLUSH // 4, 0, span, 5 - j) for j in range(4)] + [(FLUSH, j * span // 10, (j + 1) * span // 10, 1) for j in range(10)]
    fkeys = [make_file(*s) for s in spec]
    n = sum(s[0] for s in spec)

    def timed(call):
        call()
        ctx.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        total, parts = [], []
        for _ in range(args.reps):
            e0.record(stream)
            call()
            e1.record(stream)
            ctx.sync()
            total.append(e0.elapsed_time(e1))
            parts.append(ctx.compaction_merge_stats()[0])
        launch = {k: statistics.median(p[j] for p in parts) for j, k in enumerate(KINDS)}
        return {"call_ms": statistics.median(total), "call_best_ms": min(total), "call_worst_ms": max(total),
                "launch_ms": launch, "passes": ctx.compaction_merge_stats()[1]}

    for vlen in (100, 400):
        fvals = [torch.randint(0, 256, (s[0], vlen), dtype=torch.uint8, device=dev, generator=gen) for s in spec]
        out = lambda: ([torch.empty(n * w, dtype=torch.uint8, device=dev) for w in (KEY, vlen)] +  # noqa: E731
                       [torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(2)] +
                       [torch.zeros(5, dtype=torch.int64, device=dev)])
        pk, pv, pko, pvo, pm = out()
        level_k, level_v = torch.cat(fkeys[4:]), torch.cat(fvals[4:])
        packed = [(dlsm_amd.Keys(k.reshape(-1), k.shape[0], KEY), v.reshape(-1), None, vlen)
                  for k, v in list(zip(fkeys[:4], fvals[:4])) + [(level_k, level_v)]]
        leg = timed(lambda: ctx.compaction_merge_dev(packed, pk, pko, pv, pvo, pm, policy=dlsm_amd.MERGE_KEEP_ALL))
        assert pm.cpu().tolist() == [n, n, n * KEY, n * vlen, 0], pm
        res["legs"].append(dict(leg, case="packed", runs=5, n=n, value_len=vlen))
        if args.packed_only:
            continue
        blocks, files, index_bytes = [], [], 0
        for k, v in zip(fkeys, fvals):
            m = k.shape[0]
            d_cap, i_cap = dlsm_amd.table_build_bound(m, m * KEY, m * vlen)
            data, index = (torch.empty(c + 16, dtype=torch.uint8, device=dev) for c in (d_cap, i_cap))
            ce, built = torch.zeros(64, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
            ctx.table_build_dev(dlsm_amd.Keys(k.reshape(-1), m, KEY), v.reshape(-1), data, index, ce, built, value_len=vlen,
                                chunk_bytes=CHUNK)
            ctx.sync()
            b, ends = built.cpu().tolist(), [0] + ce.cpu().tolist()
            assert b[3] == 0 and b[2] <= 64, b
            blocks.append(index[:b[1]])
            files.append([data[ends[c]:ends[c + 1]] for c in range(b[2])])
            index_bytes += b[1] - 5
        ti, td = ctx.tableindex(blocks, on_device=True), ctx.tabledata(files, on_device=True)
        floor_ms = (index_bytes + n * (8 + KEY) + n * 48) / rate / 1e6
        for name, runs in (("tables-5", [[0], [1], [2], [3], list(range(4, 14))]), ("tables-14", [[f] for f in range(14)])):
            tk, tv, tko, tvo, tm = out()
            leg = timed(lambda: ctx.compaction_merge_tables_dev(ti, td, runs, tk, tko, tv, tvo, tm,
                                                                policy=dlsm_amd.MERGE_KEEP_ALL))
            assert tm.cpu().tolist() == [n, n, n * KEY, n * vlen, 0], tm
            assert torch.equal(tk, pk) and torch.equal(tv, pv), "the tables merge's bytes differ from the packed merge's"
            res["legs"].append(dict(leg, case=name, runs=len(runs), n=n, value_len=vlen, record_floor_ms=floor_ms,
                                    record_over_floor=leg["launch_ms"]["record"] / floor_ms))
            del tk, tv
        hb = [bytes(b.cpu().numpy()) for b in blocks]
        hf = [[bytes(c.cpu().numpy()) for c in f] for f in files]
        t0 = time.perf_counter()
        m = dlsm_amd.compaction_merge_tables(hb, hf, [[0], [1], [2], [3], list(range(4, 14))], dlsm_amd.MERGE_KEEP_ALL,
                                             keys_cap=n * KEY, values_cap=n * vlen, pair_cap=n)[5]
        res["legs"].append({"case": "host", "runs": 5, "n": n, "value_len": vlen, "call_ms": (time.perf_counter() - t0) * 1e3})
        assert m == (n, n, n * KEY, n * vlen, 0), m
        ti.close()
        td.close()
        del hb, hf, blocks, files
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
