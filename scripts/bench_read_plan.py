"""Read plan of a batched Get (dlsm_version_read_plan_dev) on the version of
scripts/bench_version_probe.py: db_bench's final state at config 5 (4 + 5 + 40
+ 377 = 426 files), 100 M uniform lookups, half of which miss every file.

Per mode (FIRST: each Get's next file; ALL: every file) it times, in
interleaved rounds on one stream with device events:
  probe        dlsm_version_probe_dev alone (slot masks + level picks)
  plan         dlsm_version_read_plan_dev alone, on the probe's output
  probe+plan   the two back to back: the cost added per batch
  torch_sort   torch's stable sort of the same per-task file ids (int32, in Get
               order) on the same device -- the sort alone, without the gather
               of Get indices a caller would still need
and once per round the device-to-host copy of the masks and picks (28 B per
Get into page-locked memory): what bucketing on the host would start with.
The plan's byte model (read_plan.hip) over the copy rate dlsm_stream_kernel
kind 1 reaches in the same process gives the floor the plan is compared with.
The plan of the first --check Gets is compared with a numpy restatement, the
full plans with torch's sorted order.  Prints one JSON line; --out writes it.

    python scripts/bench_read_plan.py [--lookups 100000000] [--rounds 5] [--out profiles/read_plan.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def numpy_plan(files, mask, lf, first):
    """The contract restated: (Get, file) pairs Get by Get, slot by slot, stable-sorted by file."""
    import numpy as np

    l0 = sorted((j for j, f in enumerate(files) if f.level == 0), key=lambda j: -files[j].number)
    lv = [np.array([j for j, f in enumerate(files) if f.level == level], dtype=np.int64) for level in range(1, 6)]
    if first:
        mask = mask & (~mask + np.uint64(1))
    gets, fids, slots = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for s in range(len(l0) + 5):
        g = np.nonzero((mask >> np.uint64(s)) & np.uint64(1))[0]
        if g.size == 0:
            continue
        gets.append(g)
        fids.append(np.full(g.size, l0[s]) if s < len(l0) else lv[s - len(l0)][lf[g, s - len(l0)].astype(np.int64)])
        slots.append(np.full(g.size, s))
    gets, fids, slots = np.concatenate(gets), np.concatenate(fids), np.concatenate(slots)
    o = np.lexsort((slots, gets))
    gets, fids = gets[o], fids[o]
    o = np.argsort(fids, kind="stable")
    begin = np.zeros(len(files) + 1, dtype=np.uint64)
    begin[1:] = np.cumsum(np.bincount(fids, minlength=len(files)))
    return begin, gets[o].astype(np.uint32)


def task_ids(files, mask, lf, first, dev):
    """Per-task (Get, file id, is a level task) on the device, Get by Get: the
    input torch's sort gets."""
    import numpy as np
    import torch

    l0 = sorted((j for j, f in enumerate(files) if f.level == 0), key=lambda j: -files[j].number)
    lv = [torch.tensor([j for j, f in enumerate(files) if f.level == level], dtype=torch.int32, device=dev)
          for level in range(1, 6)]
    m = mask & (-mask) if first else mask
    gets, fids, level_tasks = [], [], 0
    for s in range(len(l0) + 5):
        g = torch.nonzero((m >> s) & 1).flatten()
        if g.numel() == 0:
            continue
        if s < len(l0):
            f = torch.full((g.numel(),), l0[s], dtype=torch.int32, device=dev)
        else:
            f = lv[s - len(l0)][lf[g, s - len(l0)].long()]
            level_tasks += int(g.numel())
        gets.append(g.to(torch.int32))
        fids.append(f)
    gets, fids = torch.cat(gets), torch.cat(fids)
    o = torch.sort(gets, stable=True).indices  # Get by Get; a Get's tasks stay in slot order
    return gets[o].contiguous(), fids[o].contiguous(), level_tasks


def copy_rate(dev, stream, nbytes, reps=5):
    """Best GB/s (read + written) of dlsm_stream_kernel kind 1 over its shapes."""
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
    ap.add_argument("--lookups", type=int, default=100_000_000)
    ap.add_argument("--space", type=int, default=100_000_000, help="key space V")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--check", type=int, default=1_000_000, help="Gets whose plan is compared with numpy")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dlsm_amd
    from dlsm_amd import workload as W

    dev = torch.device("cuda", 0)
    ctx = dlsm_amd.Context(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    V, Q = args.space, args.lookups
    files = W.dbbench_version(ctx, dev, V)
    ver = ctx.version(files, on_device=True)
    n_files = len(files)
    rng = np.random.default_rng(12)
    qv = torch.from_numpy(rng.integers(0, 2 * V, Q, dtype=np.int64)).to(dev)
    qk = dlsm_amd.Keys(W.dbbench_keys_torch(qv), Q, 20)
    del qv
    mask = torch.zeros(Q, dtype=torch.int64, device=dev)
    lf = torch.zeros((Q, 5), dtype=torch.int32, device=dev)
    snap = (1 << 56) - 1
    begin = torch.zeros(n_files + 1, dtype=torch.int64, device=dev)
    dropped = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.version_probe_dev(ver, qk, snap, mask, lf)
    ctx.sync()

    res = {"what": "read plan of a batched Get (probe answers grouped by file), device-resident",
           "files": n_files, "lookups": Q, "chunk": dlsm_amd.read_plan_chunk(), "rounds": args.rounds,
           "reps": args.reps, "modes": {}}
    res["copy_gb_s"] = copy_rate(dev, stream, 2_000_000_000)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def probe():
        ctx.version_probe_dev(ver, qk, snap, mask, lf)

    # the numpy check on the first --check Gets, both modes
    nc = min(args.check, Q)
    hm = mask[:nc].cpu().numpy().view(np.uint64)
    hl = lf[:nc].cpu().numpy().view(np.uint32)
    for name, mode in (("first", dlsm_amd.PLAN_FIRST), ("all", dlsm_amd.PLAN_ALL)):
        wb, wg = numpy_plan(files, hm, hl, mode == dlsm_amd.PLAN_FIRST)
        g = torch.full((max(1, len(wg)),), -1, dtype=torch.int32, device=dev)
        ctx.version_read_plan_dev(ver, mask[:nc], lf[:nc], mode, begin, g, dropped)
        ctx.sync()
        ok = (np.array_equal(begin.cpu().numpy().view(np.uint64), wb) and
              np.array_equal(g.cpu().numpy().view(np.uint32)[:len(wg)], wg) and int(dropped.cpu()[0]) == 0)
        res["modes"][name] = {"numpy_checked": nc, "matches_numpy": bool(ok)}

    hmask = torch.empty(Q, dtype=torch.int64, pin_memory=True)
    hlf = torch.empty((Q, 5), dtype=torch.int32, pin_memory=True)

    def d2h():
        hmask.copy_(mask, non_blocking=True)
        hlf.copy_(lf, non_blocking=True)

    legs = {}
    setup = {}
    for name, mode in (("first", dlsm_amd.PLAN_FIRST), ("all", dlsm_amd.PLAN_ALL)):
        tg, tf, level_tasks = task_ids(files, mask, lf, mode == dlsm_amd.PLAN_FIRST, dev)
        T = int(tf.numel())
        gets = torch.full((max(T, 1),), -1, dtype=torch.int32, device=dev)
        setup[name] = (mode, tg, tf, gets, T, level_tasks)

        def plan(mode=mode, gets=gets):
            ctx.version_read_plan_dev(ver, mask, lf, mode, begin, gets, dropped)

        # warm-up of every shape, and the full-size check against torch's sorted order
        plan()
        order = torch.sort(tf, stable=True).indices
        ctx.sync()
        same = bool(torch.equal(tg[order], gets[:T])) and int(begin[-1].item()) == T and int(dropped.item()) == 0
        cnt = torch.bincount(tf.long(), minlength=n_files)
        same = same and bool(torch.equal(torch.cumsum(cnt, 0), begin[1:]))
        res["modes"][name].update({"tasks": T, "level_tasks": level_tasks, "matches_torch_sort_order": same})
        del order
        legs[name] = {"plan": [], "probe_plan": [], "torch_sort": []}
    legs["probe"], legs["d2h"] = [], []
    for _ in range(args.rounds):
        legs["probe"].append(timed(probe))
        for name in ("first", "all"):
            mode, tg, tf, gets, T, _ = setup[name]

            def plan(mode=mode, gets=gets):
                ctx.version_read_plan_dev(ver, mask, lf, mode, begin, gets, dropped)

            def both():
                probe()
                plan()

            legs[name]["plan"].append(timed(plan))
            legs[name]["probe_plan"].append(timed(both))
            legs[name]["torch_sort"].append(timed(lambda tf=tf: torch.sort(tf, stable=True)))
        legs["d2h"].append(timed(d2h))

    def stat(xs):
        return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}

    res["probe"] = stat(legs["probe"])
    res["d2h_masks_and_picks"] = dict(stat(legs["d2h"]), bytes=28 * Q)
    for name in ("first", "all"):
        mode, _, _, _, T, level_tasks = setup[name]
        r = res["modes"][name]
        for leg in ("plan", "probe_plan", "torch_sort"):
            r[leg] = stat(legs[name][leg])
        # byte model (read_plan.hip): FIRST: mask + pick, id written, id read, Get index written;
        # ALL: masks + picks read by both launches, Get index written.  Picks: the 4-B word alone
        # (the floor) and the whole 20-B row (what the sectors around it may cost).
        if mode == dlsm_amd.PLAN_FIRST:
            lo, hi = 8 * Q + 4 * level_tasks + 8 * Q + 4 * T, 8 * Q + 20 * Q + 8 * Q + 4 * T
        else:
            lo, hi = 2 * (8 * Q + 4 * level_tasks) + 4 * T, 2 * (8 * Q + 20 * Q) + 4 * T
        floor = lo / (res["copy_gb_s"] * 1e9) * 1e3
        r.update({"model_bytes": lo, "model_bytes_whole_pick_rows": hi, "floor_ms": round(floor, 3),
                  "floor_ms_whole_pick_rows": round(hi / (res["copy_gb_s"] * 1e9) * 1e3, 3),
                  "plan_over_floor": round(r["plan"]["median_ms"] / floor, 2),
                  "torch_sort_over_plan": round(r["torch_sort"]["median_ms"] / r["plan"]["median_ms"], 2),
                  "added_per_batch_ms": round(r["probe_plan"]["median_ms"] - res["probe"]["median_ms"], 3)})
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
