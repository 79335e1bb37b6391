"""The batched index seek (dlsm_index_seek_dev) in the round loop of a batched
Get, on the version of scripts/bench_version_probe.py: db_bench's final state at
config 5 (5 + 40 + 377 level files + 4 flush files of 153,846 keys = 426 files),
one index block per file with one entry of a 28-byte internal key per key.

The index blocks are written on the GPU with torch (no Python loop over
entries; ``index_block_torch`` is dlsm_amd/index_block.py's fixed-length writer
restated in torch, compared here with it on one small table) and sealed with
the library's device crc32c.  Timed with device events on one stream:
  open         dlsm_tableindex_create_blocks of the 426 device-resident blocks
               (wall clock; it synchronises once), beside the copy ceiling
  loop         probe, then plan(FIRST) -> seek -> advance until a plan is empty,
               per call and per round; the only host read is file_begin's last
               entry (8 bytes) per round
  seek         the first round's seek alone, interleaved with
  searchsorted torch.searchsorted of the same tasks over pre-decoded u64 keys
               (file << 40 | value, handed to it for free), and
  d2h          what the host round trip the seek replaces would move per round:
               file_begin and gets to page-locked memory, a hit byte per Get back
The seek's byte floor is its byte model (index_seek.hip) over the copy rate
dlsm_stream_kernel kind 1 reaches in the same process.  Every Get's final state
is compared with arithmetic on the files' value ranges.  Prints one JSON line;
--out writes it.

    python scripts/bench_index_seek.py [--lookups 100000000] [--rounds 5] [--out profiles/index_seek.json]
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

KV_BYTES = 132  # a pair's bytes in the data region: the handles' offsets are multiples of it


def index_contents_torch(values, seq, dev):
    """The index block's contents for a table holding db_bench keys of `values`
    (ascending int64 on `dev`), every pair KV_BYTES long at i * KV_BYTES, in a
    buffer with room for the 5-byte trailer; returns (buffer, content bytes)."""
    import torch

    import dlsm_amd
    from dlsm_amd import workload as W

    n = int(values.numel())
    keys = torch.empty((n, 28), dtype=torch.uint8, device=dev)
    keys[:, :20] = W.dbbench_keys_torch(values).reshape(n, 20)
    tr = (seq << 8) | 1
    keys[:, 20:] = torch.tensor(list(tr.to_bytes(8, "little")), dtype=torch.uint8, device=dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * KV_BYTES
    lo = torch.ones(n, dtype=torch.int64, device=dev)
    for j in range(1, 6):
        lo += (off >= (1 << (7 * j))).to(torch.int64)
    size = dlsm_amd.index_block.varint(KV_BYTES)
    elen = 3 + 28 + lo + len(size)
    end = torch.cumsum(elen, 0)
    at = end - elen
    total = int(end[-1].item()) if n else 0
    out = torch.zeros(total + 4 * (n + 1) + 5, dtype=torch.uint8, device=dev)
    out[at + 1] = 28
    out[at + 2] = (lo + len(size)).to(torch.uint8)
    out[(at + 3)[:, None] + torch.arange(28, device=dev)[None, :]] = keys
    for j in range(6):
        m = lo > j
        b = ((off[m] >> (7 * j)) & 127) | torch.where(lo[m] > j + 1, 128, 0)
        out[at[m] + 31 + j] = b.to(torch.uint8)
    for j, b in enumerate(size):
        out[at + 31 + lo + j] = b
    tail = torch.cat([at.to(torch.int32), torch.tensor([n], dtype=torch.int32, device=dev)])
    out[total:total + 4 * (n + 1)] = tail.view(torch.uint8)
    return out, total + 4 * (n + 1)


def index_block_torch(ctx, values, seq, dev):
    """index_contents_torch sealed: type byte 0 and the masked crc32c (computed on the device)."""
    import torch

    import dlsm_amd

    out, n = index_contents_torch(values, seq, dev)
    torch.cuda.synchronize(dev)
    crc = ctx.crc32c_dev([out[:n + 1]])[0]
    out[-4:] = torch.tensor(list(dlsm_amd.crc32c_mask(crc).to_bytes(4, "little")), dtype=torch.uint8, device=dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lookups", type=int, default=100_000_000)
    ap.add_argument("--space", type=int, default=100_000_000, help="key space V")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--check", type=int, default=1_000_000, help="Gets whose outcome is compared with the ranges")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import dlsm_amd
    from dlsm_amd import index_block as ib
    from dlsm_amd import workload as W

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from bench_read_plan import copy_rate

    dev = torch.device("cuda", 0)
    ctx = dlsm_amd.Context(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream)
    V, Q = args.space, args.lookups
    files = W.dbbench_version(ctx, dev, V)
    ranges = W.dbbench_version_ranges(V)
    n_files = len(files)
    assert len(ranges) == n_files
    ver = ctx.version(files, on_device=True)
    res = {"what": "index seek of a planned Get batch in the round loop (probe, plan FIRST, seek, advance), device-resident",
           "files": n_files, "lookups": Q, "fence_interval": dlsm_amd.index_fence_interval(),
           "lib_variant": os.environ.get("DLSM_LIB_VARIANT", ""), "rounds": args.rounds, "reps": args.reps}

    # the writer restated in torch against the package's numpy writer, on a small table
    small = torch.arange(7, 7 + 3 * 40_000, 3, dtype=torch.int64, device=dev)
    kb = np.concatenate([W.dbbench_keys_np(small.cpu().numpy().astype(np.uint64)).reshape(-1, 20),
                         np.tile(np.frombuffer(((9 << 8) | 1).to_bytes(8, "little"), dtype=np.uint8), (40_000, 1))], axis=1)
    want = ib.build_index_block_fixed(kb, np.arange(40_000, dtype=np.uint64) * KV_BYTES, np.full(40_000, KV_BYTES, np.uint64))
    res["writer_matches_numpy"] = index_block_torch(ctx, small, 9, dev).cpu().numpy().tobytes() == want
    assert res["writer_matches_numpy"]

    blocks, comp = [], []
    for f, (lo, step, cnt) in enumerate(ranges):
        vals = torch.arange(lo, lo + step * cnt, step, dtype=torch.int64, device=dev)[:cnt]
        assert W.dbbench_keys_np(np.array([lo], dtype=np.uint64)).tobytes() == bytes(files[f].smallest)
        blocks.append(index_block_torch(ctx, vals, 100 + f, dev))
        comp.append((f << 40) | vals)
    comp = torch.cat(comp)  # ascending: files in order, values ascending inside a file
    entries = int(comp.numel())
    block_bytes = sum(int(b.numel()) for b in blocks)
    res.update({"entries": entries, "block_bytes": block_bytes})
    res["copy_gb_s"] = copy_rate(dev, stream, 2_000_000_000)

    opens = []
    ti = None
    for _ in range(3):
        if ti is not None:
            ti.close()
        ctx.sync()
        t0 = time.perf_counter()
        ti = ctx.tableindex(blocks, on_device=True)
        opens.append((time.perf_counter() - t0) * 1e3)
    assert ti.n_entries == entries
    # copy_ceiling_ms: one copy of the blocks at the streaming rate (the open also reads them once more to validate)
    res["open"] = {"wall_ms": [round(x, 2) for x in opens], "device_bytes": ti.device_bytes,
                   "copy_ceiling_ms": round(2 * block_bytes / (res["copy_gb_s"] * 1e9) * 1e3, 3),
                   "ingest_kernels_ms": round(ctx.block_open_stats()[2], 3)}
    del blocks

    rng = np.random.default_rng(12)
    qv = torch.from_numpy(rng.integers(0, 2 * V, Q, dtype=np.int64)).to(dev)
    qk = dlsm_amd.Keys(W.dbbench_keys_torch(qv), Q, 20)
    mask = torch.zeros(Q, dtype=torch.int64, device=dev)
    lf = torch.zeros((Q, 5), dtype=torch.int32, device=dev)
    snap = (1 << 56) - 1
    begin = torch.zeros(n_files + 1, dtype=torch.int64, device=dev)
    gets = torch.zeros(Q, dtype=torch.int32, device=dev)
    gs = torch.zeros(Q, dtype=torch.uint8, device=dev)
    gh = torch.zeros((Q, 16), dtype=torch.uint8, device=dev)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def loop():
        """One whole batch; returns per-call times per round and the task counts."""
        gs.zero_()
        gh.zero_()
        marks = [ev()]
        marks[0].record(stream)
        ctx.version_probe_dev(ver, qk, snap, mask, lf)
        marks.append(ev())
        marks[-1].record(stream)
        tasks = []
        while True:
            ctx.version_read_plan_dev(ver, mask, lf, dlsm_amd.PLAN_FIRST, begin, gets)
            marks.append(ev())
            marks[-1].record(stream)
            ctx.index_seek_dev(ti, qk, snap, begin, gets, get_state=gs, get_handle=gh)
            marks.append(ev())
            marks[-1].record(stream)
            ctx.version_masks_advance_dev(mask, gs)
            marks.append(ev())
            marks[-1].record(stream)
            t = int(begin[n_files].item())  # the 8-byte "is anything left" read
            if t == 0:
                break
            tasks.append(t)
        ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(len(marks) - 1)]
        per_round = [dict(plan=ms[1 + 3 * r], seek=ms[2 + 3 * r], advance=ms[3 + 3 * r]) for r in range(len(tasks) + 1)]
        return ms[0], per_round, tasks, marks[0].elapsed_time(marks[-1])

    loop()  # warm-up
    # every Get's outcome, from the ranges: the newest file holding the value wins, flush files (newest last) first
    nc = min(args.check, Q)
    st = gs[:nc].cpu().numpy()
    h = gh[:nc].cpu().numpy().reshape(-1).view(dlsm_amd.KV_HANDLE)
    v = qv[:nc].cpu().numpy()
    want_f = np.full(nc, -1, dtype=np.int64)
    want_i = np.zeros(nc, dtype=np.int64)
    order = sorted(range(n_files), key=lambda f: (files[f].level != 0, -files[f].number if files[f].level == 0 else files[f].level))
    for f in order:
        lo, step, cnt = ranges[f]
        d = v - lo
        inside = (want_f < 0) & (d >= 0) & (d % step == 0) & (d // step < cnt)
        want_f[inside] = f
        want_i[inside] = d[inside] // step
    found = want_f >= 0
    ok = (np.array_equal(st, found.astype(np.uint8)) and np.array_equal(h["file"][found], want_f[found].astype(np.uint32)) and
          np.array_equal(h["offset"][found], (want_i[found] * KV_BYTES).astype(np.uint64)) and
          bool((h["size"][found] == KV_BYTES).all()) and not h["offset"][~found].any())
    res["outcomes_match_ranges"] = bool(ok)
    res["outcomes_checked"] = nc
    res["found"] = int((gs != 0).sum().item())

    loops = [loop() for _ in range(args.rounds)]
    res["tasks_per_round"] = loops[0][2]

    def stat(xs):
        return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}

    res["loop"] = {"probe": stat([l[0] for l in loops]), "whole": stat([l[3] for l in loops]),
                   "rounds": [{k: stat([l[1][r][k] for l in loops]) for k in ("plan", "seek", "advance")}
                              for r in range(len(loops[0][1]))]}
    for k in ("plan", "seek", "advance"):
        res["loop"][k + "_all_rounds"] = stat([sum(r[k] for r in l[1]) for l in loops])

    # the first round's seek alone, torch.searchsorted on free u64 keys, and the host round trip's copies
    ctx.version_probe_dev(ver, qk, snap, mask, lf)
    ctx.version_read_plan_dev(ver, mask, lf, dlsm_amd.PLAN_FIRST, begin, gets)
    ctx.sync()
    T = int(begin[n_files].item())
    cnt = (begin[1:] - begin[:-1])
    tfile = torch.repeat_interleave(torch.arange(n_files, device=dev), cnt)
    tcomp = (tfile << 40) | qv[gets[:T].long()]
    del tfile

    def timed(fn):
        e0, e1 = ev(), ev()
        e0.record(stream)
        for _ in range(args.reps):
            fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / args.reps

    ts = torch.zeros(T, dtype=torch.uint8, device=dev)
    th = torch.zeros((T, 16), dtype=torch.uint8, device=dev)
    hb = torch.empty(n_files + 1, dtype=torch.int64, pin_memory=True)
    hg = torch.empty(Q, dtype=torch.int32, pin_memory=True)
    hh = torch.zeros(Q, dtype=torch.uint8, pin_memory=True)

    def d2h():
        hb.copy_(begin, non_blocking=True)
        hg[:T].copy_(gets[:T], non_blocking=True)
        gs.copy_(hh, non_blocking=True)

    legs = {"seek_get_arrays": [], "seek_task_arrays": [], "searchsorted": [], "d2h": []}
    pos = torch.searchsorted(comp, tcomp)
    hit = comp[pos.clamp(max=entries - 1)] == tcomp
    ctx.index_seek_dev(ti, qk, snap, begin, gets, cap=T, task_state=ts, task_handle=th)
    ctx.sync()
    res["task_states_match_searchsorted"] = bool(torch.equal(ts, hit.to(torch.uint8)))
    del pos, hit
    for _ in range(args.rounds):
        legs["seek_get_arrays"].append(timed(lambda: ctx.index_seek_dev(ti, qk, snap, begin, gets, get_state=gs, get_handle=gh)))
        legs["seek_task_arrays"].append(timed(lambda: ctx.index_seek_dev(ti, qk, snap, begin, gets, cap=T, task_state=ts,
                                                                         task_handle=th)))
        legs["searchsorted"].append(timed(lambda: torch.searchsorted(comp, tcomp)))
        legs["d2h"].append(timed(d2h))
    res["first_round"] = {"tasks": T, **{k: stat(x) for k, x in legs.items()}}
    # byte model per task (index_seek.hip): Get index 4, key 20, file record 40 (shared by a file's tasks:
    # not counted), log2(fences) x 16 fence bytes and log2(S) x (4 restart + 3 header + 28 key) window bytes
    # (upper levels shared through L2: the floor counts only the last fence and the last window step),
    # entry's handle ~4, outputs 1 + 16 where found (half the tasks here)
    floor_bytes = T * (4 + 20 + 16 + (4 + 31) + 4) + res["found"] * 17
    floor = floor_bytes / (res["copy_gb_s"] * 1e9) * 1e3
    sk = res["first_round"]["seek_get_arrays"]["median_ms"]
    res["first_round"].update({"floor_bytes": floor_bytes, "floor_ms": round(floor, 3), "seek_over_floor": round(sk / floor, 2),
                               "searchsorted_over_seek": round(res["first_round"]["searchsorted"]["median_ms"] / sk, 2),
                               "d2h_bytes": 8 * (n_files + 1) + 4 * T + Q})
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
