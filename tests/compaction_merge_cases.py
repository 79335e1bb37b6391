"""The runs the compaction merge's CPU and GPU tests are made of, and what
dlsm_amd/compaction.py (pure Python) says their merge is.  T is the
implementation's records per merge tile, C its pairs per chunk of the record,
decide and offset passes, Sp its output bytes per gather step."""
import struct

import numpy as np

import dlsm_amd
from dlsm_amd import compaction as cp
from table_build_cases import VALUES

T, Sp, C = dlsm_amd.merge_tile(), dlsm_amd.merge_span(), dlsm_amd.merge_chunk()
P16 = b"sixteen-byte-pfx"


def ik(user, seq, t=1):
    return user + struct.pack("<Q", seq << 8 | t)


def val(r, j, vlen):
    return bytes((r * 31 + j * 7 + b) & 255 for b in range(vlen(j)))


def numbered(lengths, user=lambda x: b"%08d" % x, vlen=VALUES["mix"], stride=3):
    """Run r holds user keys r % stride, r % stride + stride, ...: runs r and
    r + stride share their user keys, at sequence 100 + r."""
    runs = [[(ik(user(j * stride + r % stride), 100 + r, (j + r) % 4 != 0), val(r, j, vlen)) for j in range(n)]
            for r, n in enumerate(lengths)]
    return [sorted(run, key=lambda p: (p[0][:-8], -cp.trailer(p[0]))) for run in runs]


def listed(*runs, vlen=VALUES["v17"]):
    """Runs from (user key, sequence[, type]) lists, sorted here."""
    out = []
    for r, keys in enumerate(runs):
        iks = sorted((ik(*k) for k in keys), key=lambda k: (k[:-8], -cp.trailer(k)))
        out.append([(k, val(r, j, vlen)) for j, k in enumerate(iks)])
    return out


def filler(n, seq=50):
    return [(b"%08d" % j, seq) for j in range(n)]


def total_edge(what, delta):
    """Two runs whose key (or value) total ends delta bytes from Sp."""
    n = Sp // 64  # 32-byte keys and values: both totals are Sp - 32 before the last pair grows
    runs = numbered([n, n - 1], user=lambda x: b"%024d" % x, vlen=lambda j: 32, stride=2)
    k, v = runs[1][-1]
    runs[1][-1] = (k[:-8] + b"p" * (32 + delta) + k[-8:], v) if what == "keys" else (k, v + b"q" * (32 + delta))
    return runs


LEN = [0, 1, T - 1, T, T + 1, 2 * T + 3]
CASES = {f"R{R}-{p}": dict(runs=numbered([LEN[(r + R) % 6] for r in range(R)]), policy=p, snapshot=s)
         for R in (1, 2, 3, 5, 8) for p, s in ((0, 0), (1, 103))}
CASES.update({
    "all-empty": dict(runs=[[], [], []]),
    "disjoint": dict(runs=listed(filler(T + 5), [(b"z%07d" % j, 9) for j in range(T + 9)])),
    "disjoint-reversed": dict(runs=listed([(b"z%07d" % j, 9) for j in range(T + 9)], filler(T + 5))),
    "run-inside-a-gap": dict(runs=listed(filler(2 * T + 7), [(b"00000003x%05d" % j, 9) for j in range(2 * T + 1)])),
    "interleave": dict(runs=numbered([T + 3, T + 3], stride=2), policy=1, snapshot=10 ** 6),
    "compare-paths": dict(runs=listed(
        [(b"", 5), (b"a", 5), (b"a\0\0", 5), (P16, 7), (P16 + b"x", 7), (P16 + b"xy", 3), (b"short", 4), (P16 + b"\0", 1)],
        [(b"", 9), (b"a\0", 5), (b"a", 5), (P16 + b"x", 9), (P16 + b"y", 2), (P16[:15], 4), (P16 + b"xy", 3, 0)],
        [(b"a\0", 7), (P16 + b"\0", 1), (P16 + b"x", 8), (b"short", 4), (b"shor", 4)]), policy=1, snapshot=7),
    "group-over-a-tile-edge": dict(runs=listed(filler(T - 2) + [(b"zz", 40)], [(b"zz", 30), (b"zz", 20)], [(b"zz", 35)],
                                               [(b"zz", 10), (b"zzz", 1)]), policy=1, snapshot=25),
    "hidden-at-a-chunk-start": dict(runs=listed(filler(C - 1) + [(b"zz", 9)], [(b"zz", 5), (b"zzz", 5)]), policy=1,
                                    snapshot=9),
    "type-2-restarts": dict(runs=listed([(b"m", 9), (b"m", 7), (b"n", 3)], [(b"m", 8, 2), (b"m", 6), (b"n", 2, 2)]),
                            policy=1, snapshot=100),
})
CASES.update({f"snapshot-{w}": dict(runs=numbered([40] * 6), policy=1, snapshot=s)
              for w, s in (("below", 99), ("inside", 103), ("above", 10 ** 6))})
CASES.update({f"values-{v}-{k}": dict(runs=numbered([T + 1, 300], user=u, vlen=VALUES[v]), policy=1, snapshot=103)
              for v in VALUES for k, u in (("fixed", lambda x: b"%020d" % x), ("var", lambda x: b"%d" % 7 ** (x % 40) + b"%05d" % x))})
CASES.update({f"{w}-total{d:+d}": dict(runs=total_edge(w, d)) for w in ("keys", "values") for d in (-1, 0, 1)})
CASES.update({f"cap-{n}": dict(runs=numbered([T + 1, 300, 77]), policy=1, snapshot=101, **kw)
              for n, kw in (("keys-mid", {"keys_cap": 9001}), ("keys-0", {"keys_cap": 0}), ("values-mid", {"values_cap": Sp + 5}),
                            ("values-0", {"values_cap": 0}), ("pairs-mid", {"pair_cap": T - 3}), ("pairs-0", {"pair_cap": 0}))})
# malformed input: only merged.n_in and merged.flags are specified
BAD = {
    "short-key": (numbered([5, 300]), lambda runs: runs[1].__setitem__(7, (b"1234567", b"v")), 8),
    "equal-neighbours": (numbered([T + 1, 9]), lambda runs: runs[0].__setitem__(4, runs[0][3]), 16),
    "descent-at-a-chunk-start": (numbered([5, 2 * C]), lambda runs: runs[1].__setitem__(C - 5, runs[1][C - 7]), 16),
}


def expected(case):
    """What the merge of a case must give under its caps."""
    pairs, src = cp.merge_runs(case["runs"], case.get("policy", 0), case.get("snapshot", 0))
    keys, values = b"".join(p[0] for p in pairs), b"".join(p[1] for p in pairs)
    ko = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])]).astype(np.uint64)
    vo = np.concatenate([[0], np.cumsum([len(p[1]) for p in pairs])]).astype(np.uint64)
    caps = [case.get("keys_cap", len(keys)), case.get("values_cap", len(values)), case.get("pair_cap", len(pairs))]
    flags = (len(keys) > caps[0]) + 2 * (len(values) > caps[1]) + 4 * (len(pairs) > caps[2])
    p = min(len(pairs), caps[2])
    return dict(keys=np.frombuffer(keys, dtype=np.uint8)[:caps[0]], values=np.frombuffer(values, dtype=np.uint8)[:caps[1]],
                key_off=ko[:p + 1], value_off=vo[:p + 1], src=np.array(src[:p], dtype=np.uint64), caps=caps,
                merged=[sum(map(len, case["runs"])), len(pairs), len(keys), len(values), flags])


def packed(items):
    """(bytes, offsets or None, length): one length where the lengths are uniform."""
    data = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8).copy()
    if len(set(map(len, items))) == 1:
        return data, None, len(items[0])
    return data, np.concatenate([[0], np.cumsum([len(x) for x in items])]).astype(np.uint64), 0
