"""The table sets and scan batches the range scan's tests are made of, built
with the helpers of compaction_tables_cases.  What a scan must give comes from compaction.scan_runs over compaction.table_pairs: the reference's
sequential walk of every table, then an explicit DBIter loop."""
import numpy as np

from dlsm_amd import compaction as cp
from compaction_merge_cases import P16, ik, listed
from compaction_tables_cases import SHARED, case, host_args, level, two_files  # noqa: F401 (host_args, two_files: the tests')

U = lambda x: b"%08d" % x + b"k" * (x % 7)  # noqa: E731  (level's user keys: 8 to 14 bytes)
W = lambda x: b"%016d" % x                  # noqa: E731
one = lambda *runs: [[r] for r in listed(*runs)]  # noqa: E731  (a one-file run each)
A, B, Cc, D = b"apple", b"berry", b"cherry", b"damson"
SMALL = [level([150, 77], 100), level([60], 101, first=1), level([30], 102, first=0, step=4)]

CASES = {
    # starts: below every key, a stored key, between two keys, above every key
    "one-file": case([level([9], 100)], starts=[b"", U(4), b"00000005", b"9"], snapshot=100, limit=4),
    # a run without files, files without entries; a start between two files, a scan across a file boundary; Q = 1
    "empty-run-and-files": case([level([5, 0, 4], 100), [], level([0], 101)], starts=[b"00000009"], snapshot=200, limit=3),
    "across-files": case([level([5, 0, 4], 100), [], level([0], 101)], starts=[U(6), b"", U(16), b"0000001", U(8)],
                         snapshot=200, limit=4),
    # 40-byte pairs, two to a 96-byte chunk: the scans cross chunk and file boundaries; Q = 5
    "across-chunks": case([level([6, 6], 100, user=W, vlen=lambda j: 8)], order=[0, 1], chunk_bytes=96,
                          starts=[b"", W(3), W(10), W(11), W(22)], snapshot=100, limit=8),
    # apple: the newest entry above the snapshot; berry: a level-0 tombstone hides the values below; damson: a
    # tombstone is the very last entry
    "three-runs": case(one([(A, 120), (B, 104, 0), (D, 103, 0)], [(A, 104), (B, 103), (Cc, 102)], [(A, 101), (B, 100)]),
                       starts=[b"", A, B, Cc, D], snapshot=105, limit=5),
    # 70 versions of one key: 5 above the snapshot, one yielded, 64 hidden by the record carried over
    "seventy-versions": case(one([(A, 101 + j) for j in range(70)] + [(B, 7), (Cc, 8, 0), (D, 9)]), starts=[b"", A + b"\0"],
                             snapshot=165, limit=3),
    # the most runs a call takes; `zz` lies in every run
    "sixty-four-runs": case(one(*[[(b"%04d" % (64 * j + r), 100 + r, (j + r) % 3 != 0) for j in range(3)] + [(b"zz", 100 + r)]
                                  for r in range(64)]), starts=[b"", b"0100", b"zz"], snapshot=140, limit=200),
    "limit-1": case(SMALL, starts=[b"", U(100), U(453)], snapshot=101, limit=1),
    "limit-cap": case(SMALL, starts=[U(400), b""], snapshot=101, limit=1024),  # both scans end by exhaustion
    # the same internal key in two runs: the lower run's pair is the one yielded
    "same-internal-key": case(one([(A, 100), (B, 100)], [(A, 100), (Cc, 100)]), starts=[b""], snapshot=100, limit=4),
    # keys that share their first 16 bytes and differ later, or end there
    "shared-prefixes": case([[SHARED[0]], [SHARED[1]], [SHARED[2]]], chunk_bytes=200,
                            starts=[b"", P16, P16 + b"aa", P16 + b"b" * 20, P16 + b"b" * 20 + b"!"], snapshot=8, limit=6),
    "bad-type": case(one([(A, 5), (B, 6, 2), (Cc, 7)], [(B, 4)]), starts=[b"", Cc], snapshot=9, limit=3),
    "bad-type-behind-the-limit": case(one([(A, 5), (B, 6, 2), (Cc, 7)], [(B, 4)]), starts=[b"", Cc], snapshot=9, limit=1),
    "cap-keys": case(SMALL, starts=[U(10), U(200)], snapshot=101, limit=40, keys_cap=1001),
    "cap-values": case(SMALL, starts=[U(10), U(200)], snapshot=101, limit=40, values_cap=901),
    "cap-pairs": case(SMALL, starts=[U(10), U(200)], snapshot=101, limit=40, pair_cap=33),
}


def mismatch():
    """A handle that straddles a chunk, yielded by the scan from the smallest key."""
    return dict(two_files(handles=lambda h: h.__setitem__(1, (40, 48))), starts=[b""], snapshot=100, limit=12)


def keys_of(items):
    """(bytes, offsets): the start keys packed with offsets."""
    return (np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8).copy(),
            np.concatenate([[0], np.cumsum([len(x) for x in items])]).astype(np.uint64))


def want(c):
    """The scans of a case: the walk of every listed table, then scan_runs."""
    runs, where = [], []
    for run in c["runs"]:
        runs.append([])
        where.append([])
        for f in run:
            at = 0
            for k, v in cp.table_pairs(c["tables"][f][0][:-5], c["tables"][f][1]):
                runs[-1].append((k, v))
                where[-1].append((at, 8 + len(k) + len(v) | f << 32))
                at += 8 + len(k) + len(v)
    q, limit = len(c["starts"]), c["limit"]
    count, handle, pairs, flags = [], np.zeros((q * limit, 2), dtype=np.uint64), [], 0
    for s, start in enumerate(c["starts"]):
        got, src, bad = cp.scan_runs(runs, start, c["snapshot"], limit)
        flags |= 8 if bad else 0
        count.append(len(got))
        pairs += got
        for j, x in enumerate(src):
            handle[s * limit + j] = where[x >> 32][x & 0xffffffff]
    keys, values = b"".join(p[0] for p in pairs), b"".join(p[1] for p in pairs)
    ko = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])]).astype(np.uint64)
    vo = np.concatenate([[0], np.cumsum([len(p[1]) for p in pairs])]).astype(np.uint64)
    caps = [c.get("keys_cap", len(keys)), c.get("values_cap", len(values)), c.get("pair_cap", len(pairs))]
    flags |= (len(keys) > caps[0]) | (len(values) > caps[1]) << 1 | (len(pairs) > caps[2]) << 2
    return dict(count=np.array(count, dtype=np.uint32), pair_begin=np.concatenate([[0], np.cumsum(count)]).astype(np.uint64),
                handle=handle, keys=np.frombuffer(keys[:caps[0]], dtype=np.uint8), key_off=ko[:caps[2] + 1],
                values=np.frombuffer(values[:caps[1]], dtype=np.uint8), value_off=vo[:caps[2] + 1],
                scanned=(q, len(pairs), len(keys), len(values), flags), caps=caps, pairs=pairs)


OUTPUTS = ("count", "pair_begin", "handle", "keys", "key_off", "values", "value_off")
