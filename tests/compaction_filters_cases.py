"""The cut runs the compaction filters' CPU and GPU tests are made of, and the
expected blocks: the oracle's full filter over every file's user keys (the
8-byte trailers stripped here), sealed by the oracle."""
import functools

import numpy as np

import oracle
from compaction_merge_cases import ik

CHUNK = 4096  # pairs per hash / partition workgroup


def k28(j, seq=5):
    return ik(b"%020d" % j, seq)


def var(j, seq=5):
    """Internal keys of 9..40 bytes."""
    return ik((b"%08d" % j + b"k" * 24)[:1 + (j * 7) % 32], seq)


def versions(key, users, per):
    return [key(u, 9 - v) for u in range(users) for v in range(per)]


# name: (internal keys, pairs per file, bits per key)
CASES = {
    # hundreds of files of L = 1 inside one chunk
    "tiny-k28": ([k28(j) for j in range(3400)], [1, 2, 31] * 100, 10),
    "tiny-var": ([ik(b"", 7)] + [var(j) for j in range(1, 3400)], [1, 2, 31] * 100, 10),  # key 0: 8 bytes, no user key
    # a cut on a multiple of the chunk, at one less and one more, then a file over three chunks
    "chunk-edges": ([var(j) for j in range(17000)], [CHUNK, CHUNK - 1, 2, 17000 - 2 * CHUNK - 1], 10),
    # three versions per user key, cut between the versions: the same hash on both sides, the dedup restarts
    "straddle": (versions(var, 50, 3), [4] * 37 + [2], 10),
    "straddle-chunk": (versions(k28, 1400, 3), [CHUNK + 1, 104 - 1], 10),  # ... and across a chunk edge
    # 160 user keys twice: ceil(3200 / 512) = 7 lines by n, ceil(1600 / 512) = 4, made odd: 5, by the distinct count
    "dups-lower-L": (versions(k28, 160, 2) + [k28(1000 + j) for j in range(30)], [320, 30], 10),
    # 391 lines: three slices of 128 lines and a short one at the smallest slice the planner chooses
    "slices-var": ([var(j) for j in range(20100)], [20000, 100], 10),
    "slices-k28-k8": ([k28(j) for j in range(9000)], [40, 8960], 12),  # k = 8: the general probe loop
    "k8-var": (versions(var, 700, 2), [700, 700], 12),
}


def pack(iks):
    """(bytes, offsets or None, one length): one length wherever the lengths are uniform."""
    data = np.frombuffer(b"".join(iks) or b"\0", dtype=np.uint8)
    if len(set(map(len, iks))) == 1:
        return data, None, len(iks[0])
    return data, np.concatenate([[0], np.cumsum([len(x) for x in iks])]).astype(np.uint64), 0


def file_records(sizes):
    """The dlsm_output_file records of a cut (first and n; the rest is not read) and its totals."""
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    recs = np.zeros((len(sizes), 9), dtype=np.uint64)
    recs[:, 0], recs[:, 1] = first[:-1], sizes
    return recs, np.array([len(sizes), 0, 0, 0, 0], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(blocks, records, built): per file the sealed block (bytes), base /
    bytes / n_distinct / num_lines, and (n_files, filter_bytes, 0)."""
    iks, sizes, bpk = CASES[name]
    assert sum(sizes) == len(iks)
    blocks, recs, at, base = [], [], 0, 0
    for n in sizes:
        data, offs = oracle.pack_var([k[:-8] for k in iks[at:at + n]])
        filt = oracle.full_build(data, n, offsets=offs, bpk=bpk)
        blocks.append(oracle.filter_block(filt))
        recs.append([base, len(blocks[-1]), oracle.full_dedup_count(data, n, offsets=offs), (len(filt) - 5) // 64])
        at, base = at + n, base + (len(blocks[-1]) + 15 & ~15)
    return blocks, recs, (len(sizes), base, 0)
