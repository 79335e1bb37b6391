"""The runs the compaction output's CPU and GPU tests are made of, a plain walk
of the cut rule, and the expected bytes: dlsm_amd.table_build (the host table
build, which the code under test's kernels do not run) on every file's slice."""
import functools

import numpy as np

import dlsm_amd
from dlsm_amd import Keys
from table_build_cases import KEYS, VALUES, make

C, S = dlsm_amd.table_build_chunk(), dlsm_amd.table_build_span()
K28, VAR, MIX = KEYS["k28"], KEYS["var"], VALUES["mix"]


def sizes(iks, vals):
    return [8 + len(k) + len(v) for k, v in zip(iks, vals)]


def _at(n, k):
    """max_file_bytes that puts the first cut in front of pair k of n var/mix pairs."""
    return sum(sizes(*make(n, VAR, MIX))[:k])


# name: (n, key length, value length, max_file_bytes, chunk_bytes)
CASES = {
    "n0": (0, VAR, MIX, 100, 0),
    "n1": (1, VAR, MIX, 100, 50),
    "one-file": (300, VAR, MIX, 0, 1000),
    "exact": (25, K28, lambda j: 28, 640, 0),          # 64-byte pairs: the tenth lands on the threshold
    "short-by-1": (25, K28, lambda j: 28, 641, 0),     # ... one byte short: the eleventh joins
    "big-pair": (30, K28, lambda j: 1000 if j == 12 else 28, 300, 128),
    "every-pair": (2 * C + 3, KEYS["k8"], VALUES["v1"], 1, 0),
    "every-pair-var": (300, VAR, MIX, 1, 100),
    "cut-C-1": (C + 40, VAR, MIX, _at(C + 40, C - 1), 4096),
    "cut-C": (C + 40, VAR, MIX, _at(C + 40, C), 4096),
    "cut-C+1": (C + 40, VAR, MIX, _at(C + 40, C + 1), 4096),
    # file 0 is ten 64-byte pairs, file 1 one pair that ends at S + d of the padded space, file 2 the rest
    **{f"span{d:+d}": (14, K28, lambda j, d=d: S - 640 + d - 36 if j == 10 else 28, 640, 0) for d in (-1, 0, 1)},
    # files of 20 KB: every file's relative offsets cross 128 and 16,384 where the run's do not, and the run's
    # chunk boundaries (multiples of about 3,000) lie inside the files' first chunks
    "varint-chunks": (300, VAR, MIX, 20000, 3000),
    "oversize-chunk": (20, K28, lambda j: 28, 200, 15),
    "fixed": (C + 1, K28, VALUES["v400"], 436 * 600, 65536),
}


def cut_walk(pair_sizes, max_file_bytes):
    """first[]: the reference's loop, pair by pair."""
    first, size = [], 0
    for i, p in enumerate(pair_sizes):
        if size == 0:
            first.append(i)
        size += p
        if max_file_bytes and size >= max_file_bytes:
            size = 0
    return first


def pack(items):
    """(bytes, offsets or None, one length): one length wherever the lengths are uniform."""
    data = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8)
    if len(set(map(len, items))) == 1:
        return data, None, len(items[0])
    return data, np.concatenate([[0], np.cumsum([len(x) for x in items])]).astype(np.uint64), 0


def pad16(x):
    return (x + 15) & ~15


@functools.lru_cache(maxsize=None)
def expected(name):
    """(iks, vals, tables, records, built): per file (data, chunk_end, index block)
    as bytes / lists, the nine-number records and the totals with flags 0 or
    TABLE_OVERSIZE_PAIR."""
    n, kl, vl, mfb, cb = CASES[name]
    iks, vals = make(n, kl, vl)
    first = cut_walk(sizes(iks, vals), mfb) + [n]
    tables, recs, tot = [], [], [0, 0, 0, 0]
    for a, b in zip(first, first[1:]):
        kb, ko, klen = pack(iks[a:b])
        vb, vo, vlen = pack(vals[a:b])
        data, index, ends, built = dlsm_amd.table_build(Keys(kb, b - a, klen, ko), vb, value_off=vo, value_len=vlen,
                                                        chunk_bytes=cb)
        tables.append((data.tobytes(), ends.tolist(), index.tobytes()))
        recs.append([a, b - a, tot[0], built[0], tot[1], built[1], tot[2], built[2], built[3]])
        tot = [tot[0] + pad16(built[0]), tot[1] + pad16(built[1]), tot[2] + built[2], tot[3] | built[3]]
    return iks, vals, tables, recs, (len(tables), tot[0], tot[1], tot[2], tot[3])
