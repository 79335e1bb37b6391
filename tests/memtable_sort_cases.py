"""The batches the memtable sort's CPU and GPU tests are made of: (internal
key, value) pairs in arrival order.  What their sort must be is
dlsm_amd/compaction.py's merge_runs over the one batch (through
compaction_merge_cases.expected).  T is the implementation's records per sorted
tile, L the records a lane holds; the sizes are the smallest at which each
stage -- the register network, one tile, an unpaired segment in one pass and in
two, every pass full -- can go wrong."""
import numpy as np

import dlsm_amd
from dlsm_amd.compaction import MAX_SEQUENCE
from compaction_merge_cases import P16, ik

T, L = dlsm_amd.sort_tile(), 4
rng = np.random.default_rng(2611)
BLOB = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
# user keys of 0, 1, 15, 16, 17 and 40 bytes: proper prefixes of one another, embedded and trailing zero
# bytes, and groups longer than 16 bytes that share their first 16 (the comparator's byte path)
POOL = ([BLOB[:m] for m in (0, 1, 15, 16, 17, 40)] + [b"a", b"a\0", b"a\0\0", b"a\0b", P16, P16 + b"\0", P16[:15]] +
        [P16 + s for s in (b"x", b"xy", b"y", b"x\0", b"x" * 24)] + [BLOB[:16] + bytes([j]) * (j % 3 + 1) for j in range(9)])


def value(j):
    return bytes((j * 7 + b) & 255 for b in range(0 if j % 5 == 0 else j % 37))


def fixed(n, order="random", users=None):
    """28-byte internal keys: 20-byte user keys out of `users` (default 3n/4, so some repeat), sequence 100 + j."""
    u = rng.integers(0, users or max(3 * n // 4, 1), n)
    keys = [ik(b"%020d" % x, 100 + j, j % 4 != 0) for j, x in enumerate(u)]
    if order != "random":
        keys.sort(key=lambda k: (k[:-8], -int.from_bytes(k[-8:], "little")), reverse=order == "descending")
    return [(k, value(j)) for j, k in enumerate(keys)]


def variable(n, types=(0, 1)):
    """Keys out of POOL, sequences out of a narrow range (repeats of a whole key included), types out of `types`."""
    return [(ik(POOL[rng.integers(len(POOL))], int(rng.integers(90, 130)), int(rng.choice(types))), value(j)) for j in range(n)]


def duplicates(n):
    """Every key twice or more, its copies anywhere in the batch: only src tells them apart."""
    base = fixed(n // 3 + 1)
    return [(base[x][0], value(j)) for j, x in enumerate(rng.integers(0, len(base), n))]


CASES = {f"n{n}": dict(runs=[fixed(n)]) for n in (0, 1, L - 1, L, L + 1)}
CASES.update({
    "T-1-variable": dict(runs=[variable(T - 1)], policy=1, snapshot=110),
    "T-ascending": dict(runs=[fixed(T, "ascending")]),
    "T+1-descending": dict(runs=[fixed(T + 1, "descending")], policy=1, snapshot=0),
    "2T+5-one-user-key": dict(runs=[fixed(2 * T + 5, users=1)], policy=1, snapshot=100 + T),
    "2T+5-variable-keep": dict(runs=[variable(2 * T + 5)]),
    "3T+7-flush": dict(runs=[variable(3 * T + 7, types=(0, 1, 1, 2, 7))], policy=1, snapshot=MAX_SEQUENCE),
    "5T+1-duplicates": dict(runs=[duplicates(5 * T + 1)]),
    "8T-random": dict(runs=[fixed(8 * T)], policy=1, snapshot=100 + 4 * T),
    "cap-keys": dict(runs=[variable(T + 1)], keys_cap=9001),
    "cap-values": dict(runs=[variable(T + 1)], values_cap=7777),
    "cap-pairs": dict(runs=[variable(T + 1)], pair_cap=T - 3),
})
SHORT = fixed(2 * T + 5)  # a key shorter than 8 bytes in the last tile
SHORT[2 * T + 2] = (b"1234567", b"v")
