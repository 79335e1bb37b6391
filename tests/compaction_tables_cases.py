"""The table sets the tables merge's CPU and GPU tests are made of.  Tables come
from data_region.build_region and index_block.build_index_block; what a merge
must give comes from compaction.merge_runs over compaction.table_pairs -- the
reference's sequential walk, which looks at the first handle only.  C is the
implementation's entries per chunk of the record pass, T its records per tile."""
from dlsm_amd import compaction as cp
from dlsm_amd.data_region import build_region
from dlsm_amd.index_block import build_index_block
from compaction_merge_cases import C, P16, T, expected, ik, val
from table_build_cases import VALUES


def level(sizes, seq, first=0, step=2, user=lambda x: b"%08d" % x + b"k" * (x % 7), vlen=VALUES["mix"]):
    """The files of one level in key order: file j holds sizes[j] pairs, user
    keys numbered first, first + step, ... through the files."""
    files, x = [], first
    for n in sizes:
        files.append([(ik(user(x + step * j), seq, (x + j) % 5 != 0), val(seq, x + j, vlen)) for j in range(n)])
        x += step * n
    return files


def tables(files, chunk_bytes=None):
    """(sealed index block, chunks) per file."""
    out = []
    for pairs in files:
        chunks, handles = build_region(pairs, chunk_bytes)
        out.append((build_index_block([k for k, _ in pairs], handles), chunks))
    return out


def case(levels, order=None, unused=(), chunk_bytes=None, **kw):
    """levels: one file list per run.  The files are numbered by `order` (a
    permutation of their listing order; default reversed, so runs list their
    files out of numeric order) behind the `unused` files, which no run lists."""
    flat = [f for lv in levels for f in lv]
    order = list(order or reversed(range(len(flat))))
    number = {k: len(unused) + order.index(k) for k in range(len(flat))}
    files = list(unused) + [flat[k] for k in order]
    runs, k = [], 0
    for lv in levels:
        runs.append([number[k + j] for j in range(len(lv))])
        k += len(lv)
    return dict(tables=tables(files, chunk_bytes), runs=runs, **kw)


def want(c):
    """The merge of a case: the walk of every listed table, then merge_runs."""
    runs = [[p for f in run for p in cp.table_pairs(c["tables"][f][0][:-5], c["tables"][f][1])] for run in c["runs"]]
    return expected(dict(c, runs=runs))


LONG = P16 * 8 + b"tail"  # 132 bytes: the entry's non_shared takes two varint bytes
SHARED = [[(ik(P16 + s, 9 - r), val(r, j, lambda j: 7 * j)) for j, s in enumerate(names)]
          for r, names in enumerate(((b"", b"a", b"ab", b"b" * 20), (b"a", b"aa", b"b" * 20, b"c"), (b"b" * 20 + b"!",)))]
SMALL = [level([300, 77], 100), level([150], 101, first=1), level([60], 102, first=0, step=4)]
CASES = {
    # file and run boundaries on chunk starts, a predecessor in the chunk and the file before, empty files and runs;
    # sequences 100, 102, 105 of one user key lie in files of three runs: under snapshot 103 the oldest is hidden
    "file-sizes": case([level([C - 1, 1, 0, C], 100), level([C + 1, T + 1], 101, first=1), level([1], 102, first=8), [],
                        level([0], 104), level([40], 105, step=4)], unused=level([5], 99), chunk_bytes=4096, policy=1,
                       snapshot=103),
    "keep-all": case([level([C + 1, 3], 100), level([7], 101)], chunk_bytes=1 << 16),
    # 40-byte pairs in 80-byte chunks: every second pair ends a chunk exactly, its neighbour lies in the next
    "chunked": case([level([9, 4], 100, user=lambda x: b"%016d" % x, vlen=lambda j: 8),
                     level([5], 101, user=lambda x: b"%016d" % x, vlen=lambda j: 3 * j)], chunk_bytes=80, policy=1,
                    snapshot=101),
    "long-keys": case([[SHARED[0], [(ik(LONG, 4), b"v"), (ik(LONG + b"x", 4), b""), (ik(P16 + b"zz", 5), b"")]],
                       [SHARED[1]], [SHARED[2]]], chunk_bytes=200, policy=1, snapshot=9),
    "cap-keys": case(SMALL, policy=1, snapshot=101, keys_cap=4001),
    "cap-values": case(SMALL, policy=1, snapshot=101, values_cap=9001),
    "cap-pairs": case(SMALL, policy=1, snapshot=101, pair_cap=333),
}


def two_files(chunk_bytes=96, handles=None, region=None):
    """One run of two files (numbers 0, 1) of six 40-byte pairs each (24-byte
    keys, 8-byte values), two pairs to a 96-byte chunk; file 1 rebuilt over
    handles changed by handles(h) and chunks changed by region(chunks)."""
    lv = level([6, 6], 100, user=lambda x: b"%016d" % x, vlen=lambda j: 8)
    c = case([lv], order=[0, 1], chunk_bytes=chunk_bytes)
    chunks, h = build_region(lv[1], chunk_bytes)
    if handles:
        handles(h)
    c["tables"][1] = (build_index_block([k for k, _ in lv[1]], h), region(chunks) if region else chunks)
    return c


# malformed input and its flag: only merged.n_in and merged.flags are specified
BAD = {
    "overlapping-files": (lambda: case([level([5], 100) + level([5], 100, first=8)], order=[0, 1]), 16),
    "handle-straddles-a-chunk": (lambda: two_files(handles=lambda h: h.__setitem__(1, (40, 48))), 32),
    "header-key-size": (lambda: two_files(region=lambda ch: [ch[0], b"\x19" + ch[1][1:], ch[2]]), 32),
    # (the run's last key grows: the run still ascends)
    "pair-key-byte": (lambda: two_files(region=lambda ch: ch[:2] + [ch[2][:40 + 8 + 15] + b"z" + ch[2][40 + 8 + 16:]]), 32),
    "gap-between-handles": (lambda: two_files(None, handles=lambda h: h.__setitem__(slice(3, 6), [(o + 4, 40) for o, _ in h[3:]]),
                                              region=lambda ch: [ch[0][:120] + b"\0\0\0\0" + ch[0][120:]]), 32),
}


def host_args(c):
    return [t[0] for t in c["tables"]], [t[1] for t in c["tables"]], c["runs"]


def total(c):
    """The listed files' entry total, by their index blocks' counts."""
    return sum(int.from_bytes(c["tables"][f][0][-9:-5], "little") for run in c["runs"] for f in run)
