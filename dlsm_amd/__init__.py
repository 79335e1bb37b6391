"""dlsm_amd -- MI355X-native SSTable Bloom-filter engine for dLSM.

Python face of the C ABI (``include/dlsm_bloom.h``).  The compute path is the
hand-written gfx950 HIP library ``dlsm_amd/lib/libdlsm_bloom.so``; this package
only marshals buffers (numpy arrays for host memory, torch tensors for device
memory) and mirrors the reference's class surface:

* :class:`FullFilterBlockBuilder` / :class:`FullFilterBlockReader`
  (table/full_filter_block.h:33-94)
* :class:`BloomFilterPolicy` (include/TimberSaw/filter_policy.h:31-71,
  util/bloom.cc)

There is no CPU fallback: without the HIP library every call raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib as _L
from ._lib import (BLOCK_CHECKSUM, BLOCK_FILTER, BLOCK_INDEX, BLOCK_OK, BLOCK_SHORT, BLOCK_TYPE, BlockError,
                   DlsmError, check, dlsm_build_job, dlsm_keyset)

__all__ = [
    "Keys", "Context", "FilterSet", "DlsmError", "BlockError", "BLOCK_OK", "BLOCK_SHORT", "BLOCK_CHECKSUM",
    "BLOCK_TYPE", "BLOCK_FILTER", "device_available", "bloom_hash",
    "full_size", "legacy_size", "full_parse", "FullFilterBlockBuilder",
    "FullFilterBlockReader", "BloomFilterPolicy", "PATH_AUTO", "PATH_DIRECT", "PATH_SLICED",
    "crc32c", "crc32c_mask", "Version", "VersionFile", "PLAN_FIRST", "PLAN_ALL", "read_plan_chunk",
    "ShardMap", "MAX_SHARDS", "ROUTE_ALIGN", "shard_route_cap", "shard_route_chunk",
    "TableIndex", "BLOCK_INDEX", "GET_NOTFOUND", "GET_FOUND", "GET_DELETED", "GET_CORRUPT", "KV_HANDLE",
    "index_fence_interval", "index_seek_block", "index_block_check", "index_block_seek",
    "TableData", "kv_read_chunk", "kv_read_span", "kv_pair_read",
    "table_build", "table_build_chunk", "table_build_span", "table_build_bound",
    "compaction_merge", "merge_tile", "merge_span", "merge_chunk", "MERGE_KEEP_ALL", "MERGE_DROP_HIDDEN",
    "compaction_merge_tables", "MERGE_TABLE_MISMATCH", "range_scan", "SCAN_MAX_LIMIT", "SCAN_KEYS_CAP",
    "SCAN_VALUES_CAP", "SCAN_PAIR_CAP", "SCAN_BAD_TYPE", "SCAN_TABLE_MISMATCH", "memtable_sort", "sort_tile",
    "compaction_output", "compaction_output_bound", "output_tables", "OUTPUT_FILE_FIELDS", "OUTPUT_MAX_FILES", "OUTPUT_FILE_CAP", "OUTPUT_INPUT_FLAGGED",
    "compaction_filters", "compaction_filters_bound", "filter_blocks", "FILTER_REC_FIELDS", "FILTERS_MAX_SLICES", "FILTERS_CAP",
    "FILTERS_TOO_MANY_LINES", "FILTERS_INPUT_FLAGGED",
]

PATH_AUTO, PATH_DIRECT, PATH_SLICED = 0, 1, 2
INTERNAL_KEY_TRAILER = 8  # dlsm_keyset.suffix_len for internal keys (db/dbformat.h:374-377)
SELECT_FLUSH, SELECT_COMPACTION = 0, 1  # dlsm_internal_keys_select_dev policies
OPT_PATH, OPT_PROBE_ROUND_KEYS, OPT_BUILD_GROUPS = 0, 1, 2  # dlsm_ctx_set_option
OPT_PROBE_CHUNK_LG, OPT_PROBE_SLICE_LG, OPT_BUILD_EXACT, OPT_PROBE_ROUND_SERIAL = 3, 4, 5, 6
OPT_FAULT_INJECT = 7  # test hook: builds / probes on the context return -value
OPT_VERSION_SLICE_BYTES, OPT_VERSION_PASS_SLICES = 8, 9  # sliced version probe: level threshold, slices per pass
OPT_PROBE_MULTI = 10  # multi-group filter sets: 1 one pass over every group (default), 0 a pass per group
PLAN_FIRST, PLAN_ALL = 0, 1  # dlsm_version_read_plan_dev modes: each Get's lowest set slot / every set slot
MAX_SHARDS, ROUTE_ALIGN = 511, 4  # DLSM_MAX_SHARDS, DLSM_ROUTE_ALIGN
GET_NOTFOUND, GET_FOUND, GET_DELETED, GET_CORRUPT = 0, 1, 2, 3  # DLSM_GET_*: a seek task's (or a Get's) state
# dlsm_kv_handle as a numpy record (16 bytes); device arrays of it are uint8[n, 16] or int64[n, 2] tensors
KV_HANDLE = np.dtype([("offset", "<u8"), ("size", "<u4"), ("file", "<u4")])


def lib():
    return _L._lib()


def device_available() -> bool:
    n = C.c_int(0)
    try:
        lib().dlsm_device_count(C.byref(n))
    except OSError:
        return False
    return n.value > 0


def read_plan_chunk() -> int:
    """Gets per workgroup-chunk of the read plan's kernels."""
    return int(lib().dlsm_version_read_plan_chunk())


def shard_route_chunk() -> int:
    """Gets per workgroup-chunk of the shard route's kernels."""
    return int(lib().dlsm_shard_route_chunk())


def index_fence_interval() -> int:
    """Entries per fence of an opened table index."""
    return int(lib().dlsm_index_fence_interval())


def index_seek_block() -> int:
    """Tasks per workgroup step of the index seek's kernel."""
    return int(lib().dlsm_index_seek_block())


def index_block_check(contents: bytes) -> Optional[int]:
    """The open's validation of one index block's contents on the host: the
    entry count, or None where a rule fails."""
    a = np.frombuffer(bytes(contents) + b"\0", dtype=np.uint8)
    n = C.c_uint64()
    st = lib().dlsm_index_block_check(a.ctypes.data, len(contents), C.byref(n))
    if st == _L.DLSM_E_CORRUPT:
        return None
    check(st, "index_block_check")
    return int(n.value)


def index_block_seek(contents: bytes, user_key: bytes, snapshot: int, file: int = 0):
    """Table::InternalGet's index step for one key on the host: (state,
    offset, size, file)."""
    a = np.frombuffer(bytes(contents) + b"\0", dtype=np.uint8)
    k = np.frombuffer(bytes(user_key) + b"\0", dtype=np.uint8)
    st, h = C.c_uint8(), _L.dlsm_kv_handle()
    check(lib().dlsm_index_block_seek(a.ctypes.data, len(contents), k.ctypes.data, len(user_key), snapshot, file,
                                      C.byref(st), C.byref(h)), "index_block_seek")
    return int(st.value), int(h.offset), int(h.size), int(h.file)


def kv_read_chunk() -> int:
    """Items per workgroup chunk of the value read's size pass."""
    return int(lib().dlsm_kv_read_chunk())


def kv_read_span() -> int:
    """Output bytes per workgroup step of the value read's copy."""
    return int(lib().dlsm_kv_read_span())


TABLE_DATA_CAP, TABLE_INDEX_CAP, TABLE_CHUNK_CAP, TABLE_SHORT_KEY = 1, 2, 4, 8
TABLE_PAIR_TOO_BIG, TABLE_INDEX_TOO_BIG, TABLE_OVERSIZE_PAIR = 16, 32, 64


def table_build_chunk() -> int:
    """Pairs per workgroup chunk of the table build's size and offset passes."""
    return int(lib().dlsm_table_build_chunk())


def table_build_span() -> int:
    """Output bytes per workgroup step of the table build's region write."""
    return int(lib().dlsm_table_build_span())


def table_build_bound(n: int, key_bytes: int, value_bytes: int):
    """(the region's exact length, an index capacity no block of the pairs passes)."""
    d, x = C.c_uint64(), C.c_uint64()
    check(lib().dlsm_table_build_bound(n, key_bytes, value_bytes, C.byref(d), C.byref(x)), "table_build_bound")
    return int(d.value), int(x.value)


def _table_io(keys: "Keys", values, value_off, value_len: int, chunk_bytes: int, data, data_cap, index, index_cap,
              chunk_end, chunk_cap, built):
    n = keys.n
    if value_off is not None:
        _need(value_off, 8 * (n + 1), "value_off")
    else:
        _need(values, n * value_len, "values")
    data_cap = _nbytes(data) if data_cap is None else int(data_cap)
    index_cap = _nbytes(index) if index_cap is None else int(index_cap)
    chunk_cap = _nbytes(chunk_end) // 8 if chunk_cap is None else int(chunk_cap)
    for x, nb, what in ((data, data_cap, "data"), (index, index_cap, "index"), (chunk_end, 8 * chunk_cap, "chunk_end"),
                        (built, 32, "built")):
        _need(x, nb, what)
    ti = _L.dlsm_table_input(keys.c(), _ptr(values), _ptr(value_off), value_len, chunk_bytes)
    to = _L.dlsm_table_output(_ptr(data), data_cap, _ptr(index), index_cap, _ptr(chunk_end), chunk_cap, _ptr(built))
    return ti, to


def table_build(keys: "Keys", values: np.ndarray, *, value_off: Optional[np.ndarray] = None, value_len: int = 0,
                chunk_bytes: int = 0, data_cap: Optional[int] = None, index_cap: Optional[int] = None,
                chunk_cap: Optional[int] = None, ctx: Optional["Context"] = None):
    """The host form of the table build (dlsm_table_build; no device is
    touched): ``keys`` are the internal keys in table order (host arrays),
    ``values`` the packed values with ``value_off`` (uint64[n + 1]) or one
    ``value_len``.  Returns (data uint8, index uint8, chunk_end uint64, built)
    with built = (data_bytes, index_bytes, n_chunks, flags); the arrays are cut
    at min(total, cap).  The caps default to what the pairs need."""
    n = keys.n
    kb = int(keys.offsets[n] - keys.offsets[0]) if keys.offsets is not None else n * keys.key_len
    vb = int(value_off[n] - value_off[0]) if value_off is not None else n * value_len
    need_d, need_i = table_build_bound(n, kb, vb)
    data_cap = need_d if data_cap is None else int(data_cap)
    index_cap = need_i if index_cap is None else int(index_cap)
    chunk_cap = n + 1 if chunk_cap is None else int(chunk_cap)
    data, index = np.zeros(max(data_cap, 1), dtype=np.uint8), np.zeros(max(index_cap, 1), dtype=np.uint8)
    ends, built = np.zeros(max(chunk_cap, 1), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    ti, to = _table_io(keys, values, value_off, value_len, chunk_bytes, data, data_cap, index, index_cap, ends,
                       chunk_cap, built)
    check(lib().dlsm_table_build(ctx.h if ctx is not None else None, C.byref(ti), C.byref(to)), "table_build")
    b = tuple(int(x) for x in built)
    return data[:min(b[0], data_cap)], index[:min(b[1], index_cap)], ends[:min(b[2], chunk_cap)], b


MERGE_KEEP_ALL, MERGE_DROP_HIDDEN = 0, 1  # dlsm_compaction_merge policies
MERGE_KEYS_CAP, MERGE_VALUES_CAP, MERGE_PAIR_CAP, MERGE_SHORT_KEY, MERGE_UNSORTED = 1, 2, 4, 8, 16
MERGE_TABLE_MISMATCH = 32


def merge_tile() -> int:
    """Records per workgroup step of a compaction merge pass."""
    return int(lib().dlsm_merge_tile())


def merge_span() -> int:
    """Output bytes per workgroup step of the compaction merge's gather."""
    return int(lib().dlsm_merge_span())


def merge_chunk() -> int:
    """Pairs per workgroup chunk of the compaction merge's record, decide and offset passes."""
    return int(lib().dlsm_merge_chunk())


def _merge_io(runs, keys, keys_cap, key_off, values, values_cap, value_off, src, pair_cap, merged):
    """runs: (Keys, values, value_off or None, value_len) per sorted run."""
    if not 1 <= len(runs) <= 64:
        raise ValueError("compaction_merge: 1 to 64 runs")
    mr = (_L.dlsm_merge_run * len(runs))()
    for r, (k, v, vo, vl) in enumerate(runs):
        if vo is not None:
            _need(vo, 8 * (k.n + 1), "value_off")
        else:
            _need(v, k.n * vl, "values")
        mr[r] = _L.dlsm_merge_run(k.c(), _ptr(v), _ptr(vo), vl)
    return mr, _merge_out(keys, keys_cap, key_off, values, values_cap, value_off, src, pair_cap, merged)


def _merge_out(keys, keys_cap, key_off, values, values_cap, value_off, src, pair_cap, merged):
    keys_cap = _nbytes(keys) if keys_cap is None else int(keys_cap)
    values_cap = _nbytes(values) if values_cap is None else int(values_cap)
    pair_cap = max(_nbytes(key_off) // 8 - 1, 0) if pair_cap is None else int(pair_cap)
    for x, nb, what in ((keys, keys_cap, "keys"), (values, values_cap, "values"), (key_off, 8 * (pair_cap + 1), "key_off"),
                        (value_off, 8 * (pair_cap + 1), "value_off"), (merged, 40, "merged")):
        _need(x, nb, what)
    if src is not None:
        _need(src, 8 * pair_cap, "src")
    mo = _L.dlsm_merge_output(_ptr(keys), keys_cap, _ptr(key_off), _ptr(values), values_cap, _ptr(value_off), _ptr(src),
                              pair_cap, _ptr(merged))
    return mo


def _table_runs(runs):
    """runs: a list of file-number lists.  Returns (dlsm_table_run array, what it points into)."""
    keep = [np.ascontiguousarray(r, dtype=np.uint32) for r in runs]
    tr = (_L.dlsm_table_run * max(len(runs), 1))()
    for r, a in enumerate(keep):
        tr[r] = _L.dlsm_table_run(a.ctypes.data_as(C.POINTER(C.c_uint32)) if a.size else None, a.size)
    return tr, keep


def _host_tables(blocks, files, what):
    """Sealed index blocks (bytes or None) and chunk lists in the host forms'
    argument form: (n, block pointers, lengths, chunk records, chunk_begin,
    what they point into)."""
    n = len(blocks)
    if len(files) != n:
        raise ValueError(what + ": one chunk list per block")
    bk = [None if b is None else np.frombuffer(bytes(b) + b"\0", dtype=np.uint8) for b in blocks]
    pa = (C.c_void_p * max(n, 1))(*[None if a is None else a.ctypes.data for a in bk])
    la = (C.c_uint64 * max(n, 1))(*[0 if a is None else a.size - 1 for a in bk])
    begin = np.zeros(n + 1, dtype=np.uint32)
    ck, recs = [], []
    for f, chunks in enumerate(files):
        for c in (chunks or []):
            ck.append(np.frombuffer(bytes(c) + b"\0", dtype=np.uint8))
            recs.append(_L.dlsm_data_chunk(ck[-1].ctypes.data, ck[-1].size - 1))
        begin[f + 1] = len(recs)
    ca = (_L.dlsm_data_chunk * max(len(recs), 1))(*recs)
    return n, pa, la, ca, begin, (bk, ck)


def compaction_merge_tables(blocks, files, runs, policy: int = MERGE_DROP_HIDDEN, smallest_snapshot: int = 0, *,
                            keys_cap: int, values_cap: int, pair_cap: int, ctx: Optional["Context"] = None):
    """The host form of the merge out of tables (dlsm_compaction_merge_tables;
    no device is touched): ``blocks[f]`` is file f's sealed index block (bytes)
    or None, ``files[f]`` the list of its data chunks (bytes) as for TableIndex
    and TableData, ``runs`` a list of file-number lists -- a level-0 file each,
    or a deeper level's files in key order.  The caps size the outputs.
    Returns what compaction_merge returns, src counting through each run's
    concatenated files."""
    n, pa, la, ca, begin, _held = _host_tables(blocks, files, "compaction_merge_tables")
    tr, _keep = _table_runs(runs)
    keys, values = np.zeros(max(keys_cap, 1), dtype=np.uint8), np.zeros(max(values_cap, 1), dtype=np.uint8)
    key_off, value_off = np.zeros(pair_cap + 1, dtype=np.uint64), np.zeros(pair_cap + 1, dtype=np.uint64)
    src, merged = np.zeros(max(pair_cap, 1), dtype=np.uint64), np.zeros(5, dtype=np.uint64)
    mo = _merge_out(keys, keys_cap, key_off, values, values_cap, value_off, src, pair_cap, merged)
    check(lib().dlsm_compaction_merge_tables(ctx.h if ctx is not None else None, pa, la, ca,
                                             begin.ctypes.data_as(C.POINTER(C.c_uint32)), n, tr, len(runs), policy,
                                             smallest_snapshot, C.byref(mo)), "compaction_merge_tables")
    m = tuple(int(x) for x in merged)
    p = min(m[1], pair_cap)
    return (keys[:min(m[2], keys_cap)], key_off[:p + 1], values[:min(m[3], values_cap)], value_off[:p + 1], src[:p], m)


SCAN_MAX_LIMIT = 1024  # DLSM_SCAN_MAX_LIMIT
SCAN_KEYS_CAP, SCAN_VALUES_CAP, SCAN_PAIR_CAP, SCAN_BAD_TYPE, SCAN_TABLE_MISMATCH = 1, 2, 4, 8, 32


def _scan_out(q, limit, count, pair_begin, handle, keys, keys_cap, key_off, values, values_cap, value_off, pair_cap,
              scanned):
    for x, nb, what in ((count, 4 * q, "count"), (pair_begin, 8 * (q + 1), "pair_begin"), (handle, 16 * q * limit, "handle"),
                        (keys, keys_cap, "keys"), (values, values_cap, "values"), (key_off, 8 * (pair_cap + 1), "key_off"),
                        (value_off, 8 * (pair_cap + 1), "value_off"), (scanned, 40, "scanned")):
        _need(x, nb, what)
    return _L.dlsm_scan_output(_ptr(count), _ptr(pair_begin), _ptr(handle), _ptr(keys), keys_cap, _ptr(key_off),
                               _ptr(values), values_cap, _ptr(value_off), pair_cap, _ptr(scanned))


def range_scan(blocks, files, runs, starts: "Keys", snapshot: int, limit: int, *, keys_cap: int, values_cap: int,
               pair_cap: int, ctx: Optional["Context"] = None):
    """The host form of the range scan (dlsm_range_scan; no device is touched):
    tables and ``runs`` as for compaction_merge_tables, ``starts`` the scans'
    start user keys (host arrays).  Scan q is Seek(starts[q]) and Next() until
    ``limit`` pairs are yielded under ``snapshot``.  The caps size the outputs.
    Returns a dict: count uint32[Q], pair_begin uint64[Q + 1], handle
    uint64[Q * limit, 2] (offset, size | file << 32), keys, key_off, values,
    value_off (cut at min(total, cap)) and scanned = (n_scans, n_pairs,
    key_bytes, value_bytes, flags)."""
    n, pa, la, ca, begin, _held = _host_tables(blocks, files, "range_scan")
    tr, _keep = _table_runs(runs)
    q = starts.n
    o = dict(count=np.zeros(q, dtype=np.uint32), pair_begin=np.zeros(q + 1, dtype=np.uint64),
             handle=np.zeros((q * limit, 2), dtype=np.uint64), keys=np.zeros(max(keys_cap, 1), dtype=np.uint8),
             key_off=np.zeros(pair_cap + 1, dtype=np.uint64), values=np.zeros(max(values_cap, 1), dtype=np.uint8),
             value_off=np.zeros(pair_cap + 1, dtype=np.uint64), scanned=np.zeros(5, dtype=np.uint64))
    so = _scan_out(q, limit, o["count"], o["pair_begin"], o["handle"], o["keys"], keys_cap, o["key_off"], o["values"],
                   values_cap, o["value_off"], pair_cap, o["scanned"])
    ks = starts.c()
    check(lib().dlsm_range_scan(ctx.h if ctx is not None else None, pa, la, ca, begin.ctypes.data_as(C.POINTER(C.c_uint32)),
                                n, tr, len(runs), C.byref(ks), snapshot, limit, C.byref(so)), "range_scan")
    m = tuple(int(x) for x in o["scanned"])
    p = min(m[1], pair_cap)
    o.update(keys=o["keys"][:min(m[2], keys_cap)], values=o["values"][:min(m[3], values_cap)], key_off=o["key_off"][:p + 1],
             value_off=o["value_off"][:p + 1], scanned=m)
    return o


def compaction_merge(runs, policy: int = MERGE_DROP_HIDDEN, smallest_snapshot: int = 0, *,
                     keys_cap: Optional[int] = None, values_cap: Optional[int] = None, pair_cap: Optional[int] = None,
                     ctx: Optional["Context"] = None):
    """The host form of the compaction merge (dlsm_compaction_merge; no device
    is touched): ``runs`` is a list of (Keys, values, value_off or None,
    value_len) over host arrays, each run sorted.  Returns (keys uint8,
    key_off uint64, values uint8, value_off uint64, src uint64, merged) with
    merged = (n_in, n_out, key_bytes, value_bytes, flags); the arrays are cut at
    min(total, cap).  The caps default to what the inputs hold."""
    return _merge_host(runs, policy, smallest_snapshot, keys_cap, values_cap, pair_cap, ctx, False)


def sort_tile() -> int:
    """Records one workgroup of the memtable sort sorts in LDS."""
    return int(lib().dlsm_memtable_sort_tile())


def memtable_sort(batch, policy: int = MERGE_DROP_HIDDEN, smallest_snapshot: int = 0, *,
                  keys_cap: Optional[int] = None, values_cap: Optional[int] = None, pair_cap: Optional[int] = None,
                  ctx: Optional["Context"] = None):
    """The host form of the memtable sort (dlsm_memtable_sort; no device is
    touched): ``batch`` is one (Keys, values, value_off or None, value_len)
    over host arrays, in arrival order.  Returns what compaction_merge returns,
    the pairs in InternalKeyComparator order and src the input index of each."""
    return _merge_host([batch], policy, smallest_snapshot, keys_cap, values_cap, pair_cap, ctx, True)


def _merge_host(runs, policy, smallest_snapshot, keys_cap, values_cap, pair_cap, ctx, sort):
    """compaction_merge, or memtable_sort of the one run."""
    def nb(x, off, n, ln):
        return int(off[n] - off[0]) if off is not None else n * ln

    n = sum(k.n for k, _, _, _ in runs)
    kb = sum(nb(k.data, k.offsets, k.n, k.key_len) for k, _, _, _ in runs)
    vb = sum(nb(v, vo, k.n, vl) for k, v, vo, vl in runs)
    keys_cap = kb if keys_cap is None else int(keys_cap)
    values_cap = vb if values_cap is None else int(values_cap)
    pair_cap = n if pair_cap is None else int(pair_cap)
    keys, values = np.zeros(max(keys_cap, 1), dtype=np.uint8), np.zeros(max(values_cap, 1), dtype=np.uint8)
    key_off, value_off = np.zeros(pair_cap + 1, dtype=np.uint64), np.zeros(pair_cap + 1, dtype=np.uint64)
    src, merged = np.zeros(max(pair_cap, 1), dtype=np.uint64), np.zeros(5, dtype=np.uint64)
    mr, mo = _merge_io(runs, keys, keys_cap, key_off, values, values_cap, value_off, src, pair_cap, merged)
    h = ctx.h if ctx is not None else None
    if sort:
        check(lib().dlsm_memtable_sort(h, mr, policy, smallest_snapshot, C.byref(mo)), "memtable_sort")
    else:
        check(lib().dlsm_compaction_merge(h, mr, len(runs), policy, smallest_snapshot, C.byref(mo)), "compaction_merge")
    m = tuple(int(x) for x in merged)
    p = min(m[1], pair_cap)
    return (keys[:min(m[2], keys_cap)], key_off[:p + 1], values[:min(m[3], values_cap)], value_off[:p + 1], src[:p], m)


OUTPUT_MAX_FILES, OUTPUT_FILE_CAP, OUTPUT_INPUT_FLAGGED = 4096, 128, 256  # the other bits are the TABLE_* ones
OUTPUT_FILE_FIELDS = ("first", "n", "data_base", "data_bytes", "index_base", "index_bytes", "chunk_base", "n_chunks",
                      "flags")  # a dlsm_output_file: nine uint64


def compaction_output_bound(pair_cap: int, key_bytes: int, value_bytes: int, max_file_bytes: int, chunk_bytes: int):
    """(data_cap, index_cap, chunk_cap, file_cap) that no output of such a run passes."""
    v = [C.c_uint64() for _ in range(4)]
    check(lib().dlsm_compaction_output_bound(pair_cap, key_bytes, value_bytes, max_file_bytes, chunk_bytes,
                                             *[C.byref(x) for x in v]), "compaction_output_bound")
    return tuple(int(x.value) for x in v)


def _output_io(keys: "Keys", values, value_off, value_len: int, merged, max_file_bytes: int, chunk_bytes: int, data,
               data_cap, index, index_cap, chunk_end, chunk_cap, files, file_cap, built):
    n = keys.n
    if value_off is not None:
        _need(value_off, 8 * (n + 1), "value_off")
    else:
        _need(values, n * value_len, "values")
    data_cap = _nbytes(data) if data_cap is None else int(data_cap)
    index_cap = _nbytes(index) if index_cap is None else int(index_cap)
    chunk_cap = _nbytes(chunk_end) // 8 if chunk_cap is None else int(chunk_cap)
    file_cap = _nbytes(files) // 72 if file_cap is None else int(file_cap)
    for x, nb, what in ((data, data_cap, "data"), (index, index_cap, "index"), (chunk_end, 8 * chunk_cap, "chunk_end"),
                        (files, 72 * file_cap, "files"), (built, 40, "built"), (merged, 40, "merged")):
        _need(x, nb, what)
    oi = _L.dlsm_output_input(keys.c(), _ptr(values), _ptr(value_off), value_len, _ptr(merged), max_file_bytes,
                              chunk_bytes)
    oo = _L.dlsm_output_output(_ptr(data), data_cap, _ptr(index), index_cap, _ptr(chunk_end), chunk_cap, _ptr(files),
                               file_cap, _ptr(built))
    return oi, oo


def compaction_output(keys: "Keys", values: np.ndarray, merged, *, value_off: Optional[np.ndarray] = None,
                      value_len: int = 0, max_file_bytes: int = 0, chunk_bytes: int = 0, data_cap: Optional[int] = None,
                      index_cap: Optional[int] = None, chunk_cap: Optional[int] = None, file_cap: Optional[int] = None,
                      ctx: Optional["Context"] = None):
    """The host form of the compaction output (dlsm_compaction_output; no
    device is touched): the run a compaction merge returned -- ``keys`` with
    keys.n the pair capacity, ``values``, ``merged`` (its five-number record, of
    which n_out pairs are taken) -- cut at ``max_file_bytes`` and built file by
    file.  Returns (tables, files, built): per file below the caps (data uint8,
    chunk_end uint64, index_block uint8), the file records (uint64[F, 9],
    OUTPUT_FILE_FIELDS) and built = (n_files, data_bytes, index_bytes, n_chunks,
    flags).  The caps default to dlsm_compaction_output_bound's."""
    n = keys.n
    kb = int(keys.offsets[n] - keys.offsets[0]) if keys.offsets is not None else n * keys.key_len
    vb = int(value_off[n] - value_off[0]) if value_off is not None else n * value_len
    need = compaction_output_bound(n, kb, vb, max_file_bytes, chunk_bytes)
    need = need[:3] + (min(need[3], OUTPUT_MAX_FILES),)
    data_cap, index_cap, chunk_cap, file_cap = (b if c is None else int(c) for b, c in
                                                zip(need, (data_cap, index_cap, chunk_cap, file_cap)))
    data, index = np.zeros(max(data_cap, 1), dtype=np.uint8), np.zeros(max(index_cap, 1), dtype=np.uint8)
    ends, files = np.zeros(max(chunk_cap, 1), dtype=np.uint64), np.zeros((max(file_cap, 1), 9), dtype=np.uint64)
    built, m = np.zeros(5, dtype=np.uint64), np.ascontiguousarray(merged, dtype=np.uint64)
    oi, oo = _output_io(keys, values, value_off, value_len, m, max_file_bytes, chunk_bytes, data, data_cap, index,
                        index_cap, ends, chunk_cap, files, file_cap, built)
    check(lib().dlsm_compaction_output(ctx.h if ctx is not None else None, C.byref(oi), C.byref(oo)),
          "compaction_output")
    b = tuple(int(x) for x in built)
    files = files[:min(b[0], file_cap)]
    return output_tables(data[:data_cap], index[:index_cap], ends[:chunk_cap], files), files, b


FILTERS_MAX_SLICES, FILTERS_CAP, FILTERS_TOO_MANY_LINES, FILTERS_INPUT_FLAGGED = 512, 1, 2, 256
FILTER_REC_FIELDS = ("base", "bytes", "n_distinct", "num_lines")  # a dlsm_output_filter: four uint64


def compaction_filters_bound(pair_cap: int, file_cap: int, bits_per_key: int = 10) -> int:
    """filters_cap that the filter blocks of no cut of such a run pass."""
    v = C.c_uint64()
    check(lib().dlsm_compaction_filters_bound(pair_cap, file_cap, bits_per_key, C.byref(v)), "compaction_filters_bound")
    return int(v.value)


def _filters_io(keys: "Keys", merged, files, out_built, file_cap, bits_per_key: int, filters, filters_cap, recs, built):
    file_cap = _nbytes(files) // 72 if file_cap is None else int(file_cap)
    filters_cap = _nbytes(filters) if filters_cap is None else int(filters_cap)
    for x, nb, what in ((files, 72 * file_cap, "files"), (recs, 32 * file_cap, "recs"), (filters, filters_cap, "filters"),
                        (merged, 40, "merged"), (out_built, 40, "out_built"), (built, 24, "built")):
        _need(x, nb, what)
    fi = _L.dlsm_filters_input(keys.c(), _ptr(merged), _ptr(files), _ptr(out_built), file_cap, bits_per_key)
    fo = _L.dlsm_filters_output(_ptr(filters), filters_cap, _ptr(recs), _ptr(built))
    return fi, fo


def compaction_filters(keys: "Keys", merged, files, out_built, *, bits_per_key: int = 10,
                       filters_cap: Optional[int] = None, ctx: Optional["Context"] = None):
    """The host form of the compaction filters (dlsm_compaction_filters; no
    device is touched): the run as compaction_output took it, and the file
    records (uint64[F, 9]) and totals it returned.  Returns (blocks, recs,
    built): the sealed filter block of every file that lies below
    ``filters_cap`` (uint8 each, None for one that does not), the records
    (uint64[F, 4], FILTER_REC_FIELDS) and built = (n_files, filter_bytes,
    flags).  filters_cap defaults to dlsm_compaction_filters_bound's."""
    files = np.ascontiguousarray(files, dtype=np.uint64).reshape(-1, 9)
    file_cap = len(files)
    if filters_cap is None:
        filters_cap = compaction_filters_bound(keys.n, file_cap, bits_per_key)
    filters, recs = np.zeros(max(filters_cap, 1), dtype=np.uint8), np.zeros((max(file_cap, 1), 4), dtype=np.uint64)
    built = np.zeros(3, dtype=np.uint64)
    fi, fo = _filters_io(keys, np.ascontiguousarray(merged, dtype=np.uint64), files if file_cap else np.zeros(9, np.uint64),
                         np.ascontiguousarray(out_built, dtype=np.uint64), file_cap, bits_per_key, filters, filters_cap,
                         recs, built)
    check(lib().dlsm_compaction_filters(ctx.h if ctx is not None else None, C.byref(fi), C.byref(fo)),
          "compaction_filters")
    b = tuple(int(x) for x in built)
    recs = recs[:b[0]]
    return filter_blocks(filters[:filters_cap], recs), recs, b


def filter_blocks(filters, recs):
    """Slice a compaction filters call's buffer by its records: the sealed
    block per file, None for a file that does not lie wholly in the buffer."""
    end = _nbytes(filters)
    return [filters[int(r[0]):int(r[0] + r[1])] if int(r[0] + r[1]) <= end else None for r in recs]


def output_tables(data, index, chunk_end, files):
    """Slice a compaction output's buffers by its file records: (data,
    chunk_end, index_block) per file, each cut at its buffer's end."""
    out = []
    for r in files:
        r = {k: int(v) for k, v in zip(OUTPUT_FILE_FIELDS, r)}
        out.append((data[r["data_base"]:r["data_base"] + r["data_bytes"]],
                    chunk_end[r["chunk_base"]:r["chunk_base"] + r["n_chunks"]],
                    index[r["index_base"]:r["index_base"] + r["index_bytes"]]))
    return out


def kv_pair_read(chunks, handle, user_key: bytes, state: int = GET_FOUND):
    """The value read of one Get on the host: ``chunks`` are one file's data
    chunks (bytes each, in offset order), ``handle`` is (offset, size[, file]).
    Returns (state, value) with value None unless the state is GET_FOUND."""
    keep = [np.frombuffer(bytes(c) + b"\0", dtype=np.uint8) for c in chunks]
    ca = (_L.dlsm_data_chunk * max(len(keep), 1))(*[_L.dlsm_data_chunk(a.ctypes.data, a.size - 1) for a in keep])
    h = _L.dlsm_kv_handle(int(handle[0]), int(handle[1]), int(handle[2]) if len(handle) > 2 else 0)
    k = np.frombuffer(bytes(user_key) + b"\0", dtype=np.uint8)
    st, v, vl = C.c_uint8(state), C.c_void_p(), C.c_uint32()
    check(lib().dlsm_kv_pair_read(ca, len(keep), C.byref(h), k.ctypes.data, len(user_key), C.byref(st), C.byref(v),
                                  C.byref(vl)), "kv_pair_read")
    if st.value != GET_FOUND:
        return int(st.value), None
    return GET_FOUND, C.string_at(v.value, vl.value) if vl.value else b""


def shard_route_cap(n: int, n_shards: int) -> int:
    """Slots of ``gets`` (and rows of ``keys_out``) a route of n Gets over
    n_shards shards needs: n + 3 per bin, rounded up to ROUTE_ALIGN."""
    return int(lib().dlsm_shard_route_cap(n, n_shards))


def bloom_hash(key: bytes) -> int:
    """BloomHash (include/TimberSaw/filter_policy.h:26-28), host side."""
    b = C.create_string_buffer(bytes(key), len(key) + 1)
    return int(lib().dlsm_bloom_hash(b, len(key)))


class PinnedArray:
    """A page-locked host uint8 array (dlsm_host_alloc), freed on close()."""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        check(lib().dlsm_host_alloc(nbytes, C.byref(p)), "host_alloc")
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(self.ptr))

    def close(self):
        if self.ptr:
            lib().dlsm_host_free(C.c_void_p(self.ptr))
            self.ptr = None
            self.array = None


def full_size(n_dedup: int, bits_per_key: int = 10):
    L = C.c_uint32(0)
    nb = C.c_uint64(0)
    check(lib().dlsm_bloom_full_size(n_dedup, bits_per_key, C.byref(L), C.byref(nb)))
    return int(nb.value), int(L.value)


def legacy_size(n: int, bits_per_key: int = 10) -> int:
    nb = C.c_uint64(0)
    check(lib().dlsm_bloom_legacy_size(n, bits_per_key, C.byref(nb)))
    return int(nb.value)


def full_parse(filt: bytes):
    """(status, num_probes, num_lines, log2_line) -- FullFilterBlockReader ctor."""
    b = C.create_string_buffer(bytes(filt), max(len(filt), 1))
    k, L, lg = C.c_int(0), C.c_uint32(0), C.c_int(0)
    st = lib().dlsm_bloom_full_parse(b, len(filt), C.byref(k), C.byref(L), C.byref(lg))
    return st, k.value, L.value, lg.value


def crc32c(data: bytes, init: int = 0) -> int:
    """crc32c::Extend(init, data) (util/crc32c.h:17-22), host helper."""
    b = C.create_string_buffer(bytes(data), len(data) + 1)
    return int(lib().dlsm_crc32c_extend(init, b, len(data)))


def hash_batch(keys: "Keys", out: Optional[np.ndarray] = None, threads: int = 0) -> np.ndarray:
    """BloomHash of every key of a host key set on the host's cores
    (dlsm_bloom_hash_batch): uint32[n], numpy or a pinned torch CPU tensor's
    storage passed as ``out``."""
    if out is None:
        out = np.empty(max(keys.n, 1), dtype=np.uint32)
    if isinstance(out, np.ndarray):
        ok = out.itemsize == 4 and out.size >= keys.n and out.flags["C_CONTIGUOUS"]
    else:  # a torch CPU tensor
        ok = out.element_size() == 4 and out.numel() >= keys.n and out.is_contiguous() and not out.is_cuda
    if not ok:
        raise ValueError("hash_batch: `out` must be contiguous host memory of >= n 4-byte elements")
    ks = keys.c()
    check(lib().dlsm_bloom_hash_batch(C.byref(ks), _ptr(out), threads), "hash_batch")
    return out[: keys.n] if isinstance(out, np.ndarray) else out


def host_read_bytes(buf, threads: int = 0) -> int:
    """Stream a host buffer (numpy array or CPU torch tensor, size a multiple
    of 8 bytes) on the host-hash pool, NUMA-placed like hash_batch
    (dlsm_host_read_bytes); returns the XOR fold of its 64-bit words."""
    n = buf.nbytes if isinstance(buf, np.ndarray) else buf.numel() * buf.element_size()
    fold = C.c_uint64(0)
    check(lib().dlsm_host_read_bytes(_ptr(buf), n, threads, C.byref(fold)), "host_read_bytes")
    return int(fold.value)


def crc32c_mask(crc: int) -> int:
    return int(lib().dlsm_crc32c_mask(crc))


def _ptr(x) -> Optional[int]:
    """Address of a numpy array or torch tensor (host or device)."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return int(x.data_ptr())


def _nbytes(x) -> int:
    """Bytes of a numpy array or torch tensor (0 for None)."""
    if x is None:
        return 0
    if isinstance(x, np.ndarray):
        return int(x.nbytes)
    return int(x.numel()) * int(x.element_size())


def _need(x, nbytes: int, what: str):
    """The binding's guard: a buffer the library writes or reads through a raw
    pointer must hold at least nbytes (a short device buffer would be written
    past its end by the kernels)."""
    if _nbytes(x) < nbytes:
        raise ValueError(f"{what}: buffer of {_nbytes(x)} bytes, {nbytes} needed")


def cu_subset(per_xcd: int, n_cus: int = 256, n_xcds: int = 8) -> list:
    """per_xcd compute units on each XCD under both CU-mask numberings a
    multi-XCD part may use (bit i on XCD i // (n_cus / n_xcds), or on XCD
    i % n_xcds): i = (n_cus / n_xcds) x + n_xcds j + x, j < per_xcd <= 4."""
    per = n_cus // n_xcds
    if not 1 <= per_xcd <= per // n_xcds:
        raise ValueError(f"per_xcd must be in [1, {per // n_xcds}]")
    return sorted(per * x + n_xcds * j + x for x in range(n_xcds) for j in range(per_xcd))


def cu_mask_stream(device: int, cus, n_cus: int = 256):
    """A torch ExternalStream over a new hipStream_t restricted to the CUs in
    `cus` (dlsm_stream_create_cu_mask).  The stream lives as long as the process."""
    import torch

    words = (C.c_uint32 * ((n_cus + 31) // 32))()
    for i in cus:
        words[i // 32] |= 1 << (i % 32)
    raw = C.c_void_p()
    check(lib().dlsm_stream_create_cu_mask(device, words, len(words), C.byref(raw)), "cu_mask_stream")
    return torch.cuda.ExternalStream(raw.value, device=torch.device("cuda", device))


@dataclass
class Keys:
    """A packed key set: ``data`` (uint8) + ``offsets`` (uint64[n+1]) or fixed ``key_len``.

    ``data``/``offsets`` are numpy arrays (host) or torch tensors (device)."""
    data: object
    n: int
    key_len: int = 20
    offsets: object = None
    suffix_len: int = 0  # INTERNAL_KEY_TRAILER: internal keys, hashed as ExtractUserKey(key)

    def c(self) -> dlsm_keyset:
        if self.offsets is None:
            _need(self.data, self.n * self.key_len, "Keys.data")
        else:
            _need(self.offsets, 8 * (self.n + 1), "Keys.offsets")
            # host offsets: the data must also hold the bytes they index (key
            # n-1 ends at offsets[n]); device offsets are not read back here (a
            # synchronising copy per call), the caller vouches for them
            if isinstance(self.offsets, np.ndarray) and self.n:
                _need(self.data, int(self.offsets[self.n]), "Keys.data")
        return dlsm_keyset(_ptr(self.data), _ptr(self.offsets), self.key_len, self.suffix_len, self.n)

    @staticmethod
    def pack(keys: Sequence[bytes]) -> "Keys":
        offs = np.zeros(len(keys) + 1, dtype=np.uint64)
        if keys:
            offs[1:] = np.cumsum([len(k) for k in keys])
        data = np.frombuffer(b"".join(keys) + b"\0" * 16, dtype=np.uint8).copy()
        return Keys(data, len(keys), 0, offs)


@dataclass
class VersionFile:
    """One SSTable of a version (RemoteMemTableMetaData's smallest / largest /
    number + its full filter).  ``largest_trailer`` = seq << 8 | type of the
    largest internal key; ``filter`` = bytes (host) or a device uint8 tensor,
    or None for a table without a filter."""
    level: int
    number: int
    smallest: bytes
    largest: bytes
    largest_trailer: int
    filter: object = None


class Version:
    """A version's files and filters resident on one device (search order:
    level-0 newest first, then one candidate per level 1..5)."""
    NUM_LEVELS = 6

    def __init__(self, ctx: "Context", files: Sequence[VersionFile], on_device: bool = False, *,
                 sealed: bool = False, verify_checksums: bool = True):
        """sealed: every file's ``filter`` is its sealed filter block (filter +
        5-byte trailer), verified on the device; a bad block raises BlockError."""
        n = len(files)
        arr = (_L.dlsm_version_file * max(n, 1))()
        keep = []
        for j, f in enumerate(files):
            sm = np.frombuffer(bytes(f.smallest) + b"\0", dtype=np.uint8)
            lg = np.frombuffer(bytes(f.largest) + b"\0", dtype=np.uint8)
            keep += [sm, lg]
            if f.filter is None:
                fp, fl = None, 0
            elif on_device:
                fp, fl = _ptr(f.filter), int(f.filter.numel())
            else:
                fa = np.frombuffer(bytes(f.filter), dtype=np.uint8)
                keep.append(fa)
                fp, fl = fa.ctypes.data, fa.size
            arr[j] = _L.dlsm_version_file(sm.ctypes.data, len(f.smallest), lg.ctypes.data,
                                          len(f.largest), f.largest_trailer, f.number, f.level, 0,
                                          fp, fl)
        h = C.c_void_p()
        if sealed:
            status = np.zeros(max(n, 1), dtype=np.uint8)
            st = lib().dlsm_version_create_blocks(ctx.h, arr, n, 1 if on_device else 0,
                                                  1 if verify_checksums else 0, status.ctypes.data, C.byref(h))
            if st == _L.DLSM_E_CORRUPT:
                raise BlockError(st, "version_create_blocks", status[:n])
            check(st, "version_create_blocks")
        else:
            check(lib().dlsm_version_create(ctx.h, arr, n, 1 if on_device else 0, C.byref(h)),
                  "version_create")
        self.h = h
        self.n_files = n
        a, b = C.c_int(), C.c_int()
        check(lib().dlsm_version_slots(h, C.byref(a), C.byref(b)), "version_slots")
        self.n_l0, self.n_slots = a.value, b.value

    def close(self):
        if getattr(self, "h", None):
            lib().dlsm_version_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class ShardMap:
    """The upper bounds of a sharded database's shards resident on one device
    (DBImpl_Sharding's shards_pool keys, db/db_impl_sharding.cpp:9-35):
    ``bounds`` strictly ascending byte strings, 1..MAX_SHARDS of them."""

    def __init__(self, ctx: "Context", bounds: Sequence[bytes]):
        n = len(bounds)
        arrs = [np.frombuffer(bytes(b) + b"\0", dtype=np.uint8) for b in bounds]
        pa = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        la = (C.c_uint64 * max(n, 1))(*[len(b) for b in bounds])
        h = C.c_void_p()
        check(lib().dlsm_shardmap_create(ctx.h, pa, la, n, C.byref(h)), "shardmap_create")
        self.h = h
        self.n_shards = n

    def close(self):
        if getattr(self, "h", None):
            lib().dlsm_shardmap_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class TableIndex:
    """The index blocks of a version's tables resident on one device
    (dlsm_tableindex): ``blocks[f]`` is file f's sealed index block (bytes, or
    a device uint8 tensor with on_device) or None for a file whose index is
    not held.  A block that fails its checks raises BlockError with every
    file's BLOCK_* code."""

    def __init__(self, ctx: "Context", blocks, on_device: bool = False, *, verify_checksums: bool = True):
        n = len(blocks)
        if on_device:
            keep = list(blocks)
            ptrs = [None if b is None else _ptr(b) for b in keep]
            lens = [0 if b is None else int(b.numel()) for b in keep]
        else:
            keep = [None if b is None else np.frombuffer(bytes(b) + b"\0", dtype=np.uint8) for b in blocks]
            ptrs = [None if a is None else a.ctypes.data for a in keep]
            lens = [0 if a is None else a.size - 1 for a in keep]
        pa = (C.c_void_p * max(n, 1))(*ptrs)
        la = (C.c_uint64 * max(n, 1))(*lens)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        h = C.c_void_p()
        st = lib().dlsm_tableindex_create_blocks(ctx.h, pa, la, n, 1 if on_device else 0,
                                                 1 if verify_checksums else 0, status.ctypes.data, C.byref(h))
        self.h = h if st == _L.DLSM_OK else None
        if st == _L.DLSM_E_CORRUPT:
            assert h.value is None
            raise BlockError(st, "tableindex_create_blocks", status[:n])
        check(st, "tableindex_create_blocks")
        self.n_files = n
        self.block_status = status[:n]
        nf, ne, nb = C.c_int(), C.c_uint64(), C.c_uint64()
        check(lib().dlsm_tableindex_size(h, C.byref(nf), C.byref(ne), C.byref(nb)), "tableindex_size")
        self.n_entries, self.device_bytes = int(ne.value), int(nb.value)

    def close(self):
        if getattr(self, "h", None):
            lib().dlsm_tableindex_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class TableData:
    """The data regions of a version's tables on one device (dlsm_tabledata):
    ``files[f]`` is the list of file f's data chunks in offset order (bytes
    each, or device uint8 tensors with on_device, which are referenced in
    place and kept alive here), or None / an empty list for a file whose data
    is not held."""

    def __init__(self, ctx: "Context", files, on_device: bool = False):
        n = len(files)
        begin = np.zeros(n + 1, dtype=np.uint32)
        keep, recs = [], []
        for f, chunks in enumerate(files):
            for c in (chunks or []):
                if on_device:
                    keep.append(c)
                    recs.append(_L.dlsm_data_chunk(_ptr(c) if c.numel() else None, int(c.numel())))
                else:
                    a = np.frombuffer(bytes(c) + b"\0", dtype=np.uint8)
                    keep.append(a)
                    recs.append(_L.dlsm_data_chunk(a.ctypes.data, a.size - 1))
            begin[f + 1] = len(recs)
        ca = (_L.dlsm_data_chunk * max(len(recs), 1))(*recs)
        h = C.c_void_p()
        st = lib().dlsm_tabledata_create(ctx.h, ca, begin.ctypes.data_as(C.POINTER(C.c_uint32)), n,
                                         1 if on_device else 0, C.byref(h))
        self.h = h if st == _L.DLSM_OK else None
        check(st, "tabledata_create")
        self._keep = keep if on_device else None
        self.n_files = n
        nf, nc, nb = C.c_int(), C.c_uint64(), C.c_uint64()
        check(lib().dlsm_tabledata_size(h, C.byref(nf), C.byref(nc), C.byref(nb)), "tabledata_size")
        self.n_chunks, self.device_bytes = int(nc.value), int(nb.value)

    def close(self):
        if getattr(self, "h", None):
            lib().dlsm_tabledata_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class FilterSet:
    """F parsed full filters resident on one device (FullFilterBlockReader state)."""

    def __init__(self, ctx: "Context", filters, on_device: bool = False, *,
                 sealed: bool = False, verify_checksums: bool = True):
        """sealed: ``filters`` are sealed filter blocks (filter + 5-byte
        trailer), verified on the device; a bad block raises BlockError."""
        self.ctx = ctx
        F = len(filters)
        if on_device:
            ptrs = [_ptr(f) for f in filters]
            lens = [int(f.numel()) for f in filters]
            self._keep = list(filters)
        else:
            arrs = [np.frombuffer(bytes(f), dtype=np.uint8) for f in filters]
            ptrs = [a.ctypes.data for a in arrs]
            lens = [a.size for a in arrs]
            self._keep = arrs
        self.n_filters = F
        self.lens = [max(n - 5, 0) for n in lens] if sealed else lens  # the filters' own lengths
        h = C.c_void_p()
        pa = (C.c_void_p * F)(*ptrs)
        la = (C.c_uint64 * F)(*lens)
        if sealed:
            status = np.zeros(max(F, 1), dtype=np.uint8)
            st = lib().dlsm_filterset_create_blocks(ctx.h, pa, la, F, 1 if on_device else 0,
                                                    1 if verify_checksums else 0, status.ctypes.data, C.byref(h))
            if st == _L.DLSM_E_CORRUPT:
                raise BlockError(st, "filterset_create_blocks", status[:F])
            check(st, "filterset_create_blocks")
        else:
            check(lib().dlsm_filterset_create(ctx.h, pa, la, F, 1 if on_device else 0, C.byref(h)),
                  "filterset_create")
        self.h = h
        self._keep = None

    @property
    def mask_bytes(self) -> int:
        return (self.n_filters + 7) // 8

    def close(self):
        if getattr(self, "h", None):
            lib().dlsm_filterset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One device + one HIP stream + workspace (``dlsm_ctx``)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check(lib().dlsm_ctx_create(device, C.byref(h)), "ctx_create")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            lib().dlsm_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing -----------------------------------------------------------
    def sync(self):
        check(lib().dlsm_ctx_sync(self.h), "sync")

    def set_path(self, path: int):
        check(lib().dlsm_ctx_set_path(self.h, path), "set_path")

    def set_option(self, option: int, value: int):
        check(lib().dlsm_ctx_set_option(self.h, option, value), "set_option")

    def set_probe_round(self, keys: int):
        """Keys per pipelined probe round (0 = one round)."""
        self.set_option(OPT_PROBE_ROUND_KEYS, keys)

    def set_probe_serial(self, serial: bool):
        """Probe rounds one after another on this context's stream (DLSM_OPT_PROBE_ROUND_SERIAL)."""
        self.set_option(OPT_PROBE_ROUND_SERIAL, 1 if serial else 0)

    def set_build_groups(self, groups: int):
        """Job groups of a pipelined build (0 = auto, 1..4)."""
        self.set_option(OPT_BUILD_GROUPS, groups)

    def set_build_exact(self, mode: int):
        """0 auto, 1 count distinct hashes before bucketing, 2 never (DLSM_OPT_BUILD_EXACT)."""
        self.set_option(OPT_BUILD_EXACT, mode)

    def get_option(self, option: int) -> int:
        v = C.c_uint64()
        check(lib().dlsm_ctx_get_option(self.h, option, C.byref(v)), "get_option")
        return int(v.value)

    def set_probe_shape(self, chunk_lg: int, slice_lg: int):
        """Sliced probe shape: 2^chunk_lg keys per partition chunk (12..14),
        2^slice_lg stacked lines per LDS slice (7 = 64 KiB, 8 = 128 KiB)."""
        self.set_option(OPT_PROBE_CHUNK_LG, chunk_lg)
        self.set_option(OPT_PROBE_SLICE_LG, slice_lg)

    def set_stream(self, stream=None):
        """Run on a torch.cuda.Stream (or its raw handle); None = own stream."""
        raw = None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
        check(lib().dlsm_ctx_set_stream(self.h, raw), "set_stream")

    def set_partition_stream(self, stream=None, cus: int = 0):
        """Partition passes on `stream` (a CU-masked stream: cu_mask_stream),
        slice / unpermute passes on the context stream; None = one stream."""
        raw = None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
        check(lib().dlsm_ctx_set_partition_stream(self.h, raw, cus if raw else 0), "set_partition_stream")

    @property
    def stream_handle(self) -> int:
        return int(lib().dlsm_ctx_stream(self.h) or 0)

    def reserve(self, max_keys: int, max_jobs: int):
        check(lib().dlsm_ctx_reserve(self.h, max_keys, max_jobs), "reserve")

    def stats(self):
        """(device allocations made so far, workspace bytes held)."""
        n, b = C.c_uint64(), C.c_uint64()
        check(lib().dlsm_ctx_stats(self.h, C.byref(n), C.byref(b)), "stats")
        return int(n.value), int(b.value)

    # -- full filter build --------------------------------------------------
    @staticmethod
    def _jobs(tables: Sequence[Keys], outs, caps):
        n = len(tables)
        arr = (dlsm_build_job * max(n, 1))()
        for j, t in enumerate(tables):
            arr[j].keys = t.c()
            arr[j].out = _ptr(outs[j])
            arr[j].out_cap = caps[j]
        return arr

    def full_build(self, tables: Sequence[Keys], bits_per_key: int = 10, caps=None) -> list:
        """Host keys -> host filter bytes (synchronous).  One filter per table."""
        n = len(tables)
        if caps is None:
            caps = [full_size(t.n, bits_per_key)[0] for t in tables]
        outs = [np.zeros(max(c, 1), dtype=np.uint8) for c in caps]
        jobs = self._jobs(tables, outs, caps)
        lens = (C.c_uint64 * max(n, 1))()
        check(lib().dlsm_bloom_full_build(self.h, jobs, n, bits_per_key, lens), "full_build")
        return [outs[j][: lens[j]].tobytes() for j in range(n)]

    def full_build_dev(self, tables: Sequence[Keys], outs, out_lens, bits_per_key: int = 10):
        """Device keys (torch tensors) -> device slots; asynchronous on this ctx's stream."""
        _need(out_lens, 8 * len(tables), "full_build_dev out_lens")
        caps = [int(o.numel()) for o in outs]
        jobs = self._jobs(tables, outs, caps)
        check(lib().dlsm_bloom_full_build_dev(self.h, jobs, len(tables), bits_per_key,
                                              _ptr(out_lens)), "full_build_dev")

    def bind_full_build_dev(self, tables: Sequence[Keys], outs, out_lens, bits_per_key: int = 10):
        """full_build_dev with its arguments marshalled once: returns a
        zero-argument callable (one ctypes call per invocation; the GIL is
        released inside it), for per-step loops on several host threads."""
        _need(out_lens, 8 * len(tables), "bind_full_build_dev out_lens")
        caps = [int(o.numel()) for o in outs]
        jobs = self._jobs(tables, outs, caps)
        fn, h, n, lp = lib().dlsm_bloom_full_build_dev, self.h, len(tables), _ptr(out_lens)
        keep = (jobs, list(tables), list(outs), out_lens)

        def call():
            st = fn(h, jobs, n, bits_per_key, lp)
            if st:
                check(st, "full_build_dev")

        call.keep = keep
        return call

    def full_build_hashed(self, hash_sets, bits_per_key: int = 10, caps=None) -> list:
        """Filters from BloomHash values (numpy uint32 arrays, AddKey order;
        consecutive equal hashes are dropped like AddKey) -- host in/out."""
        sets = [np.ascontiguousarray(h, dtype=np.uint32) for h in hash_sets]
        tables = [Keys(h if h.size else np.zeros(1, dtype=np.uint32), h.size, 4) for h in sets]
        if caps is None:
            caps = [full_size(h.size, bits_per_key)[0] for h in sets]
        outs = [np.zeros(max(c, 1), dtype=np.uint8) for c in caps]
        jobs = self._jobs(tables, outs, caps)
        n = len(tables)
        lens = (C.c_uint64 * max(n, 1))()
        check(lib().dlsm_bloom_full_build_hashed(self.h, jobs, n, bits_per_key, lens), "full_build_hashed")
        return [outs[j][: lens[j]].tobytes() for j in range(n)]

    def full_build_hashed_dev(self, hash_sets, outs, out_lens, bits_per_key: int = 10):
        """Device form: hash_sets are device uint32 tensors."""
        _need(out_lens, 8 * len(hash_sets), "full_build_hashed_dev out_lens")
        tables = [Keys(h, int(h.numel()), 4) for h in hash_sets]
        caps = [int(o.numel()) for o in outs]
        jobs = self._jobs(tables, outs, caps)
        check(lib().dlsm_bloom_full_build_hashed_dev(self.h, jobs, len(tables), bits_per_key, _ptr(out_lens)),
              "full_build_hashed_dev")

    def full_build_block(self, tables: Sequence[Keys], bits_per_key: int = 10, caps=None) -> list:
        """Filter + 5-byte block trailer (FinishFilterBlock), host in/out."""
        n = len(tables)
        if caps is None:
            caps = [full_size(t.n, bits_per_key)[0] + 5 for t in tables]
        outs = [np.zeros(max(c, 1), dtype=np.uint8) for c in caps]
        jobs = self._jobs(tables, outs, caps)
        lens = (C.c_uint64 * max(n, 1))()
        check(lib().dlsm_bloom_full_build_block(self.h, jobs, n, bits_per_key, lens), "full_build_block")
        return [outs[j][: lens[j]].tobytes() for j in range(n)]

    def full_build_block_dev(self, tables: Sequence[Keys], outs, out_lens, bits_per_key: int = 10):
        caps = [int(o.numel()) for o in outs]
        jobs = self._jobs(tables, outs, caps)
        check(lib().dlsm_bloom_full_build_block_dev(self.h, jobs, len(tables), bits_per_key,
                                                    _ptr(out_lens)), "full_build_block_dev")

    def full_build_block_hashed(self, hash_sets, bits_per_key: int = 10, caps=None) -> list:
        """Sealed filter blocks from BloomHash values (numpy uint32 arrays,
        AddKey order) -- host in/out."""
        sets = [np.ascontiguousarray(h, dtype=np.uint32) for h in hash_sets]
        tables = [Keys(h if h.size else np.zeros(1, dtype=np.uint32), h.size, 4) for h in sets]
        if caps is None:
            caps = [full_size(h.size, bits_per_key)[0] + 5 for h in sets]
        outs = [np.zeros(max(c, 1), dtype=np.uint8) for c in caps]
        jobs = self._jobs(tables, outs, caps)
        n = len(tables)
        lens = (C.c_uint64 * max(n, 1))()
        check(lib().dlsm_bloom_full_build_block_hashed(self.h, jobs, n, bits_per_key, lens),
              "full_build_block_hashed")
        return [outs[j][: lens[j]].tobytes() for j in range(n)]

    def full_build_block_hashed_dev(self, hash_sets, outs, out_lens, bits_per_key: int = 10):
        """Device form: hash_sets are device uint32 tensors, outs device slots."""
        _need(out_lens, 8 * len(hash_sets), "full_build_block_hashed_dev out_lens")
        tables = [Keys(h, int(h.numel()), 4) for h in hash_sets]
        caps = [int(o.numel()) for o in outs]
        jobs = self._jobs(tables, outs, caps)
        check(lib().dlsm_bloom_full_build_block_hashed_dev(self.h, jobs, len(tables), bits_per_key,
                                                           _ptr(out_lens)), "full_build_block_hashed_dev")

    def blocks_check(self, blocks, on_device: bool = False, verify_checksums: bool = True) -> np.ndarray:
        """ReadFilterBlock's trailer checks of sealed blocks of any contents
        (bytes, or device uint8 tensors with on_device): uint8[n] of
        BLOCK_OK / BLOCK_SHORT / BLOCK_CHECKSUM / BLOCK_TYPE."""
        n = len(blocks)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        if on_device:
            keep = list(blocks)
            ptrs = [_ptr(b) if int(b.numel()) else None for b in keep]
            lens = [int(b.numel()) for b in keep]
        else:
            keep = [np.frombuffer(bytes(b) + b"\0", dtype=np.uint8) for b in blocks]
            ptrs = [a.ctypes.data for a in keep]
            lens = [a.size - 1 for a in keep]
        pa = (C.c_void_p * max(n, 1))(*ptrs)
        la = (C.c_uint64 * max(n, 1))(*lens)
        st = lib().dlsm_blocks_check(self.h, pa, la, n, 1 if on_device else 0, 1 if verify_checksums else 0,
                                     status.ctypes.data)
        if st != _L.DLSM_E_CORRUPT:
            check(st, "blocks_check")
        return status[:n]

    def block_open_stats(self):
        """(bytes read, bytes written, milliseconds between the events around
        the two launches) of this context's last block check / open."""
        r, w, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        check(lib().dlsm_block_open_stats(self.h, C.byref(r), C.byref(w), C.byref(ms)), "block_open_stats")
        return int(r.value), int(w.value), float(ms.value)

    def crc32c_dev(self, bufs) -> list:
        """crc32c::Value of device tensors (uint8), computed on the GPU."""
        n = len(bufs)
        ptrs = (C.c_void_p * max(n, 1))(*[_ptr(b) for b in bufs])
        lens = (C.c_uint64 * max(n, 1))(*[int(b.numel()) for b in bufs])
        out = (C.c_uint32 * max(n, 1))()
        check(lib().dlsm_crc32c_dev(self.h, ptrs, lens, n, out), "crc32c_dev")
        return [int(out[j]) for j in range(n)]

    # -- internal keys: flush / compaction selection, user-key gather --------
    def internal_keys_select_dev(self, keys: Keys, policy: int, smallest_snapshot: int, keep):
        """keep (device uint8[n]) <- 1 for every key the flush / compaction loop
        passes to TableBuilder::Add.  Returns (n_kept, kept_user_key_bytes,
        first_corrupt or None).  A flush over a corrupt key raises DlsmError
        (DLSM_E_CORRUPT) like the reference's IOError."""
        ks = keys.c()
        nk, nb, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
        st = lib().dlsm_internal_keys_select_dev(self.h, C.byref(ks), policy, smallest_snapshot,
                                                 _ptr(keep), C.byref(nk), C.byref(nb), C.byref(bad))
        check(st, "internal_keys_select_dev")
        return int(nk.value), int(nb.value), (None if bad.value == 2**64 - 1 else int(bad.value))

    def user_keys_gather_dev(self, keys: Keys, keep, out, offsets=None):
        """Pack ExtractUserKey(key) of the kept keys into `out` (device uint8);
        variable-length keys also fill `offsets` (device uint64[n_kept+1])."""
        ks = keys.c()
        check(lib().dlsm_user_keys_gather_dev(self.h, C.byref(ks), _ptr(keep), _ptr(out), _ptr(offsets)),
              "user_keys_gather_dev")

    # -- legacy block-based filter block (table/filter_block.cc) -------------
    def filter_block_build_dev(self, keys: Keys, block_key_end, block_end_offset,
                               bits_per_key: int = 10, out=None):
        """FilterBlockBuilder over a table's keys (data block b ends at key
        block_key_end[b], then StartBlock(block_end_offset[b])).  Returns the
        block as a device uint8 tensor (or fills `out` and returns its length)."""
        import torch

        ke = np.ascontiguousarray(block_key_end, dtype=np.uint64)
        eo = np.ascontiguousarray(block_end_offset, dtype=np.uint64)
        nb = C.c_uint64()
        check(lib().dlsm_filter_block_size(_ptr(ke), _ptr(eo), len(ke), keys.n,
                                           bits_per_key, C.byref(nb)), "filter_block_size")
        ret = out is None
        if out is None:
            out = torch.empty(nb.value, dtype=torch.uint8, device=f"cuda:{self.device}")
        ln = C.c_uint64()
        ks = keys.c()
        check(lib().dlsm_filter_block_build_dev(self.h, C.byref(ks), _ptr(ke), _ptr(eo),
                                                len(ke), bits_per_key, _ptr(out), int(out.numel()),
                                                C.byref(ln)), "filter_block_build_dev")
        return out[: ln.value] if ret else ln.value

    def filter_block_probe_dev(self, block, keys: Keys, block_offsets, out):
        """FilterBlockReader::KeyMayMatch(block_offsets[i], key i) -> out[i] (device)."""
        ks = keys.c()
        check(lib().dlsm_filter_block_probe_dev(self.h, _ptr(block), int(block.numel()), C.byref(ks),
                                                _ptr(block_offsets), _ptr(out)), "filter_block_probe_dev")

    # -- MultiGet-style probe of a version -------------------------------------
    def version(self, files: Sequence[VersionFile], on_device: bool = False, *, sealed: bool = False,
                verify_checksums: bool = True) -> Version:
        return Version(self, files, on_device, sealed=sealed, verify_checksums=verify_checksums)

    def version_probe_dev(self, v: Version, keys: Keys, snapshot: int, slot_mask, level_file=None):
        """slot_mask (device uint64[n]): bit s = search slot s is a file Version::Get
        visits and whose filter passes the key; level_file (device int32/uint32
        [n, 5], optional): per level the candidate file's index in the level."""
        ks = keys.c()
        check(lib().dlsm_version_probe_dev(self.h, v.h, C.byref(ks), snapshot, _ptr(slot_mask),
                                           _ptr(level_file)), "version_probe_dev")

    def version_read_plan_dev(self, v: Version, slot_mask, level_file, mode: int, file_begin, gets,
                              dropped=None, *, n: Optional[int] = None, cap: Optional[int] = None):
        """The probe's answers grouped by file (compressed sparse rows): gets
        (device uint32[cap]) holds, for file f of the caller's ``files`` list, the
        Gets that must read it at [file_begin[f], file_begin[f+1]), ascending;
        file_begin (device uint64[n_files + 1]) is exact even when cap is too
        small.  mode: PLAN_FIRST (each Get's lowest set slot) or PLAN_ALL;
        dropped (device uint64[1], optional) counts malformed tasks.
        Asynchronous; n defaults to slot_mask's length, cap to gets' length."""
        n = int(slot_mask.numel()) if n is None else int(n)
        cap = (0 if gets is None else int(gets.numel())) if cap is None else int(cap)
        _need(slot_mask, 8 * n, "slot_mask")
        if level_file is not None:
            _need(level_file, 20 * n, "level_file")
        _need(file_begin, 8 * (v.n_files + 1), "file_begin")
        _need(gets, 4 * cap, "gets")
        if dropped is not None:
            _need(dropped, 8, "dropped")
        check(lib().dlsm_version_read_plan_dev(self.h, v.h, _ptr(slot_mask), _ptr(level_file), n, mode,
                                               _ptr(file_begin), _ptr(gets), cap, _ptr(dropped)),
              "version_read_plan_dev")

    def version_masks_advance_dev(self, slot_mask, hit, *, n: Optional[int] = None):
        """Ends a read round: slot_mask[i] = 0 where hit[i] (device uint8[n]) is
        non-zero, else slot_mask[i] without its lowest set bit.  Asynchronous."""
        n = int(slot_mask.numel()) if n is None else int(n)
        _need(slot_mask, 8 * n, "slot_mask")
        _need(hit, n, "hit")
        check(lib().dlsm_version_masks_advance_dev(self.h, _ptr(slot_mask), _ptr(hit), n),
              "version_masks_advance_dev")

    # -- shard route: the first step of a sharded Get ---------------------------
    def shardmap(self, bounds: Sequence[bytes]) -> ShardMap:
        return ShardMap(self, bounds)

    def shard_route_dev(self, m: ShardMap, keys: Keys, shard_off, shard_cnt, gets, keys_out=None, *,
                        cap: Optional[int] = None):
        """Get_Target_Shard for a device Get batch: bin s (shard s, or
        n_shards = "no shard") owns gets[shard_off[s] : shard_off[s] +
        shard_cnt[s]] (device uint32[cap]), the bin's Get indices ascending;
        shard_off / shard_cnt are device uint64[n_shards + 1], every offset a
        multiple of ROUTE_ALIGN.  keys_out (device uint8[cap * key_len],
        fixed-length keys only): key gets[p] copied to row p.  Asynchronous;
        cap defaults to gets' length and must be >= shard_route_cap(n, n_shards)."""
        cap = (0 if gets is None else int(gets.numel())) if cap is None else int(cap)
        _need(shard_off, 8 * (m.n_shards + 1), "shard_off")
        _need(shard_cnt, 8 * (m.n_shards + 1), "shard_cnt")
        _need(gets, 4 * cap, "gets")
        if keys_out is not None:
            _need(keys_out, cap * keys.key_len, "keys_out")
        ks = keys.c()
        check(lib().dlsm_shard_route_dev(self.h, m.h, C.byref(ks), _ptr(shard_off), _ptr(shard_cnt), _ptr(gets),
                                         _ptr(keys_out), cap), "shard_route_dev")

    # -- table index: the index step of Table::InternalGet ----------------------
    def tableindex(self, blocks, on_device: bool = False, *, verify_checksums: bool = True) -> TableIndex:
        return TableIndex(self, blocks, on_device, verify_checksums=verify_checksums)

    def index_seek_dev(self, ti: TableIndex, keys: Keys, snapshot: int, file_begin, gets, *, cap: Optional[int] = None,
                       task_state=None, task_handle=None, get_state=None, get_handle=None):
        """Seek every task of a read plan (file_begin, gets: the plan's device
        outputs) in its file's index block.  task_state (device uint8[cap]) /
        task_handle (device, 16 bytes per task: KV_HANDLE) are written per
        task; get_state (device uint8[n]) / get_handle (16 bytes per Get) only
        where a task's state is not GET_NOTFOUND -- zero-fill them before the
        first round of a PLAN_FIRST loop; get_state is then the ``hit`` of
        version_masks_advance_dev.  Asynchronous; cap defaults to gets' length."""
        cap = (0 if gets is None else int(gets.numel())) if cap is None else int(cap)
        _need(file_begin, 8 * (ti.n_files + 1), "file_begin")
        _need(gets, 4 * cap, "gets")
        for x, per, what in ((task_state, 1, "task_state"), (task_handle, 16, "task_handle")):
            if x is not None:
                _need(x, per * cap, what)
        for x, per, what in ((get_state, 1, "get_state"), (get_handle, 16, "get_handle")):
            if x is not None:
                _need(x, per * keys.n, what)
        ks = keys.c()
        check(lib().dlsm_index_seek_dev(self.h, ti.h, C.byref(ks), snapshot, _ptr(file_begin), _ptr(gets), cap,
                                        _ptr(task_state), _ptr(task_handle), _ptr(get_state), _ptr(get_handle)),
              "index_seek_dev")

    # -- value read: the tail of Table::InternalGet ------------------------------
    def tabledata(self, files, on_device: bool = False) -> TableData:
        return TableData(self, files, on_device)

    def kv_read_dev(self, td: TableData, keys: Keys, state, handle, value_off, values, *, gets=None, count=None,
                    cap: Optional[int] = None, values_cap: Optional[int] = None, n_corrupt=None):
        """Read the values of a seeked batch: state (device uint8[cap], updated
        in place) and handle (device, 16 bytes per item: KV_HANDLE) are the
        seek's per-Get arrays, or its per-task arrays with gets (device
        uint32[cap]: each item's key index) and count (a device uint64: the
        item count, e.g. file_begin[n_files:]).  value_off (device uint64[cap +
        1]) gets the values' exclusive byte offsets and the total, values
        (device uint8, 16-byte aligned) the bytes below min(total, values_cap);
        n_corrupt (device uint64[1]) the items set to GET_CORRUPT.
        Asynchronous; cap defaults to state's length, values_cap to values'."""
        cap = (0 if state is None else int(state.numel())) if cap is None else int(cap)
        values_cap = _nbytes(values) if values_cap is None else int(values_cap)
        _need(state, cap, "state")
        _need(handle, 16 * cap, "handle")
        _need(value_off, 8 * (cap + 1) if cap else 0, "value_off")
        _need(values, values_cap, "values")
        for x, nb, what in ((gets, 4 * cap, "gets"), (count, 8, "count"), (n_corrupt, 8, "n_corrupt")):
            if x is not None:
                _need(x, nb, what)
        ks = keys.c()
        check(lib().dlsm_kv_read_dev(self.h, td.h, C.byref(ks), _ptr(gets), _ptr(count), cap, _ptr(state), _ptr(handle),
                                     _ptr(value_off), _ptr(values), values_cap, _ptr(n_corrupt)), "kv_read_dev")

    def kv_read_stats(self):
        """(size, offsets, copy) device milliseconds of the last kv_read_dev
        (call after sync) and the copy's grid in workgroups."""
        ms, wgs = (C.c_double * 3)(), C.c_uint32()
        check(lib().dlsm_kv_read_stats(self.h, ms, C.byref(wgs)), "kv_read_stats")
        return (float(ms[0]), float(ms[1]), float(ms[2])), int(wgs.value)

    def kv_read(self, td: TableData, keys: Keys, state: np.ndarray, handle: np.ndarray, *, gets=None,
                count: Optional[int] = None, values_cap: int = 0):
        """The host-memory form: state (uint8[cap], updated in place), handle
        (KV_HANDLE[cap]).  Returns (value_off uint64[m + 1], values uint8,
        n_corrupt)."""
        if not isinstance(state, np.ndarray) or state.dtype != np.uint8 or not state.flags.c_contiguous:
            raise ValueError("state: a contiguous numpy uint8 array is needed")
        cap = int(state.size)
        if not isinstance(handle, np.ndarray) or handle.dtype.itemsize != 16 or not handle.flags.c_contiguous:
            raise ValueError("handle: a contiguous numpy array of 16-byte records (KV_HANDLE) is needed")
        _need(handle, 16 * cap, "handle")
        if gets is not None:
            if not isinstance(gets, np.ndarray) or gets.dtype != np.uint32 or not gets.flags.c_contiguous:
                raise ValueError("gets: a contiguous numpy uint32 array is needed")
            _need(gets, 4 * cap, "gets")
        m = cap if count is None else min(int(count), cap)
        cnt = None if count is None else np.array([count], dtype=np.uint64)
        value_off = np.zeros(cap + 1, dtype=np.uint64)
        values = np.zeros(max(values_cap, 1), dtype=np.uint8)
        bad = np.zeros(1, dtype=np.uint64)
        ks = keys.c()
        check(lib().dlsm_kv_read(self.h, td.h, C.byref(ks), _ptr(gets), _ptr(cnt), cap, _ptr(state), _ptr(handle),
                                 _ptr(value_off), _ptr(values), values_cap, _ptr(bad)), "kv_read")
        return value_off[:m + 1], values[:min(int(value_off[m]), values_cap)], int(bad[0])

    # -- table build: the data region and the sealed index block ----------------
    def table_build_dev(self, keys: Keys, values, data, index, chunk_end, built, *, value_off=None, value_len: int = 0,
                        chunk_bytes: int = 0, data_cap: Optional[int] = None, index_cap: Optional[int] = None,
                        chunk_cap: Optional[int] = None):
        """Build a table's data region and sealed index block on the device:
        ``keys`` are the internal keys in table order, ``values`` the packed
        values with ``value_off`` (device uint64[n + 1]) or one ``value_len``.
        data / index (device uint8, 16-byte aligned), chunk_end (device uint64)
        and built (device uint64[4]: data_bytes, index_bytes, n_chunks, flags)
        are written; the caps default to the buffers' lengths.  Asynchronous."""
        ti, to = _table_io(keys, values, value_off, value_len, chunk_bytes, data, data_cap, index, index_cap,
                           chunk_end, chunk_cap, built)
        check(lib().dlsm_table_build_dev(self.h, C.byref(ti), C.byref(to)), "table_build_dev")

    def table_build(self, keys: Keys, values, **kw):
        """The host-memory form (see dlsm_amd.table_build)."""
        return table_build(keys, values, ctx=self, **kw)

    def table_build_stats(self):
        """(size, offsets, region, index, seal) device milliseconds of the last
        table_build_dev (call after sync) and the writes' grid in workgroups."""
        ms, wgs = (C.c_double * 5)(), C.c_uint32()
        check(lib().dlsm_table_build_stats(self.h, ms, C.byref(wgs)), "table_build_stats")
        return tuple(float(x) for x in ms), int(wgs.value)

    # -- compaction merge: sorted runs into one run ------------------------------
    def compaction_merge_dev(self, runs, keys, key_off, values, value_off, merged, *, src=None,
                             policy: int = MERGE_DROP_HIDDEN, smallest_snapshot: int = 0,
                             keys_cap: Optional[int] = None, values_cap: Optional[int] = None,
                             pair_cap: Optional[int] = None):
        """Merge sorted runs on the device: ``runs`` is a list of (Keys, values,
        value_off or None, value_len) over device tensors.  keys / values
        (device uint8, 16-byte aligned) get the kept internal keys / values
        back to back, key_off / value_off (device uint64[pair_cap + 1]) their
        offsets, src (device uint64[pair_cap], optional) run << 32 | index per
        output pair, merged (device uint64[5]) n_in, n_out, key_bytes,
        value_bytes, flags.  The output is the table build's input form.  The
        caps default to the buffers' lengths.  Asynchronous."""
        mr, mo = _merge_io(runs, keys, keys_cap, key_off, values, values_cap, value_off, src, pair_cap, merged)
        check(lib().dlsm_compaction_merge_dev(self.h, mr, len(runs), policy, smallest_snapshot, C.byref(mo)),
              "compaction_merge_dev")

    # -- memtable sort: an unsorted batch into a sorted run --------------------------
    def memtable_sort_dev(self, batch, keys, key_off, values, value_off, merged, *, src=None,
                          policy: int = MERGE_DROP_HIDDEN, smallest_snapshot: int = 0,
                          keys_cap: Optional[int] = None, values_cap: Optional[int] = None,
                          pair_cap: Optional[int] = None):
        """Sort one batch of pairs in arrival order on the device: ``batch`` is
        one (Keys, values, value_off or None, value_len) over device tensors.
        The outputs are compaction_merge_dev's -- the table build's input form
        -- with src the input index of each output pair.  Asynchronous;
        compaction_merge_stats reports it."""
        mr, mo = _merge_io([batch], keys, keys_cap, key_off, values, values_cap, value_off, src, pair_cap, merged)
        check(lib().dlsm_memtable_sort_dev(self.h, mr, policy, smallest_snapshot, C.byref(mo)), "memtable_sort_dev")

    def memtable_sort(self, batch, policy: int = MERGE_DROP_HIDDEN, smallest_snapshot: int = 0, **kw):
        """The host-memory form (see dlsm_amd.memtable_sort)."""
        return memtable_sort(batch, policy, smallest_snapshot, ctx=self, **kw)

    # -- compaction output: a merged run cut into size-capped tables ---------------
    def compaction_output_dev(self, keys: Keys, values, merged, data, index, chunk_end, files, built, *, value_off=None,
                              value_len: int = 0, max_file_bytes: int = 0, chunk_bytes: int = 0,
                              data_cap: Optional[int] = None, index_cap: Optional[int] = None,
                              chunk_cap: Optional[int] = None, file_cap: Optional[int] = None):
        """Write every output table of a compaction on the device: ``keys``
        (keys.n the pair capacity), ``values`` / ``value_off`` and ``merged``
        (device uint64[5], read on the device) are what compaction_merge_dev
        left.  data / index (device uint8, 16-byte aligned), chunk_end (device
        uint64), files (device uint64[file_cap * 9], OUTPUT_FILE_FIELDS) and
        built (device uint64[5]: n_files, data_bytes, index_bytes, n_chunks,
        flags) are written; the caps default to the buffers' lengths.
        Asynchronous, no host read-back."""
        oi, oo = _output_io(keys, values, value_off, value_len, merged, max_file_bytes, chunk_bytes, data, data_cap,
                            index, index_cap, chunk_end, chunk_cap, files, file_cap, built)
        check(lib().dlsm_compaction_output_dev(self.h, C.byref(oi), C.byref(oo)), "compaction_output_dev")

    def compaction_output(self, keys: Keys, values, merged, **kw):
        """The host-memory form (see dlsm_amd.compaction_output)."""
        return compaction_output(keys, values, merged, ctx=self, **kw)

    def compaction_output_stats(self):
        """(size, offsets, cut, entries, region, index, seal) device
        milliseconds of the last compaction_output_dev (call after sync) and
        the writes' grid in workgroups."""
        ms, wgs = (C.c_double * 7)(), C.c_uint32()
        check(lib().dlsm_compaction_output_stats(self.h, ms, C.byref(wgs)), "compaction_output_stats")
        return tuple(float(x) for x in ms), int(wgs.value)

    # -- compaction filters: the sealed filter block of every output file ------------
    def compaction_filters_dev(self, keys: Keys, merged, files, out_built, filters, recs, built, *, bits_per_key: int = 10,
                               file_cap: Optional[int] = None, filters_cap: Optional[int] = None):
        """Write the sealed filter block of every file compaction_output_dev
        cut out of the run: ``keys`` (keys.n the pair capacity) and ``merged``
        as that call took them, ``files`` and ``out_built`` the records and
        totals it wrote -- all device memory, read on the device.  filters
        (device uint8, 16-byte aligned), recs (device uint64[file_cap * 4],
        FILTER_REC_FIELDS) and built (device uint64[3]: n_files, filter_bytes,
        flags) are written; the caps default to the buffers' lengths.
        Asynchronous, no host read-back."""
        fi, fo = _filters_io(keys, merged, files, out_built, file_cap, bits_per_key, filters, filters_cap, recs, built)
        check(lib().dlsm_compaction_filters_dev(self.h, C.byref(fi), C.byref(fo)), "compaction_filters_dev")

    def compaction_filters(self, keys: Keys, merged, files, out_built, **kw):
        """The host-memory form (see dlsm_amd.compaction_filters)."""
        return compaction_filters(keys, merged, files, out_built, ctx=self, **kw)

    def compaction_filters_stats(self):
        """(hash, plan, partition, slice, finish) device milliseconds of the
        last compaction_filters_dev (call after sync), its lgR (2^lgR lines per
        slice) and the slice launch's grid in workgroups."""
        ms, lg, wgs = (C.c_double * 5)(), C.c_int(), C.c_uint32()
        check(lib().dlsm_compaction_filters_stats(self.h, ms, C.byref(lg), C.byref(wgs)), "compaction_filters_stats")
        return tuple(float(x) for x in ms), int(lg.value), int(wgs.value)

    def compaction_merge(self, runs, policy: int = MERGE_DROP_HIDDEN, smallest_snapshot: int = 0, **kw):
        """The host-memory form (see dlsm_amd.compaction_merge)."""
        return compaction_merge(runs, policy, smallest_snapshot, ctx=self, **kw)

    def compaction_merge_tables_dev(self, ti: "TableIndex", td: "TableData", runs, keys, key_off, values, value_off,
                                    merged, *, src=None, policy: int = MERGE_DROP_HIDDEN, smallest_snapshot: int = 0,
                                    keys_cap: Optional[int] = None, values_cap: Optional[int] = None,
                                    pair_cap: Optional[int] = None):
        """compaction_merge_dev with its inputs read straight out of the opened
        tables ``ti`` / ``td``: ``runs`` is a list of file-number lists, a
        level-0 file each or a deeper level's files in key order; a run's pairs
        are its files' entries in the order listed.  The outputs are
        compaction_merge_dev's, src counting through each run's concatenated
        files.  Asynchronous."""
        tr, _keep = _table_runs(runs)
        mo = _merge_out(keys, keys_cap, key_off, values, values_cap, value_off, src, pair_cap, merged)
        check(lib().dlsm_compaction_merge_tables_dev(self.h, ti.h, td.h, tr, len(runs), policy, smallest_snapshot,
                                                     C.byref(mo)), "compaction_merge_tables_dev")

    def compaction_merge_tables(self, blocks, files, runs, policy: int = MERGE_DROP_HIDDEN, smallest_snapshot: int = 0,
                                **kw):
        """The host-memory form (see dlsm_amd.compaction_merge_tables)."""
        return compaction_merge_tables(blocks, files, runs, policy, smallest_snapshot, ctx=self, **kw)

    def range_scan(self, blocks, files, runs, starts: Keys, snapshot: int, limit: int, **kw):
        """The host-memory form (see dlsm_amd.range_scan)."""
        return range_scan(blocks, files, runs, starts, snapshot, limit, ctx=self, **kw)

    def compaction_merge_stats(self):
        """(record, partition, merge, decide, offsets, gather) device
        milliseconds of the last compaction_merge_dev,
        compaction_merge_tables_dev or memtable_sort_dev (the tile sort in the
        record slot; call after sync) and its number of merge
        passes."""
        ms, passes = (C.c_double * 6)(), C.c_uint32()
        check(lib().dlsm_compaction_merge_stats(self.h, ms, C.byref(passes)), "compaction_merge_stats")
        return tuple(float(x) for x in ms), int(passes.value)

    # -- full filter probe --------------------------------------------------
    def filterset(self, filters, on_device: bool = False, *, sealed: bool = False,
                  verify_checksums: bool = True) -> FilterSet:
        return FilterSet(self, filters, on_device, sealed=sealed, verify_checksums=verify_checksums)

    def full_probe(self, fs: FilterSet, keys: Keys) -> np.ndarray:
        mask = np.zeros(max(keys.n * fs.mask_bytes, 1), dtype=np.uint8)
        ks = keys.c()
        check(lib().dlsm_bloom_full_probe(self.h, fs.h, C.byref(ks), mask.ctypes.data), "full_probe")
        return mask[: keys.n * fs.mask_bytes]

    def full_probe_hashed_dev(self, fs: FilterSet, hashes, mask, n: Optional[int] = None):
        """Probe from BloomHash values (device uint32 tensor); asynchronous."""
        n = int(hashes.numel()) if n is None else n
        _need(mask, n * fs.mask_bytes, "full_probe_hashed_dev mask")
        ks = Keys(hashes, n, 4).c()
        check(lib().dlsm_bloom_full_probe_hashed_dev(self.h, fs.h, C.byref(ks), _ptr(mask)),
              "full_probe_hashed_dev")

    def full_probe_dev(self, fs: FilterSet, keys: Keys, mask):
        _need(mask, keys.n * fs.mask_bytes, "full_probe_dev mask")
        ks = keys.c()
        check(lib().dlsm_bloom_full_probe_dev(self.h, fs.h, C.byref(ks), _ptr(mask)),
              "full_probe_dev")

    def bind_full_probe_dev(self, fs: FilterSet, keys: Keys, mask):
        """full_probe_dev with its arguments marshalled once (see bind_full_build_dev)."""
        _need(mask, keys.n * fs.mask_bytes, "bind_full_probe_dev mask")
        ks = keys.c()
        fn, h, fh, kp, mp = lib().dlsm_bloom_full_probe_dev, self.h, fs.h, C.byref(ks), _ptr(mask)
        keep = (ks, fs, keys, mask)

        def call():
            st = fn(h, fh, kp, mp)
            if st:
                check(st, "full_probe_dev")

        call.keep = keep
        return call

    # -- legacy FilterPolicy format -----------------------------------------
    def legacy_build(self, tables: Sequence[Keys], bits_per_key: int = 10) -> list:
        n = len(tables)
        caps = [legacy_size(t.n, bits_per_key) for t in tables]
        outs = [np.zeros(c, dtype=np.uint8) for c in caps]
        jobs = self._jobs(tables, outs, caps)
        lens = (C.c_uint64 * max(n, 1))()
        check(lib().dlsm_bloom_legacy_build(self.h, jobs, n, bits_per_key, lens), "legacy_build")
        return [outs[j][: lens[j]].tobytes() for j in range(n)]

    def legacy_build_dev(self, tables: Sequence[Keys], outs, out_lens, bits_per_key: int = 10):
        _need(out_lens, 8 * len(tables), "legacy_build_dev out_lens")
        caps = [int(o.numel()) for o in outs]
        jobs = self._jobs(tables, outs, caps)
        check(lib().dlsm_bloom_legacy_build_dev(self.h, jobs, len(tables), bits_per_key,
                                                _ptr(out_lens)), "legacy_build_dev")

    def legacy_probe(self, filt: bytes, keys: Keys) -> np.ndarray:
        fa = np.frombuffer(bytes(filt) + b"\0", dtype=np.uint8)
        out = np.zeros(max(keys.n, 1), dtype=np.uint8)
        ks = keys.c()
        check(lib().dlsm_bloom_legacy_probe(self.h, fa.ctypes.data if len(filt) else None, len(filt),
                                            C.byref(ks), out.ctypes.data), "legacy_probe")
        return out[: keys.n]

    def legacy_probe_dev(self, filt_dev, length: int, keys: Keys, out):
        _need(filt_dev, length, "legacy_probe_dev filter")
        _need(out, keys.n, "legacy_probe_dev out")
        ks = keys.c()
        check(lib().dlsm_bloom_legacy_probe_dev(self.h, _ptr(filt_dev), length, C.byref(ks),
                                                _ptr(out)), "legacy_probe_dev")


from .filter_block import BloomFilterPolicy, FullFilterBlockBuilder, FullFilterBlockReader  # noqa: E402
