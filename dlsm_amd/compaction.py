"""The compaction merge in pure Python (only open_output calls the library).

``MergingIterator`` (table/merger.cc:178-199) over the compaction's inputs
yields every pair in ``InternalKeyComparator::Compare`` order
(db/dbformat.cc:41-57): user keys ascending under ``Slice::compare`` -- which is
Python's ``bytes`` ordering -- and, within one user key, trailers descending;
``FindSmallest``'s strict ``<`` gives equal keys to the lower child first.  The
loop of ``DBImpl::DoCompactionWork`` (db/db_impl.cc:3500-3562) then drops what
rule (A) hides.  This module restates both so tests and callers can check the
device and host forms of ``dlsm_compaction_merge``.
"""
import struct

KEEP_ALL, DROP_HIDDEN = 0, 1
MAX_SEQUENCE = (1 << 56) - 1  # kMaxSequenceNumber (db/dbformat.h)


def trailer(ikey: bytes) -> int:
    return struct.unpack("<Q", ikey[-8:])[0]


def _varint(buf, p):
    v = shift = 0
    while True:
        b = buf[p]
        p += 1
        v |= (b & 127) << shift
        shift += 7
        if b < 128:
            return v, p


def table_pairs(index_contents: bytes, chunks):
    """One table as a compaction reads it (ByteAddressableSEQIterator,
    table/byte_addressable_SEQ_iterrator.cpp:48-184): the index block's
    contents give the entry count and, through the first entry's handle, the
    first pair's offset; from there the pairs are walked back to back through
    the chunks by their two Fixed32 lengths.  No other handle is looked at.
    Returns the (internal key, value) list."""
    n = struct.unpack("<I", index_contents[-4:])[0]
    if n == 0:
        return []
    _, p = _varint(index_contents, 0)       # shared
    klen, p = _varint(index_contents, p)    # non_shared
    _, p = _varint(index_contents, p)       # value_len
    at, _ = _varint(index_contents, p + klen)  # the handle's offset
    region = b"".join(chunks)               # offsets run on across the chunks
    pairs = []
    for _ in range(n):
        ks, vs = struct.unpack("<II", region[at:at + 8])
        pairs.append((region[at + 8:at + 8 + ks], region[at + 8 + ks:at + 8 + ks + vs]))
        at += 8 + ks + vs
    return pairs


def merge_runs(runs, policy=DROP_HIDDEN, snapshot=0):
    """runs: a list of runs, each a list of (internal key, value) in the run's
    order.  Returns (pairs, src): the surviving (internal key, value) in merged
    order and, per pair, run << 32 | index in run."""
    items = sorted(((ik[:-8], -trailer(ik), r, i) for r, run in enumerate(runs) for i, (ik, _) in enumerate(run)))
    pairs, src = [], []
    # last_seq is None where the reference holds kMaxSequenceNumber: "no earlier
    # entry of this user key" (a first occurrence is never hidden, as in
    # DLSM_SELECT_COMPACTION, even under a snapshot of kMaxSequenceNumber)
    has_current, current, last_seq = False, None, None
    for user, _, r, i in items:
        ik, value = runs[r][i]
        t = trailer(ik)
        drop = False
        if (t & 0xff) > 1:  # ParseInternalKey fails: "do not hide error keys"
            has_current, current, last_seq = False, None, None
        else:
            if not has_current or user != current:
                has_current, current, last_seq = True, user, None
            drop = policy == DROP_HIDDEN and last_seq is not None and last_seq <= snapshot  # rule (A)
            last_seq = t >> 8
        if not drop:
            pairs.append((ik, value))
            src.append(r << 32 | i)
    return pairs, src


def scan_runs(runs, start: bytes, snapshot: int, limit: int):
    """``DBIter`` (db/db_iter.cc:141-212, 283-298) over the merged runs after
    ``Seek(start)``, for ``limit`` calls of ``key()`` / ``Next()``: runs as for
    merge_runs, merged in its order.  Returns (pairs, src, bad_type): the
    yielded (internal key, value) list, run << 32 | index in run of each, and
    whether the iterator passed an entry whose type byte does not parse."""
    items = sorted(((ik[:-8], -trailer(ik), r, i) for r, run in enumerate(runs) for i, (ik, _) in enumerate(run)))
    pairs, src, bad_type = [], [], False
    skipping, skip = False, None  # FindNextUserEntry's state: entries of user key `skip` are hidden
    for user, neg, r, i in items:
        if len(pairs) == limit:
            break
        if (user, neg) < (start, -(snapshot << 8 | 1)):  # before where Seek(start || snapshot, kTypeForSeek) lands
            continue
        t = -neg
        if (t & 0xff) > 1:  # ParseKey fails: the entry is passed over
            bad_type = True
            continue
        if (t >> 8) > snapshot:
            continue
        if skipping and user == skip:
            continue
        skipping, skip = True, user  # a deletion hides the key's older entries; so does a yielded value, by Next()
        if (t & 0xff) == 1:
            pairs.append(runs[r][i])
            src.append(r << 32 | i)
    return pairs, src, bad_type


def open_output(ctx, data, index, chunk_end, files):
    """Open what ``Context.compaction_output_dev`` wrote where it lies: ``data``
    and ``index`` are the call's device tensors, ``chunk_end`` and ``files``
    host copies of its chunk ends and file records (one read each).  Returns a
    (TableIndex, TableData) pair over the files, file f of the call being file
    f of both."""
    import dlsm_amd

    blocks, chunks = [], []
    for d, ends, blk in dlsm_amd.output_tables(data, index, chunk_end, files):
        blocks.append(blk)
        begin = [0] + [int(e) for e in ends[:-1]]
        chunks.append([d[b:int(e)] for b, e in zip(begin, ends)])
    return dlsm_amd.TableIndex(ctx, blocks, on_device=True), dlsm_amd.TableData(ctx, chunks, on_device=True)


def open_filters(ctx, filters, recs, verify_checksums=True):
    """Open what ``Context.compaction_filters_dev`` wrote where it lies:
    ``filters`` is the call's device tensor, ``recs`` a host copy of its
    records (one read).  A filter set holds at most 64 filters, so the result
    is a list of FilterSets: file f is filter f % 64 of set f // 64.  The
    blocks' checksums are verified on the device."""
    import dlsm_amd

    blocks = dlsm_amd.filter_blocks(filters, recs)
    return [dlsm_amd.FilterSet(ctx, blocks[g:g + 64], on_device=True, sealed=True, verify_checksums=verify_checksums)
            for g in range(0, len(blocks), 64)]
