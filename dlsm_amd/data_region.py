"""The data region of a byte-addressable dLSM table, writer side.

``TableBuilder_BACS::Add`` (table/table_builder_bacs.cpp:221-226) appends every
key-value pair to the data buffer as ``Fixed32 key_size | Fixed32 value_size |
internal key | value`` and names it in the index block by ``BlockHandle{offset,
size}`` with ``size = 8 + key_size + value_size`` (table_builder_bacs.cpp:
202-203).  The buffer is flushed to a remote chunk before a pair that would not
fit (table_builder_bacs.cpp:186-189), so a pair never straddles two chunks, and
offsets run on across the chunks.  This module restates that writer so tests
and benchmarks can make data regions -- the builder itself needs the RDMA
headers; nothing here is on the read's path.
"""
from __future__ import annotations

import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np


def pair_bytes(internal_key: bytes, value: bytes) -> bytes:
    """One pair as Add appends it."""
    return struct.pack("<II", len(internal_key), len(value)) + bytes(internal_key) + bytes(value)


def build_region(pairs: Sequence[Tuple[bytes, bytes]], chunk_bytes: Optional[int] = None):
    """Add for every (internal key, value).  Returns (chunks, handles): the
    region as a list of chunks (bytes; one chunk when chunk_bytes is None, else
    a new chunk before every pair that would not fit in chunk_bytes, as
    FlushData does) and one (offset, size) per pair, offsets running across the
    chunks."""
    chunks: List[bytes] = []
    cur = bytearray()
    handles = []
    done = 0  # bytes in the finished chunks
    for k, v in pairs:
        p = pair_bytes(k, v)
        if chunk_bytes is not None and cur and len(cur) + len(p) > chunk_bytes:
            chunks.append(bytes(cur))
            done += len(cur)
            cur = bytearray()
        handles.append((done + len(cur), len(p)))
        cur += p
    chunks.append(bytes(cur))
    return chunks, handles


def build_region_fixed(keys: np.ndarray, values: np.ndarray):
    """build_region for n internal keys of one length (uint8[n, klen]) and n
    values of one length (uint8[n, vlen]) in one chunk, without a Python loop
    over the pairs.  Returns (region uint8[n * (8 + klen + vlen)], offsets
    uint64[n], sizes uint64[n])."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    values = np.ascontiguousarray(values, dtype=np.uint8)
    n, klen = keys.shape
    vlen = values.shape[1]
    if values.shape[0] != n:
        raise ValueError("one value per key")
    pair = 8 + klen + vlen
    out = np.empty((n, pair), dtype=np.uint8)
    out[:, 0:8] = np.frombuffer(struct.pack("<II", klen, vlen), dtype=np.uint8)
    out[:, 8:8 + klen] = keys
    out[:, 8 + klen:] = values
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(pair)
    return out.reshape(-1), offsets, np.full(n, pair, dtype=np.uint64)
