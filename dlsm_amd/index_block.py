"""The index block of a byte-addressable dLSM table, writer side.

``TableBuilder_BACS::Add`` (table/table_builder_bacs.cpp:195-206) adds one
index entry per key-value pair: the internal key and ``BlockHandle{offset,
size}`` of that pair, through a ``BlockBuilder`` at restart interval 1
(table_builder_bacs.cpp:27, table/block_builder.cc:74-127), and the block is
sealed like every other (``[contents][type 0][masked crc32c]``,
table_builder_bacs.cpp:313-358).  This module restates that writer so tests and
benchmarks can make index blocks; nothing here is on the seek's path.

An entry is ``varint32 shared (0) | varint32 non_shared | varint32 value_len |
internal key | varint64 offset | varint64 size``; behind the entries come one
Fixed32 restart offset per entry and Fixed32 num_restarts.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Sequence, Tuple

import numpy as np

from . import lib


def varint(v: int) -> bytes:
    """PutVarint32 / PutVarint64 (util/coding.cc:47-94)."""
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def encode_handle(offset: int, size: int) -> bytes:
    """BlockHandle::EncodeTo (table/format.cc:15-21)."""
    return varint(offset) + varint(size)


def internal_key(user_key: bytes, sequence: int, value_type: int) -> bytes:
    """user key || Fixed64(sequence << 8 | type) (db/dbformat.cc:19-22)."""
    return bytes(user_key) + struct.pack("<Q", (sequence << 8) | value_type)


def seal(contents) -> bytes:
    """contents || type 0 || Fixed32(crc32c::Mask(crc32c(contents || type)))."""
    body = np.concatenate([np.frombuffer(contents, dtype=np.uint8) if not isinstance(contents, np.ndarray)
                           else contents, np.zeros(1, dtype=np.uint8)])
    crc = lib().dlsm_crc32c_extend(0, C.c_void_p(body.ctypes.data), body.size)
    return body.tobytes() + struct.pack("<I", lib().dlsm_crc32c_mask(crc))


def build_index_contents(internal_keys: Sequence[bytes], handles: Sequence[Tuple[int, int]]) -> bytes:
    """BlockBuilder::Add for every (key, handle) at restart interval 1, then
    Finish.  The keys go in as given: the caller sorts them (BlockBuilder only
    asserts the order)."""
    out = bytearray()
    restarts = []
    for k, (off, size) in zip(internal_keys, handles):
        v = encode_handle(off, size)
        restarts.append(len(out))
        out += varint(0) + varint(len(k)) + varint(len(v)) + bytes(k) + v
    for r in restarts:
        out += struct.pack("<I", r)
    out += struct.pack("<I", len(restarts))
    return bytes(out)


def build_index_block(internal_keys: Sequence[bytes], handles: Sequence[Tuple[int, int]]) -> bytes:
    """The sealed index block of a table holding these pairs."""
    return seal(build_index_contents(internal_keys, handles))


def _varint_lens(v: np.ndarray) -> np.ndarray:
    n = np.ones(v.shape, dtype=np.int64)
    for j in range(1, 10):
        n += (v >= np.uint64(1) << np.uint64(7 * j)).astype(np.int64)
    return n


def build_index_contents_fixed(keys: np.ndarray, offsets: np.ndarray, sizes: np.ndarray) -> np.ndarray:
    """build_index_contents for n internal keys of one length (uint8[n, klen])
    and handle arrays (uint64[n]), without a Python loop over the entries.
    Returns the contents as uint8."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    n, klen = keys.shape
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    lo, ls = _varint_lens(offsets), _varint_lens(sizes)
    vlen = lo + ls  # <= 20: one byte
    head = varint(0) + varint(klen)
    hl = len(head) + 1
    elen = hl + klen + vlen
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(elen, out=start[1:])
    total = int(start[n])
    if total + 4 * (n + 1) > 0xFFFFFFFF:
        raise ValueError("index block past 4 GiB")
    out = np.zeros(total + 4 * (n + 1), dtype=np.uint8)
    at = start[:n]
    for j, b in enumerate(head):
        out[at + j] = b
    out[at + len(head)] = vlen.astype(np.uint8)
    out[(at + hl)[:, None] + np.arange(klen)[None, :]] = keys
    for val, ln, base in ((offsets, lo, at + hl + klen), (sizes, ls, at + hl + klen + lo)):
        for j in range(10):
            m = ln > j
            if not m.any():
                break
            byte = ((val[m] >> np.uint64(7 * j)) & np.uint64(127)).astype(np.uint8)
            byte |= np.where(ln[m] > j + 1, 128, 0).astype(np.uint8)
            out[base[m] + j] = byte
    tail = np.empty(n + 1, dtype="<u4")
    tail[:n] = at
    tail[n] = n
    out[total:] = tail.view(np.uint8)
    return out


def build_index_block_fixed(keys: np.ndarray, offsets: np.ndarray, sizes: np.ndarray) -> bytes:
    """The sealed form of build_index_contents_fixed."""
    return seal(build_index_contents_fixed(keys, offsets, sizes))
