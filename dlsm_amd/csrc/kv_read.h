// dlsm_amd/csrc/kv_read.h -- the tail of Table::InternalGet for a byte-addressable
// table (table/table.cc:482-508): which data chunk holds the pair a BlockHandle
// names (Find_Remote_MR, table/format.cc:63-75), the two Fixed32 lengths in
// front of the pair (TableBuilder_BACS::Add, table_builder_bacs.cpp:221-226),
// and SaveValue on the pair's own key (db/version_set.h:61-75).  Shared by the
// kernels (kv_read.hip), the host-only ABI call (bloom_capi.hip), the adapter's
// host path and the CPU test (tests/cpp/kv_read_test.cc).  Plain integer code:
// no device call.
//
// A file's data is a list of chunks in offset order; chunk c covers the offsets
// [end[c - 1], end[c]) with end[-1] = 0.  A pair at `offset` is
//   [Fixed32 key_size][Fixed32 value_size][internal key][value]
// of size = 8 + key_size + value_size bytes, and never straddles two chunks (the
// builder flushes first, table_builder_bacs.cpp:186-189).
#pragma once
#include <stdint.h>
#include <string.h>

#include "index_seek.h"

namespace dlsm {

constexpr uint32_t kKvChunk = 1024;    // items per workgroup chunk of the size and offset passes (a thread each)
constexpr uint32_t kKvSpan = 65536;    // output bytes per workgroup step of the copy
constexpr uint32_t kKvWindow = 1023;   // items whose offsets and sources a copy step stages in LDS
constexpr uint32_t kKvCopyWgsPerCu = 2;  // the copy's persistent grid: workgroups per compute unit of the device
constexpr uint32_t kKvCopyWgs = 512;   // ... where the device does not say how many it has: 256 CUs
constexpr uint32_t kKvPairMin = 16;    // two lengths and the least internal key
static_assert(kKvSpan % 16 == 0, "a span is whole 16-byte units");

// One file's chunks as the lookup sees them: end[c] is the running sum of the
// chunks' lengths, base[c] the address of chunk c's first byte.  n == 0: no
// data is held for the file.
struct KvChunks {
  const uint64_t* end;
  const uint8_t* const* base;
  uint32_t n;
};

// Find_Remote_MR: the first chunk whose end is above the offset (upper_bound:
// an offset equal to a chunk's end belongs to the next chunk); n where there is
// none.  Uniform length, one load per step.
DLSM_HD uint32_t kv_chunk_find(const uint64_t* end, uint32_t n, uint64_t offset) {
  uint32_t c = 0;
  for (uint32_t len = n; len;) {
    const uint32_t half = len >> 1;
    const bool le = end[c + half] <= offset;
    c = le ? c + half + 1 : c;
    len = le ? len - half - 1 : half;
  }
  return c;
}

// The address of the pair {offset, size}, or nullptr where the handle names no
// size bytes of one chunk (no chunk, a straddle, fewer bytes than a pair has).
DLSM_HD const uint8_t* kv_pair_locate(const KvChunks& f, uint64_t offset, uint32_t size) {
  if (size < kKvPairMin) return nullptr;
  const uint32_t c = kv_chunk_find(f.end, f.n, offset);
  if (c >= f.n) return nullptr;
  if (f.end[c] - offset < size) return nullptr;  // offset + size <= end[c], without the sum
  const uint64_t start = c ? f.end[c - 1] : 0;
  return f.base[c] + (offset - start);
}

// The decision for a located pair p of `size` (>= 16) bytes under an incoming
// DLSM_GET_FOUND: CORRUPT with length 0 unless the lengths add up to the
// handle's size (table.cc:501's assert), the type byte is a value type and the
// pair's user key is the Get's; then DELETED (length 0) or FOUND with the value.
DLSM_HD uint8_t kv_pair_decide(const uint8_t* p, uint32_t size, const uint8_t* user, uint32_t un,
                               const uint8_t** value, uint32_t* value_len) {
  *value = nullptr;
  *value_len = 0;
  const uint32_t key_size = index_fixed32(p), value_size = index_fixed32(p + 4);
  if (key_size < 8) return kGetCorrupt;
  if (uint64_t(8) + key_size + value_size != size) return kGetCorrupt;
  const uint32_t type = p[8 + key_size - 8];  // the trailer's low byte
  if (type > 1) return kGetCorrupt;
  if (index_compare_bytes(p + 8, key_size - 8, user, un) != 0) return kGetCorrupt;
  if (type == 0) return kGetDeleted;
  *value = p + 8 + key_size;
  *value_len = value_size;
  return kGetFound;
}

// The data of a table set: file f's chunks are [chunk_begin[f], chunk_begin[f + 1])
// of end / base.
struct KvTables {
  const uint32_t* chunk_begin;  // u32[n_files + 1]
  const uint64_t* end;
  const uint8_t* const* base;
  uint32_t n_files;
};

// One FOUND item: the handle checked against the tables, then the pair.
DLSM_HD uint8_t kv_item_decide(const KvTables& t, const KvHandle& h, const uint8_t* user, uint32_t un,
                               const uint8_t** value, uint32_t* value_len) {
  *value = nullptr;
  *value_len = 0;
  if (h.file >= t.n_files) return kGetCorrupt;
  const uint32_t c0 = t.chunk_begin[h.file], c1 = t.chunk_begin[h.file + 1];
  const KvChunks f{t.end + c0, t.base + c0, c1 - c0};
  const uint8_t* p = kv_pair_locate(f, h.offset, h.size);
  if (!p) return kGetCorrupt;
  return kv_pair_decide(p, h.size, user, un, value, value_len);
}

// The last i in [0, n) with off[i] <= p, given off[0] <= p (n >= 1): the item
// of output byte p is upper_bound(off, p) - 1, which skips empty values.
// Uniform length for one n.
DLSM_HD uint64_t kv_last_le(const uint64_t* off, uint64_t n, uint64_t p) {
  uint64_t i = 0;
  for (uint64_t len = n; len > 1;) {
    const uint64_t half = len >> 1;
    const bool right = off[i + half] <= p;
    i = right ? i + half : i;
    len = right ? len - half : half;
  }
  return i;
}

typedef unsigned __int128 kv_u128;
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t kv_u32x4 __attribute__((ext_vector_type(4)));
typedef kv_u32x4 kv_u32x4_u __attribute__((aligned(1)));
// the source addresses come out of memory as integers: say that they are global
typedef const __attribute__((address_space(1))) kv_u32x4_u* kv_src16;
typedef const __attribute__((address_space(1))) uint8_t* kv_src1;
#else
typedef const uint8_t* kv_src1;
#endif

// The copy's unit: the 16 output bytes at u (a multiple of 16, u < p1; values
// 16-byte aligned), p1 the end of the bytes to write.  off / src are addressed
// from an item at or before u's: off[0] <= u, off[n] >= p1, n >= 1 items, src[i]
// the address of item i's value.  A unit inside one value is one unaligned
// 16-byte load and one aligned 16-byte store; one that holds the boundary of
// two values of 16 bytes or more is two such loads and one store; any other
// boundary is assembled per byte and stored once; the partial unit at p1 is
// stored per byte.  Reads no byte outside the values and writes none outside [u, p1).
DLSM_HD void kv_copy_unit(const uint64_t* off, const uint64_t* src, uint64_t n, uint64_t u, uint64_t p1,
                          uint8_t* values) {
  uint64_t i = kv_last_le(off, n, u);
  const bool full = u + 16 <= p1;
  if (full && off[i + 1] >= u + 16) {  // inside one value
#if defined(__HIP_DEVICE_COMPILE__)
    const kv_u32x4 x = *reinterpret_cast<kv_src16>(src[i] + (u - off[i]));
    __builtin_nontemporal_store(x, reinterpret_cast<kv_u32x4*>(values + u));
#else
    memcpy(values + u, reinterpret_cast<const uint8_t*>(src[i] + (u - off[i])), 16);
#endif
    return;
  }
  // The common boundary: the unit holds the end of one value and the start of
  // the next, each at least 16 bytes long.  The last 16 bytes of the first and
  // the first 16 of the second are two independent loads inside their values;
  // as little-endian 128-bit numbers the unit is (A >> 8 (16 - k)) | (B << 8 k),
  // k = the first value's bytes in the unit (1..15).
  if (full && off[i + 1] > u && off[i + 1] - off[i] >= 16 && off[i + 2] - off[i + 1] >= 16) {  // (off[i + 1] < u + 16 <= off[n])
    const uint32_t k = static_cast<uint32_t>(off[i + 1] - u);
    const uint64_t pa = src[i] + (off[i + 1] - off[i]) - 16, pb = src[i + 1];
#if defined(__HIP_DEVICE_COMPILE__)
    const kv_u32x4 xa = *reinterpret_cast<kv_src16>(pa), xb = *reinterpret_cast<kv_src16>(pb);
    const kv_u128 A = (static_cast<kv_u128>(xa.w) << 96) | (static_cast<kv_u128>(xa.z) << 64) |
                      (static_cast<kv_u128>(xa.y) << 32) | xa.x;
    const kv_u128 B = (static_cast<kv_u128>(xb.w) << 96) | (static_cast<kv_u128>(xb.z) << 64) |
                      (static_cast<kv_u128>(xb.y) << 32) | xb.x;
#else
    kv_u128 A, B;
    memcpy(&A, reinterpret_cast<const uint8_t*>(pa), 16);
    memcpy(&B, reinterpret_cast<const uint8_t*>(pb), 16);
#endif
    const kv_u128 r = (A >> (8 * (16 - k))) | (B << (8 * k));
#if defined(__HIP_DEVICE_COMPILE__)
    const kv_u32x4 x = {static_cast<uint32_t>(r), static_cast<uint32_t>(r >> 32), static_cast<uint32_t>(r >> 64),
                        static_cast<uint32_t>(r >> 96)};
    __builtin_nontemporal_store(x, reinterpret_cast<kv_u32x4*>(values + u));
#else
    memcpy(values + u, &r, 16);
#endif
    return;
  }
  uint64_t lo = 0, hi = 0;
  for (uint32_t b = 0; b < 16; b++) {
    const uint64_t p = u + b;
    if (p >= p1) break;
    if (off[i + 1] <= p) i = i + 1 + kv_last_le(off + i + 1, n - i - 1, p);  // p < p1 <= off[n]: i + 1 < n
    const uint64_t x = reinterpret_cast<kv_src1>(src[i])[p - off[i]];
    if (!full) values[p] = static_cast<uint8_t>(x);
    lo |= b < 8 ? x << (8 * b) : 0;
    hi |= b >= 8 ? x << (8 * (b - 8)) : 0;
  }
  if (!full) return;
#if defined(__HIP_DEVICE_COMPILE__)
  const kv_u32x4 x = {static_cast<uint32_t>(lo), static_cast<uint32_t>(lo >> 32), static_cast<uint32_t>(hi),
                      static_cast<uint32_t>(hi >> 32)};
  __builtin_nontemporal_store(x, reinterpret_cast<kv_u32x4*>(values + u));
#else
  memcpy(values + u, &lo, 8);
  memcpy(values + u + 8, &hi, 8);
#endif
}

}  // namespace dlsm
