// dlsm_amd/csrc/index_seek.h -- Table::InternalGet's index step for a
// byte-addressable table (table/table.cc:452-513): the entry decoder, the
// comparator, the validation rules, the fence rule and the state decision,
// shared by the kernels (index_seek.hip), the host-only ABI calls
// (bloom_capi.hip) and the CPU test (tests/cpp/index_seek_test.cc).  Plain
// integer code: no device call.
//
// An index block's contents (TableBuilder_BACS::Add, table_builder_bacs.cpp:
// 195-206, through BlockBuilder at restart interval 1, block_builder.cc:74-127):
//   n entries  [varint32 shared = 0][varint32 non_shared][varint32 value_len]
//              [internal key: user key || Fixed64(seq << 8 | type)]
//              [BlockHandle: varint64 offset, varint64 size]
//   n x Fixed32 restart offsets (one per entry), Fixed32 n
// Nothing here is compiled from the reference: Block and BlockBuilder cannot be
// built outside an RDMA host, so this is a restatement of the lines cited.
#pragma once
#include <stdint.h>
#include <string.h>

#include "bloom_math.h"
#include "shard_route.h"

namespace dlsm {

// Entries per fence (the fence table holds the 16-byte user-key prefix of
// every kIndexFenceS-th entry).  A named constant; profiles/ holds what was
// measured about it (A/B builds: make variant VFLAGS=-DDLSM_INDEX_FENCE_S=8).
#ifndef DLSM_INDEX_FENCE_S
#define DLSM_INDEX_FENCE_S 16
#endif
constexpr uint32_t kIndexFenceS = DLSM_INDEX_FENCE_S;
static_assert(kIndexFenceS >= 2, "a window needs an entry between two fences");
// The least bytes an entry takes: 3 header bytes, an 8-byte internal key, two
// 1-byte varints and its restart offset -- bounds a block's entry count by its
// length alone.
constexpr uint32_t kIndexEntryMinBytes = 3 + 8 + 2 + 4;

enum : uint8_t { kGetNotFound = 0, kGetFound = 1, kGetDeleted = 2, kGetCorrupt = 3 };  // DLSM_GET_*

struct KvHandle {  // dlsm_kv_handle
  uint64_t offset;
  uint32_t size;
  uint32_t file;
};

DLSM_HD uint32_t index_fixed32(const uint8_t* p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;  // little-endian hosts and devices only (util/coding.h:184-193 takes the same shortcut)
}
DLSM_HD uint64_t index_fixed64(const uint8_t* p) {
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
}
DLSM_HD uint64_t index_be64(const uint8_t* p) { return __builtin_bswap64(index_fixed64(p)); }

// An index block's contents as the searches see them.  n == 0: no entry.
struct IndexView {
  const uint8_t* data;
  uint32_t restarts;  // offset of the restart array = the end of the entries
  uint32_t n;         // num_restarts = entries
};

// Block's ctor checks (table/block.cc:18-35): false where it sets size_ = 0.
DLSM_HD bool index_view(const uint8_t* data, uint64_t len, IndexView* v) {
  v->data = data;
  v->restarts = 0;
  v->n = 0;
  if (len < 4 || len > 0xffffffffull) return false;
  const uint32_t n = index_fixed32(data + len - 4);
  if (n > (len - 4) / 4) return false;
  v->n = n;
  v->restarts = static_cast<uint32_t>(len) - (1 + n) * 4;
  return true;
}

DLSM_HD uint32_t index_restart(const IndexView& v, uint32_t i) { return index_fixed32(v.data + v.restarts + 4u * i); }

// GetVarint32Ptr (util/coding.cc:120-148): at most 5 bytes, bits past 32 lost.
// Returns the offset behind the varint, or 0 on failure (p > 0 always holds on
// success since a varint takes a byte).
DLSM_HD uint32_t index_varint32(const uint8_t* d, uint32_t p, uint32_t limit, uint32_t* out) {
  uint32_t r = 0;
  for (uint32_t shift = 0; shift <= 28 && p < limit; shift += 7) {
    const uint32_t b = d[p++];
    r |= (b & 127u) << shift;
    if (b < 128u) {
      *out = r;
      return p;
    }
  }
  return 0;
}
// GetVarint64Ptr (util/coding.cc:150-176): at most 10 bytes.
DLSM_HD uint32_t index_varint64(const uint8_t* d, uint32_t p, uint32_t limit, uint64_t* out) {
  uint64_t r = 0;
  for (uint32_t shift = 0; shift <= 63 && p < limit; shift += 7) {
    const uint64_t b = d[p++];
    r |= (b & 127u) << shift;
    if (b < 128u) {
      *out = r;
      return p;
    }
  }
  return 0;
}

struct IndexEntry {
  uint32_t key;      // offset of the internal key
  uint32_t key_len;  // non_shared
  uint32_t val;      // offset of the value = key + key_len
  uint32_t val_len;
  uint32_t shared;
};

// DecodeEntry (table/block.h:63-83) of the entry at offset `at`, limit = the
// restart array.  false where it returns nullptr.  Reads no byte at or past
// v.restarts.
DLSM_HD bool index_decode(const IndexView& v, uint32_t at, IndexEntry* e) {
  const uint32_t limit = v.restarts;
  if (at > limit || limit - at < 3) return false;
  const uint8_t* d = v.data;
  uint32_t sh = d[at], ns = d[at + 1], vl = d[at + 2], p;
  if ((sh | ns | vl) < 128) {
    p = at + 3;
  } else {
    if (!(p = index_varint32(d, at, limit, &sh))) return false;
    if (!(p = index_varint32(d, p, limit, &ns))) return false;
    if (!(p = index_varint32(d, p, limit, &vl))) return false;
  }
  if (static_cast<uint64_t>(limit - p) < static_cast<uint64_t>(ns) + vl) return false;
  e->shared = sh;
  e->key = p;
  e->key_len = ns;
  e->val = p + ns;
  e->val_len = vl;
  return true;
}

// BlockHandle::DecodeFrom (table/format.cc:23-29) of an entry's value.
DLSM_HD bool index_handle(const IndexView& v, const IndexEntry& e, uint64_t* offset, uint64_t* size) {
  const uint32_t end = e.val + e.val_len;
  uint32_t p = index_varint64(v.data, e.val, end, offset);
  if (!p) return false;
  return index_varint64(v.data, p, end, size) != 0;
}

// BytewiseComparator on two byte strings (memcmp over the common length, then
// the shorter first), eight bytes at a time where both have them.
DLSM_HD int index_compare_bytes(const uint8_t* a, uint32_t an, const uint8_t* b, uint32_t bn) {
  const uint32_t n = an < bn ? an : bn;
  uint32_t j = 0;
  for (; j + 8 <= n; j += 8) {
    const uint64_t x = index_be64(a + j), y = index_be64(b + j);
    if (x != y) return x < y ? -1 : 1;
  }
  for (; j < n; j++)
    if (a[j] != b[j]) return a[j] < b[j] ? -1 : 1;
  return an < bn ? -1 : (an > bn ? 1 : 0);
}

// InternalKeyComparator::Compare (db/dbformat.cc:41-57) of the internal key
// (ik, ikn >= 8) against the target user key || Fixed64(trailer): user keys
// ascending, then trailers descending.
DLSM_HD int index_compare_target(const uint8_t* ik, uint32_t ikn, const uint8_t* user, uint32_t un, uint64_t trailer) {
  const int r = index_compare_bytes(ik, ikn - 8, user, un);
  if (r) return r;
  const uint64_t t = index_fixed64(ik + ikn - 8);
  return t > trailer ? -1 : (t < trailer ? 1 : 0);
}
DLSM_HD int index_compare_internal(const uint8_t* a, uint32_t an, const uint8_t* b, uint32_t bn) {
  return index_compare_target(a, an, b, bn - 8, index_fixed64(b + bn - 8));
}

// LookupKey's trailer (db/dbformat.h:74-81): PackSequenceAndType(snapshot, kValueTypeForSeek = 1).
DLSM_HD uint64_t index_seek_trailer(uint64_t snapshot) { return (snapshot << 8) | 1u; }

// ---- validation: one call per entry -----------------------------------------
// What the open checks of entry i (0 <= i < v.n) so that no seek reads outside
// the block and the binary search is well defined; independent per entry (entry
// i looks at restart i - 1, i, i + 1 and decodes entries i - 1 and i).
DLSM_HD bool index_entry_valid(const IndexView& v, uint32_t i) {
  const uint32_t at = index_restart(v, i);
  if (i == 0 ? at != 0 : index_restart(v, i - 1) >= at) return false;  // restart[0] == 0, strictly ascending
  IndexEntry e;
  if (!index_decode(v, at, &e)) return false;
  if (e.shared != 0 || e.key_len < 8) return false;  // block.h:235, block_builder.cc:88
  const uint32_t next = i + 1 < v.n ? index_restart(v, i + 1) : v.restarts;
  if (e.val + e.val_len != next) return false;       // ends exactly where the next one starts
  uint64_t off, size;
  if (!index_handle(v, e, &off, &size) || size > 0xffffffffull) return false;  // (dlsm_kv_handle.size is 32 bits)
  if (i > 0) {
    IndexEntry p;  // entry i - 1's own call rejects it where it does not decode
    if (index_decode(v, index_restart(v, i - 1), &p) && p.key_len >= 8 &&
        index_compare_internal(v.data + p.key, p.key_len, v.data + e.key, e.key_len) >= 0)
      return false;  // entry i sorts strictly after entry i - 1
  }
  return true;
}

// The block-level checks (one call per block), beyond index_view's: the entry
// count fits the bytes there are.
DLSM_HD bool index_header_valid(const uint8_t* data, uint64_t len, IndexView* v) {
  if (!index_view(data, len, v)) return false;
  if (v->n <= (len - 4) / kIndexEntryMinBytes) return true;
  v->n = 0;
  return false;
}

// The fence of entry i (a valid block): its user key's 16-byte prefix.
DLSM_HD RoutePrefix index_entry_prefix(const IndexView& v, uint32_t i) {
  IndexEntry e;
  if (!index_decode(v, index_restart(v, i), &e) || e.key_len < 8) return RoutePrefix{0, 0};
  return route_prefix(v.data + e.key, e.key_len - 8);
}
DLSM_HD uint32_t index_fence_count(uint32_t n, uint32_t S) { return (n + S - 1) / S; }

// ---- the search -----------------------------------------------------------------
// The fence rule.  fence[j] (j < nf = ceil(n / S)) is entry j * S's prefix; q is
// the target's.  Prefixes order user keys where they differ, so every entry
// whose prefix is below q sorts below the target and every entry whose prefix
// is above q sorts above it: the first entry >= target lies in [lo, hi], where
// lo follows the last fence strictly below q and hi is the first fence strictly
// above q (or n).  *lo, *hi bound the window search: first entry >= target in
// [lo, hi), else hi.
DLSM_HD void index_fence_window(const RoutePrefix* fence, uint32_t nf, uint32_t n, uint32_t S, const RoutePrefix& q,
                                uint32_t* lo, uint32_t* hi) {
  uint32_t a = 0;  // fences [0, a) are strictly below q
  for (uint32_t len = nf; len;) {  // branchless lower bound: one load per step
    const uint32_t half = len >> 1;
    const RoutePrefix p = fence[a + half];
    const bool below = route_prefix_lt(p, q);
    a = below ? a + half + 1 : a;
    len = below ? len - half - 1 : half;
  }
  uint32_t b = a;  // fences [a, b) equal q
  if (b < nf && !route_prefix_lt(q, fence[b])) {
    uint32_t x = b + 1, len = nf - x;  // upper bound behind the first tie
    while (len) {
      const uint32_t half = len >> 1;
      const bool le = !route_prefix_lt(q, fence[x + half]);
      x = le ? x + half + 1 : x;
      len = le ? len - half - 1 : half;
    }
    b = x;
  }
  *lo = a ? (a - 1) * S + 1 : 0;
  const uint64_t h = static_cast<uint64_t>(b) * S;
  *hi = (b < nf && h < n) ? static_cast<uint32_t>(h) : n;
}

// Block::Iter::Seek's result (block.h:205-273) inside [lo, hi]: the first entry
// whose internal key is >= the target, n when there is none.  Two dependent
// loads per step (restart offset, entry).  A touched entry that does not decode
// (never in an opened block) ends the search with n, as CorruptionError leaves
// the iterator invalid.
DLSM_HD uint32_t index_window_search(const IndexView& v, uint32_t lo, uint32_t hi, const uint8_t* user, uint32_t un,
                                     uint64_t trailer) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    IndexEntry e;
    if (!index_decode(v, index_restart(v, mid), &e) || e.shared != 0 || e.key_len < 8) return v.n;
    if (index_compare_target(v.data + e.key, e.key_len, user, un, trailer) < 0) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The state decision (table.cc:469-510 with SaveValue, db/version_set.h:61-75)
// for the entry the seek stopped at (pos == v.n: the iterator is invalid).
// NOTFOUND leaves a zero handle.
DLSM_HD uint8_t index_decide(const IndexView& v, uint32_t pos, const uint8_t* user, uint32_t un, uint32_t file,
                             KvHandle* h) {
  h->offset = 0;
  h->size = 0;
  h->file = 0;
  if (pos >= v.n) return kGetNotFound;
  IndexEntry e;
  if (!index_decode(v, index_restart(v, pos), &e) || e.key_len < 8) return kGetNotFound;
  const uint32_t type = v.data[e.key + e.key_len - 8];  // the trailer's low byte
  uint8_t state;
  if (type > 1) state = kGetCorrupt;  // ParseInternalKey fails (dbformat.h:451-461): no user-key compare
  else if (index_compare_bytes(v.data + e.key, e.key_len - 8, user, un) != 0) return kGetNotFound;
  else state = type == 1 ? kGetFound : kGetDeleted;
  uint64_t off = 0, size = 0;
  (void)index_handle(v, e, &off, &size);
  h->offset = off;
  h->size = static_cast<uint32_t>(size);
  h->file = file;
  return state;
}

// InternalGet's index step for one key on one block without fences (the
// per-Get path and the host fallback).
DLSM_HD uint8_t index_block_seek(const IndexView& v, const uint8_t* user, uint32_t un, uint64_t snapshot,
                                 uint32_t file, KvHandle* h) {
  const uint32_t pos = v.n ? index_window_search(v, 0, v.n, user, un, index_seek_trailer(snapshot)) : 0;
  return index_decide(v, pos, user, un, file, h);
}

}  // namespace dlsm
