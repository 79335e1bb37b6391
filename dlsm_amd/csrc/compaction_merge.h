// dlsm_amd/csrc/compaction_merge.h -- the rules of the compaction merge: what
// MergingIterator (table/merger.cc:178-199) over MakeInputIterator's children
// (db/version_set.cc:1565-1596) hands to the loop of DBImpl::DoCompactionWork
// (db/db_impl.cc:3500-3562), that loop's drop rule (A), and the order of
// InternalKeyComparator::Compare (db/dbformat.cc:41-57).  Shared by the kernels
// (compaction_merge.hip), the planner (host_plan.h) and the host form
// (bloom_capi.hip).  Plain integer code: no device call.  Nothing here is
// compiled from the reference: a restatement of the lines cited.
//
// Every input pair becomes one 32-byte merge record; the merge moves records
// only, and the pairs' bytes move once, in the gather.  A record holds
//   hi, lo   RoutePrefix of the user key: its first 16 bytes, zero-padded,
//            big-endian (shard_route.h);
//   inv      ~trailer: ascending inv is descending (sequence, type);
//   ref      index in run | run << 32 | length class << 40, the class
//            min(user key length, 17).
// Record compare (cm_rec_cmp):
//   the prefixes differ                  -> decided (shard_route.h's argument);
//   equal, one key of 16 bytes or fewer  -> the classes decide: the shorter key's
//            pad zeros equal the longer key's bytes, so it is a proper prefix
//            of the longer one and sorts first; equal classes are equal keys;
//   equal, both keys longer than 16      -> route_compare of the user keys
//            through the references (the only path that reads key bytes);
//   equal user keys                      -> inv decides.
// Records that compare equal leave in ascending (run, index): a pass's left
// segment holds the lower runs and wins ties, and a run's own records ascend
// strictly.
//
// A run comes in one of three forms: keys and values packed at one length each,
// packed with offsets, or -- for runs read out of opened tables (table_scan.h)
// -- one 16-byte descriptor per pair.  Which form a call's runs have is a
// template argument D of everything that reads pairs through a run, so the
// packed forms' code holds no trace of the descriptors.
#pragma once
#include <stdint.h>

#include "shard_route.h"
#include "table_build.h"

namespace dlsm {

constexpr uint32_t kCmChunk = 1024;      // pairs per workgroup chunk of the record, decide and offset passes
constexpr uint32_t kCmLane = 4;          // records a lane merges serially per tile
constexpr uint32_t kCmTileLanes = 256;   // lanes (threads) of a merge workgroup
constexpr uint32_t kCmTile = kCmLane * kCmTileLanes;  // records per workgroup step of a merge pass (32 KiB of LDS)
constexpr uint32_t kCmSpan = 65536;      // output bytes per workgroup step of the gather
constexpr uint32_t kCmWindow = 1023;     // pairs whose offsets and sources a gather step stages in LDS
constexpr uint32_t kCmMaxRuns = 64;
constexpr uint32_t kCmMaxPasses = 6;     // ceil(log2(kCmMaxRuns))
constexpr uint32_t kCmLaunchKinds = 6;   // record, partition, merge, decide, offsets, gather
static_assert(kCmSpan % 16 == 0, "a span is whole 16-byte units");
static_assert(kCmTile * 32 * 2 <= 160 * 1024 / 2, "two merge workgroups share a compute unit with room to spare");

enum : uint64_t {  // DLSM_MERGE_* of the public header
  kCmKeysCap = 1,
  kCmValuesCap = 2,
  kCmPairCap = 4,
  kCmShortKey = 8,
  kCmUnsorted = 16,
  kCmTableMismatch = 32,
};

struct CmRec {
  uint64_t hi, lo, inv, ref;
};
static_assert(sizeof(CmRec) == 32, "a record is two 16-byte units");

// A pair of a data region as the table record pass leaves it (table_scan.h):
// the address of its header [Fixed32 key_size][Fixed32 value_size], the key
// behind it and the value behind the key.  One 16-byte load.
struct alignas(16) CmDesc {
  uint64_t addr;
  uint32_t key_size, value_size;
};
static_assert(sizeof(CmDesc) == 16, "a descriptor is one 16-byte unit");

// One input run as the passes address it, pair by pair.
struct CmRun {
  const uint8_t* kbytes;
  const uint64_t* koff;  // or nullptr: klen each
  const uint8_t* vbytes;
  const uint64_t* voff;  // or nullptr: vlen each
  uint32_t klen, vlen;
  const CmDesc* desc;    // the descriptor form (D): pair i is desc[i], nothing else is looked at
  DLSM_HD uint64_t key_size(uint64_t i) const { return koff ? koff[i + 1] - koff[i] : klen; }
  DLSM_HD uint64_t value_size(uint64_t i) const { return voff ? voff[i + 1] - voff[i] : vlen; }
  DLSM_HD uint64_t key_src(uint64_t i) const { return reinterpret_cast<uint64_t>(kbytes) + (koff ? koff[i] : i * klen); }
  DLSM_HD uint64_t value_src(uint64_t i) const { return reinterpret_cast<uint64_t>(vbytes) + (voff ? voff[i] : i * vlen); }
};

// Pair i of a run, whatever its form.
struct CmPairAt {
  uint64_t key_src, value_src, key_size, value_size;
};
template <bool D>
DLSM_HD CmPairAt cm_pair_at(const CmRun& r, uint64_t i) {
  if (D) {
    const CmDesc d = r.desc[i];
    return CmPairAt{d.addr + 8, d.addr + 8 + d.key_size, d.key_size, d.value_size};
  }
  return CmPairAt{r.key_src(i), r.value_src(i), r.key_size(i), r.value_size(i)};
}

// One two-way merge of a pass: the neighbouring segments [a0, b0) and [b0, b1)
// of record positions become [a0, b1); tile0 is its first tile among the
// pass's tiles.  An unpaired segment is a pair with b0 == b1.
struct CmPair {
  uint32_t a0, b0, b1, tile0;
};

// What the kernels read besides the records: the runs, the first record
// position of every run (base[n_runs] = n), and the passes' pairs -- pass p
// merges segments of 2^p runs, its pairs are pairs[pair0[p], pair0[p + 1]).
struct CmTable {
  CmRun runs[kCmMaxRuns];
  uint64_t base[kCmMaxRuns + 1];
  CmPair pairs[kCmMaxRuns];
  uint32_t pair0[kCmMaxPasses + 1];
  uint32_t tiles[kCmMaxPasses];
  uint32_t n_runs, n_passes;
};

DLSM_HD uint32_t cm_run(const CmRec& r) { return static_cast<uint32_t>(r.ref >> 32) & 0xffu; }
DLSM_HD uint64_t cm_index(const CmRec& r) { return r.ref & 0xffffffffull; }
DLSM_HD uint32_t cm_class(const CmRec& r) { return static_cast<uint32_t>(r.ref >> 40); }
DLSM_HD uint64_t cm_src(const CmRec& r) { return r.ref & 0xffffffffffull; }  // run << 32 | index
DLSM_HD uint64_t cm_trailer(const CmRec& r) { return ~r.inv; }

// The record of pair idx of run `run`, its internal key the ks >= 8 bytes at
// src.  A key of 16 bytes or more is two 16-byte loads inside it, a shorter one
// is read per byte.
DLSM_HD CmRec cm_record_key(uint64_t src, uint64_t ks, uint32_t run, uint64_t idx) {
  const uint64_t ulen = ks - 8;
  CmRec rec;
  uint64_t trailer;
  if (ks >= 16) {
    const kv_u128 x = tb_load16(src) & tb_mask(static_cast<uint32_t>(ulen < 16 ? ulen : 16));
    rec.hi = __builtin_bswap64(static_cast<uint64_t>(x));
    rec.lo = __builtin_bswap64(static_cast<uint64_t>(x >> 64));
    trailer = static_cast<uint64_t>(tb_load16(src + ks - 16) >> 64);
  } else {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(src);
    const RoutePrefix q = route_prefix(p, ulen);
    rec.hi = q.hi;
    rec.lo = q.lo;
    trailer = 0;
    for (uint32_t b = 0; b < 8; b++) trailer |= static_cast<uint64_t>(p[ulen + b]) << (8 * b);
  }
  rec.inv = ~trailer;
  rec.ref = idx | (static_cast<uint64_t>(run) << 32) | ((ulen < 17 ? ulen : 17) << 40);
  return rec;
}

// Pair idx of run `run` (a packed form) as a record; *shortk where its key has
// fewer than 8 bytes (then nothing of the key is read).
DLSM_HD CmRec cm_record(const CmRun& r, uint32_t run, uint64_t idx, bool* shortk) {
  const uint64_t ks = r.key_size(idx);
  *shortk = ks < 8;
  if (ks < 8) return CmRec{0, 0, 0, 0};
  return cm_record_key(r.key_src(idx), ks, run, idx);
}

// Slice::compare of the two records' user keys, read through the references
// (in the descriptor form: one 16-byte load per key, then the bytes).
template <bool D = false>
DLSM_HD int cm_user_compare(const CmRec& a, const CmRec& b, const CmRun* runs) {
  const CmRun &ra = runs[cm_run(a)], &rb = runs[cm_run(b)];
  if (D) {
    const CmDesc da = ra.desc[cm_index(a)], db = rb.desc[cm_index(b)];
    return route_compare(reinterpret_cast<const uint8_t*>(da.addr + 8), da.key_size - 8,
                         reinterpret_cast<const uint8_t*>(db.addr + 8), db.key_size - 8);
  }
  return route_compare(reinterpret_cast<const uint8_t*>(ra.key_src(cm_index(a))), ra.key_size(cm_index(a)) - 8,
                       reinterpret_cast<const uint8_t*>(rb.key_src(cm_index(b))), rb.key_size(cm_index(b)) - 8);
}

// The user keys' order as far as the records alone decide it (the file
// comment's first two lines); kCmNeedsBytes where both keys are longer than 16
// bytes and share their first 16.
constexpr int kCmNeedsBytes = 2;
DLSM_HD int cm_prefix_cmp(const CmRec& a, const CmRec& b) {
  if (a.hi != b.hi) return a.hi < b.hi ? -1 : 1;
  if (a.lo != b.lo) return a.lo < b.lo ? -1 : 1;
  const uint32_t ca = cm_class(a), cb = cm_class(b);
  if (ca <= 16 || cb <= 16) return ca < cb ? -1 : (ca > cb ? 1 : 0);
  return kCmNeedsBytes;
}

// The user keys' order alone (the file comment's first three lines).
template <bool D = false>
DLSM_HD int cm_user_cmp(const CmRec& a, const CmRec& b, const CmRun* runs) {
  const int c = cm_prefix_cmp(a, b);
  return c != kCmNeedsBytes ? c : cm_user_compare<D>(a, b, runs);
}

// InternalKeyComparator::Compare: < 0, 0, > 0.
template <bool D = false>
DLSM_HD int cm_rec_cmp(const CmRec& a, const CmRec& b, const CmRun* runs) {
  const int c = cm_user_cmp<D>(a, b, runs);
  if (c) return c;
  return a.inv < b.inv ? -1 : (a.inv > b.inv ? 1 : 0);
}

// Rule (A) at a merged position: cur is dropped iff it parses, its
// predecessor in merged order parses and has the same user key, and the
// predecessor's sequence is at or below the snapshot (last_sequence_for_key).
template <bool D = false>
DLSM_HD bool cm_hidden(const CmRec& prev, const CmRec& cur, uint64_t snapshot, const CmRun* runs) {
  const uint64_t tp = cm_trailer(prev), tc = cm_trailer(cur);
  if ((tc & 0xffu) > 1 || (tp & 0xffu) > 1 || (tp >> 8) > snapshot) return false;
  return cm_user_cmp<D>(prev, cur, runs) == 0;
}

// Merge path: how many of the first diag outputs of A (na records) merged with
// B (nb records) come from A, A winning ties (diag <= na + nb).
template <bool D = false, class PA, class PB>
DLSM_HD uint32_t cm_path_split(PA A, uint32_t na, PB B, uint32_t nb, uint32_t diag, const CmRun* runs) {
  uint32_t lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (cm_rec_cmp<D>(B[diag - 1 - mid], A[mid], runs) < 0) hi = mid;  // B's record leaves before A[mid]
    else lo = mid + 1;
  }
  return lo;
}

// A lane's share of a tile: outputs [d0, d0 + count) of A merged with B, count
// <= kCmLane, into out[0, count).
template <bool D = false, class PA, class PB>
DLSM_HD void cm_merge_lane(PA A, uint32_t na, PB B, uint32_t nb, uint32_t d0, uint32_t count, CmRec* out,
                           const CmRun* runs) {
  uint32_t i = cm_path_split<D>(A, na, B, nb, d0, runs), j = d0 - i;
#pragma unroll
  for (uint32_t k = 0; k < kCmLane; k++) {
    if (k < count) {  // (no break: the loop unrolls and out[] stays in registers)
      const bool from_b = j < nb && (i >= na || cm_rec_cmp<D>(B[j], A[i], runs) < 0);
      const CmRec& x = from_b ? B[j] : A[i];
      out[k].hi = x.hi;  // (field by field: a struct copy through the select keeps out[] in memory)
      out[k].lo = x.lo;
      out[k].inv = x.inv;
      out[k].ref = x.ref;
      j += from_b ? 1 : 0;
      i += from_b ? 0 : 1;
    }
  }
}

}  // namespace dlsm
