// dlsm_amd/csrc/table_scan.h -- a compaction input read out of opened tables:
// what ByteAddressableSEQIterator (table/byte_addressable_SEQ_iterrator.cpp:
// 48-184) hands to the merging iterator for one file -- the index iterator gives
// the first pair's offset, from there the pairs are walked back to back through
// the chunks by their two Fixed32 lengths -- and how MakeInputIterator
// (db/version_set.cc:1565-1596) strings files into runs: a level-0 file is a
// run of its own, a deeper level's files in key order are one run.  Shared by
// the kernel (table_scan.hip), the planner (host_plan.h) and the host form
// (bloom_capi.hip).  Plain integer code: no device call.  Nothing here is
// compiled from the reference: a restatement of the lines cited.
//
// The walk is sequential; the scan is not.  Entry i of a file's index block
// names pair i by its BlockHandle {offset, size}, so every pair can be found on
// its own -- provided the handles name the very pairs the walk visits.  That
// is what the rules below establish, entry by entry, each looking at its
// predecessor only:
//   the handle's offset is its predecessor's offset + size (0 for the first);
//   the handle names size >= 16 bytes of one chunk (kv_pair_locate);
//   the pair's Fixed32 key_size is the entry's non_shared;
//   8 + key_size + value_size is the handle's size;
//   the pair's key bytes are the entry's key.
// An entry that breaks one sets kCmTableMismatch.  Every check comes before the
// dereference it guards: locate before the header, the header's sum before the
// key, and nothing is read from a pair that failed.  A pair that passes becomes
// a 16-byte descriptor (compaction_merge.h's third run form) and its 32-byte
// merge record, built from the pair's own key -- the bytes the gather will copy
// -- and is compared with its predecessor in the run, across file boundaries
// too, for the strict ascent every merge pass relies on (kCmUnsorted: two
// files of one level that overlap).
#pragma once
#include <stdint.h>

#include "compaction_merge.h"

namespace dlsm {

constexpr uint32_t kTsMaxFiles = 1023;  // files listed in one call: their bases fit 8 KiB of LDS

// The call's files in the order listed, run by run, as the scan addresses them:
// listed file k holds the inputs [ebase[k], ebase[k + 1]) and belongs to run
// run[k]; slots from n_listed on repeat the total.
struct TsTable {
  uint64_t ebase[kTsMaxFiles + 1];
  uint32_t file[kTsMaxFiles + 1];  // the file's number in the tableindex / tabledata
  uint8_t run[kTsMaxFiles + 1];
  uint32_t n_listed, reserved;
};

// One file: its index block's contents and its data chunks.
struct TsFile {
  IndexView index;
  KvChunks chunks;
};

// A pair that passed every rule short of the key bytes.
struct TsPair {
  const uint8_t* p;  // the pair's header
  uint32_t key_size, value_size;
  uint32_t ekey;     // the entry's key in the index contents
};

// Entry i (< f.index.n) of an opened block: its handle against its
// predecessor's, the pair located, the header against the entry and the handle.
// Reads the two entries and, once located, the pair's 8 header bytes.
DLSM_HD bool ts_pair(const TsFile& f, uint32_t i, TsPair* o) {
  const IndexView& v = f.index;
  IndexEntry e;
  if (!index_decode(v, index_restart(v, i), &e) || e.shared != 0 || e.key_len < 8) return false;
  uint64_t off, size, next = 0;
  if (!index_handle(v, e, &off, &size) || size > 0xffffffffull) return false;
  if (i > 0) {
    IndexEntry q;
    uint64_t po, ps;
    if (!index_decode(v, index_restart(v, i - 1), &q) || !index_handle(v, q, &po, &ps)) return false;
    next = po + ps;
  }
  if (off != next) return false;  // the walk would not arrive here
  const uint8_t* p = kv_pair_locate(f.chunks, off, static_cast<uint32_t>(size));
  if (!p) return false;
  const uint32_t ks = index_fixed32(p), vs = index_fixed32(p + 4);
  if (ks != e.key_len || uint64_t(8) + ks + vs != size) return false;
  o->p = p;
  o->key_size = ks;
  o->value_size = vs;
  o->ekey = e.key;
  return true;
}

// cm_rec_cmp of two pairs of this pass, whose descriptors may not be written
// yet: the key bytes come from the pairs themselves.
DLSM_HD int ts_rec_cmp(const CmRec& a, const TsPair& pa, const CmRec& b, const TsPair& pb) {
  int c = cm_prefix_cmp(a, b);
  if (c == kCmNeedsBytes) c = route_compare(pa.p + 8, pa.key_size - 8, pb.p + 8, pb.key_size - 8);
  if (c) return c;
  return a.inv < b.inv ? -1 : (a.inv > b.inv ? 1 : 0);
}

// The per-entry rule: entry i of file f is input idx of run `run`; pf / pi name
// the input before it in the run (has_prev: idx > 0; another file where i == 0).
// Returns the entry's flag bits; *d and *rec are written where the entry itself
// passes.  A predecessor that fails is reported by its own call.
DLSM_HD uint64_t ts_entry(const TsFile& f, uint32_t i, bool has_prev, const TsFile& pf, uint32_t pi, uint32_t run,
                          uint64_t idx, CmDesc* d, CmRec* rec) {
  TsPair cur, prev;
  if (!ts_pair(f, i, &cur)) return kCmTableMismatch;
  if (index_compare_bytes(cur.p + 8, cur.key_size, f.index.data + cur.ekey, cur.key_size) != 0) return kCmTableMismatch;
  d->addr = reinterpret_cast<uint64_t>(cur.p);
  d->key_size = cur.key_size;
  d->value_size = cur.value_size;
  *rec = cm_record_key(d->addr + 8, cur.key_size, run, idx);
  if (!has_prev || !ts_pair(pf, pi, &prev)) return 0;
  const CmRec before = cm_record_key(reinterpret_cast<uint64_t>(prev.p) + 8, prev.key_size, run, idx - 1);
  return ts_rec_cmp(before, prev, *rec, cur) >= 0 ? kCmUnsorted : 0;
}

}  // namespace dlsm
