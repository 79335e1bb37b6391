// dlsm_amd/csrc/range_scan.h -- the rules of a range scan over opened tables:
// what DBIter (db/db_iter.cc:141-212, 283-298) yields over a MergingIterator
// (table/merger.cc) of the runs after Seek(start) and a row of Next() calls.
// Shared by the planner (host_plan.h) and the host form (bloom_capi.hip); DLSM_HD,
// so a kernel can share it too.  Plain integer code: no device call.  Nothing
// here is compiled from the reference: a restatement of the lines cited.
//
// A run is one level-0 file or a deeper level's files in key order
// (table_scan.h); its entries are its files' index entries in the order listed,
// and a cursor names one of them by (listed file, entry).  A scan
//   seeks every run to its first entry >= start || Fixed64(snapshot << 8 | 1)
//     (rs_seek_run: the run's files searched by their last entries, then the
//     window search of index_seek.h inside the file);
//   walks the runs' entries in InternalKeyComparator order, equal internal keys
//     in ascending run (rs_before over 32-byte records, compaction_merge.h's
//     form);
//   passes over an entry whose sequence is above the snapshot, and one whose
//     type byte is above 1 (ParseKey fails; kRsBadType);
//   lets the first remaining entry of a user key decide the key -- type 1 yields
//     the pair, type 0 nothing -- and hides every later entry of it (the last
//     visible entry is carried from step to step);
//   stops at `limit` yielded pairs or when every run is exhausted.
// A yielded entry becomes its handle and, through table_scan.h's rules for one
// pair, a 16-byte descriptor of the pair's bytes (rs_yield); a pair that fails
// them sets kRsTableMismatch.  No byte outside the index contents and the
// chunks is read: every check comes before the dereference it guards.
#pragma once
#include <stdint.h>

#include "table_scan.h"

namespace dlsm {

constexpr uint32_t kRsMaxLimit = 1024;  // DLSM_SCAN_MAX_LIMIT

enum : uint64_t {  // DLSM_SCAN_* of the public header
  kRsKeysCap = 1,
  kRsValuesCap = 2,
  kRsPairCap = 4,
  kRsBadType = 8,
  kRsTableMismatch = 32,
};

// The call's runs as the scan addresses them: run r's files are listed at
// [first[r], first[r + 1]) of file[], in key order.
struct RsRuns {
  uint32_t first[kCmMaxRuns + 1];
  uint32_t file[kTsMaxFiles + 1];  // the file's number in the tableindex / tabledata
  uint32_t n_runs, reserved;
};

// One file as the scan sees it.
struct RsFile {
  IndexView index;
  KvChunks chunks;
};

struct RsCursor {
  uint32_t k, e;  // listed file, entry in it; k == the run's end: exhausted
};

// The cursor moved on to the entry it names: entries past a file's end count
// on into the next files of the run (files without entries are passed).
// Files: entries(file) and at(file) over the tableindex's numbering.
template <class Files>
DLSM_HD RsCursor rs_settle(const Files& files, const RsRuns& R, uint32_t kend, RsCursor c) {
  while (c.k < kend) {
    const uint32_t n = files.entries(R.file[c.k]);
    if (c.e < n) return c;
    c.e -= n;
    c.k++;
  }
  return RsCursor{kend, 0};
}

// Seek of run r: the first entry >= user || Fixed64(trailer), settled.
template <class Files>
DLSM_HD RsCursor rs_seek_run(const Files& files, const RsRuns& R, uint32_t r, const uint8_t* user, uint32_t un,
                             uint64_t trailer) {
  const uint32_t kend = R.first[r + 1];
  uint32_t lo = R.first[r], hi = kend;  // files below lo end below the target, files from hi on do not
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    uint32_t m = mid;
    while (m < hi && files.entries(R.file[m]) == 0) m++;
    if (m == hi) {
      hi = mid;
      continue;
    }
    const RsFile f = files.at(R.file[m]);
    IndexEntry e;
    const bool below = index_decode(f.index, index_restart(f.index, f.index.n - 1), &e) && e.key_len >= 8 &&
                       index_compare_target(f.index.data + e.key, e.key_len, user, un, trailer) < 0;
    if (below) lo = m + 1;
    else hi = m;
  }
  RsCursor c = rs_settle(files, R, kend, RsCursor{lo, 0});
  if (c.k == kend) return c;
  const RsFile f = files.at(R.file[c.k]);
  c.e = index_window_search(f.index, 0, f.index.n, user, un, trailer);
  return rs_settle(files, R, kend, c);
}

// Entry e (< f.index.n) as a record; *key / *klen its internal key in the
// index contents.  false where the entry does not decode (never in an opened
// block): the run ends there.
DLSM_HD bool rs_record(const RsFile& f, uint32_t e, uint32_t run, CmRec* rec, const uint8_t** key, uint32_t* klen) {
  IndexEntry x;
  if (!index_decode(f.index, index_restart(f.index, e), &x) || x.shared != 0 || x.key_len < 8) return false;
  *key = f.index.data + x.key;
  *klen = x.key_len;
  *rec = cm_record_key(reinterpret_cast<uint64_t>(*key), x.key_len, run, e);
  return true;
}

// The user keys' order; the key bytes are read only on kCmNeedsBytes.
DLSM_HD int rs_user_cmp(const CmRec& a, const uint8_t* ak, uint32_t an, const CmRec& b, const uint8_t* bk,
                        uint32_t bn) {
  const int c = cm_prefix_cmp(a, b);
  return c != kCmNeedsBytes ? c : route_compare(ak, an - 8, bk, bn - 8);
}

// The merged order of the runs' heads: InternalKeyComparator, then the run.
DLSM_HD bool rs_before(const CmRec& a, const uint8_t* ak, uint32_t an, const CmRec& b, const uint8_t* bk,
                       uint32_t bn) {
  const int c = rs_user_cmp(a, ak, an, b, bk, bn);
  if (c) return c < 0;
  if (a.inv != b.inv) return a.inv < b.inv;
  return cm_run(a) < cm_run(b);
}

// An entry under the snapshot: visible where it parses and is no newer.
DLSM_HD bool rs_bad_type(const CmRec& r) { return (cm_trailer(r) & 0xffu) > 1; }
DLSM_HD bool rs_visible(const CmRec& r, uint64_t snapshot) {
  const uint64_t t = cm_trailer(r);
  return (t & 0xffu) <= 1 && (t >> 8) <= snapshot;
}
DLSM_HD bool rs_is_value(const CmRec& r) { return (cm_trailer(r) & 0xffu) == 1; }

// A yielded entry: its handle as the index entry gives it, and the pair's
// descriptor where table_scan.h's rules for one pair hold (false: mismatch).
DLSM_HD bool rs_yield(const RsFile& f, uint32_t file, uint32_t e, KvHandle* h, CmDesc* d) {
  IndexEntry x;
  uint64_t off = 0, size = 0;
  if (index_decode(f.index, index_restart(f.index, e), &x)) (void)index_handle(f.index, x, &off, &size);
  h->offset = off;
  h->size = static_cast<uint32_t>(size);
  h->file = file;
  *d = CmDesc{0, 0, 0};
  TsPair p;
  if (!ts_pair(TsFile{f.index, f.chunks}, e, &p)) return false;
  if (index_compare_bytes(p.p + 8, p.key_size, f.index.data + p.ekey, p.key_size) != 0) return false;
  d->addr = reinterpret_cast<uint64_t>(p.p);
  d->key_size = p.key_size;
  d->value_size = p.value_size;
  return true;
}

// What a scan leaves besides its handles and descriptors.
struct RsResult {
  uint32_t count;  // pairs yielded
  uint64_t flags;  // kRsBadType, kRsTableMismatch
};

// One scan, entry by entry: the host form.  handle / desc: `limit` slots; the
// first `count` are written.
template <class Files>
DLSM_HD RsResult rs_scan_one(const Files& files, const RsRuns& R, const uint8_t* user, uint32_t un, uint64_t snapshot,
                             uint32_t limit, KvHandle* handle, CmDesc* desc) {
  RsCursor cur[kCmMaxRuns];
  CmRec rec[kCmMaxRuns];
  const uint8_t* key[kCmMaxRuns];
  uint32_t klen[kCmMaxRuns];
  auto load = [&](uint32_t r) {
    const uint32_t kend = R.first[r + 1];
    if (cur[r].k < kend && !rs_record(files.at(R.file[cur[r].k]), cur[r].e, r, &rec[r], &key[r], &klen[r]))
      cur[r] = RsCursor{kend, 0};
  };
  for (uint32_t r = 0; r < R.n_runs; r++) {
    cur[r] = rs_seek_run(files, R, r, user, un, index_seek_trailer(snapshot));
    load(r);
  }
  RsResult out{0, 0};
  bool seen = false;
  CmRec seen_rec{};
  const uint8_t* seen_key = nullptr;
  uint32_t seen_len = 0;
  while (out.count < limit) {
    uint32_t best = kCmMaxRuns;
    for (uint32_t r = 0; r < R.n_runs; r++) {
      if (cur[r].k == R.first[r + 1]) continue;
      if (best == kCmMaxRuns || rs_before(rec[r], key[r], klen[r], rec[best], key[best], klen[best])) best = r;
    }
    if (best == kCmMaxRuns) break;
    const CmRec& x = rec[best];
    if (rs_bad_type(x)) out.flags |= kRsBadType;
    if (rs_visible(x, snapshot)) {
      const bool first = !seen || rs_user_cmp(seen_rec, seen_key, seen_len, x, key[best], klen[best]) != 0;
      seen = true;
      seen_rec = x;
      seen_key = key[best];
      seen_len = klen[best];
      if (first && rs_is_value(x)) {
        const uint32_t file = R.file[cur[best].k];
        if (!rs_yield(files.at(file), file, cur[best].e, &handle[out.count], &desc[out.count]))
          out.flags |= kRsTableMismatch;
        out.count++;
      }
    }
    cur[best] = rs_settle(files, R, R.first[best + 1], RsCursor{cur[best].k, cur[best].e + 1});
    load(best);
  }
  return out;
}

}  // namespace dlsm
