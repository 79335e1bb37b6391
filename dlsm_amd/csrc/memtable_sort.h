// dlsm_amd/csrc/memtable_sort.h -- the geometry of the memtable sort
// (dlsm_memtable_sort_dev): n pairs in arrival order into the order of
// InternalKeyComparator::Compare (db/dbformat.cc:41-57), which the memtable's
// skip list (db/memtable.cc) keeps on the host.  The record, the comparator and
// the drop rule are compaction_merge.h's; what is new is how sorted segments
// come to be and how more than kCmMaxRuns of them are paired.  Shared by the
// kernels (memtable_sort.hip) and the planner (host_plan.h).  Plain integer
// code: no device call.
//
// Tile t holds input pairs [t * kMsTile, min((t + 1) * kMsTile, n)); one
// workgroup sorts it in LDS.  Pass p then merges neighbouring sorted segments
// of 2^p tiles, so the pairs of a pass are arithmetic on the tile number and no
// table is read: every segment but the last is whole, every pair's output
// starts at a tile edge, and every pass has ceil(n / kMsTile) tiles.  A record
// with the lower input index sits in the left segment of every merge it meets
// and the left side wins ties, so the sort is stable without an extra key.
#pragma once
#include <stdint.h>

#include "compaction_merge.h"

namespace dlsm {

constexpr uint32_t kMsTile = kCmTile;  // records one workgroup sorts in LDS (32 KiB)
constexpr uint32_t kMsMaxPasses = 22;  // ceil(log2(ceil(UINT32_MAX / kMsTile)))
static_assert(kMsTile == kCmChunk, "the tile sort shares the grid of the decide and offsets passes");
static_assert((kMsTile & (kMsTile - 1)) == 0 && (kCmTileLanes & (kCmTileLanes - 1)) == 0, "the rounds double");
static_assert((0xffffffffull + kMsTile - 1) / kMsTile <= (1ull << kMsMaxPasses), "passes for every n");

DLSM_HD uint32_t ms_tiles(uint64_t n) { return static_cast<uint32_t>((n + kMsTile - 1) / kMsTile); }

// Global passes until one segment holds all n <= UINT32_MAX records.
DLSM_HD uint32_t ms_passes(uint64_t n) {
  uint32_t p = 0;
  while ((static_cast<uint64_t>(kMsTile) << p) < n) p++;
  return p;
}

// The pair of pass `pass` that tile t < ms_tiles(n) belongs to.  In 64 bits:
// a0 + 2^(pass + 1) * kMsTile passes 2^32 near the top of the range.
DLSM_HD CmPair ms_pair(uint64_t n, uint32_t pass, uint32_t t) {
  const uint64_t pair = t >> (pass + 1), w = static_cast<uint64_t>(kMsTile) << pass;
  const uint64_t a0 = pair * 2 * w, b0 = a0 + w, b1 = a0 + 2 * w;
  return CmPair{static_cast<uint32_t>(a0), static_cast<uint32_t>(b0 < n ? b0 : n), static_cast<uint32_t>(b1 < n ? b1 : n),
                static_cast<uint32_t>(pair << (pass + 1))};
}

// A lane's kCmLane records in registers, the first c of them held, into
// ascending order: odd-even transposition, which exchanges neighbours only and
// only where the later one is strictly smaller, so equal records keep their
// input order.
template <class Less>
DLSM_HD void ms_sort_lane(CmRec* r, uint32_t c, Less less) {
  static_assert(kCmLane == 4, "the network is written out for four records");
#pragma unroll
  for (uint32_t round = 0; round < kCmLane; round++) {
#pragma unroll
    for (uint32_t k = round & 1; k + 1 < kCmLane; k += 2) {
      if (k + 1 < c && less(r[k + 1], r[k])) {
        const CmRec x = r[k];
        r[k] = r[k + 1];
        r[k + 1] = x;
      }
    }
  }
}

}  // namespace dlsm
