// dlsm_amd/csrc/sort_pass.h -- one stable counting-sort pass over at most
// kSortBins bins held in LDS: the pass under the read plan (read_plan.hip, one
// digit of the file index per pass) and the shard route (shard_route.hip, the
// shard as the only digit).  Constants, the grid (plain host code, shared with
// the planner in host_plan.h and the CPU tests) and, for the kernels, the pieces
// of the pass.
//
// The items are cut into chunks, cpw chunks per workgroup, so that at most
// kSortMaxWgs workgroups share a (bin, workgroup) table whatever the item count
// is: kSortBins x nwg <= 512 x 512 entries (1 MiB of u32 counts, 2 MiB of u64
// offsets).  Three launches, ordered by the stream alone -- no counter is
// shared between workgroups, nothing inside a launch waits for another
// workgroup:
//   count    workgroup w walks its chunks and writes its count per bin to
//            cnt[bin * nwg + w];
//   scan     one workgroup turns cnt into off[], the first output position of
//            every (bin, workgroup), in that (bin-major, then workgroup) order;
//   scatter  workgroup w walks the same items again and writes each to
//            off[bin * nwg + w] + (its rank among w's items of that bin).
// Ranks follow item order, never the arrival order of atomics: inside a wave by
// ballots over the bin's bits (the lanes with the same bin are the AND over the
// bits of bit ? ballot : ~ballot; the rank is the count of those below), across
// waves by the wave's number (each wave owns a contiguous share of the chunk
// and a row of LDS counts, touched between wave barriers only), across chunks
// and workgroups by the tables.  So a pass is stable, and its result a pure
// function of its input.  Workgroups have kSortBlock threads, two per CU: at
// most kSortMaxWgs of them share the tables, so the waves a CU needs to hide
// the loads have to come from inside a workgroup.
//
// The scatter, per chunk: (A) each wave ranks its share per bin in its own LDS
// row (rank_held, or a count of its own for items that are walked twice), (B)
// between two workgroup barriers thread d turns bin d's wave counts into the
// waves' start positions inside the chunk (the chunk's own start after the
// chunks before is kept in the thread's register), (C) each wave places its
// items (held_pos).  (B) is written out in each scatter kernel: the plan keeps
// counts and starts in two tables, the route in one, and as a shared function
// the loop is unrolled before it is inlined, which changes the route's code.
// The two scans differ (a flat scan against per-bin sums with padding) and stay
// with their kernels.
#pragma once
#include <stdint.h>

namespace dlsm {

constexpr int kSortBlock = 1024;                  // threads per count / scatter workgroup (two per CU)
constexpr int kSortWaves = kSortBlock / 64;
constexpr int kSortBinLg = 9;
constexpr uint32_t kSortBins = 1u << kSortBinLg;  // bins of a pass (LDS)
constexpr uint32_t kSortMaxWgs = 512;             // workgroups per pass: rows of the (bin, workgroup) table
constexpr int kSortScanBlock = 1024;              // the scan's single workgroup
constexpr uint32_t kSortNoItem = 0xffffffffu;     // a held slot without an item

static_assert(kSortBlock == 64 * kSortWaves, "wave64");
static_assert(kSortBins <= kSortBlock, "scatter: thread d < kSortBins owns bin d");
static_assert(static_cast<uint64_t>(kSortBins) * kSortMaxWgs <= 0xffffffffull / 8, "table index in u32");
static_assert(kSortBins % 4 == 0, "a scan may load four counts (16 B) per thread");
static_assert(kSortScanBlock == 1024 && kSortScanBlock / 64 == 16, "scan: sixteen waves");
static_assert(kSortBins <= kSortScanBlock, "scan: thread d < kSortBins owns bin d");

namespace plan {

// The grid of a pass over `items` items in chunks of `chunk`, nwg <= max_wgs.
struct SortGrid {
  uint64_t chunks = 0;
  uint32_t cpw = 1;  // chunks per workgroup
  uint32_t nwg = 0;  // workgroups (the grid); 0: nothing to do
};
inline SortGrid sort_grid(uint64_t items, uint32_t chunk, uint32_t max_wgs) {
  SortGrid g;
  g.chunks = (items + chunk - 1) / chunk;
  const uint64_t cpw = (g.chunks + max_wgs - 1) / max_wgs;
  g.cpw = static_cast<uint32_t>(cpw ? cpw : 1);
  g.nwg = static_cast<uint32_t>((g.chunks + g.cpw - 1) / g.cpw);
  return g;
}

}  // namespace plan

#ifdef __HIPCC__

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
}

// The lanes of `among` (the ballot of the wave's lanes with an item) whose bin
// equals this lane's.  bits: the bins' width, the same in every lane (a
// constant unrolls).
__device__ __forceinline__ uint64_t digit_peers(uint64_t among, uint32_t d, uint32_t bits) {
  uint64_t peers = among;
#pragma unroll
  for (uint32_t b = 0; b < bits; b++) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bb = __ballot(bit);
    peers &= bit ? bb : ~bb;
  }
  return peers;
}

// Count: the first of the peers adds them all to the workgroup's histogram.
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t d, bool active, uint64_t peers) {
  if (active && lanes_below(peers) == 0) atomicAdd(&hist[d], static_cast<uint32_t>(__builtin_popcountll(peers)));
}

// Count: workgroup w's column of the (bin, workgroup) table; indices < bins * nwg.
__device__ __forceinline__ void hist_flush(const uint32_t* hist, uint32_t bins, uint32_t* cnt, uint32_t nwg, uint32_t w,
                                           int tid) {
  for (uint32_t d = tid; d < bins; d += kSortBlock) cnt[d * nwg + w] = hist[d];
}

// The wave's contiguous share [i0, i1) of the chunk of CHUNK items that starts
// at c0 < items.
struct WaveShare {
  uint64_t i0, i1;
};
template <uint32_t CHUNK>
__device__ __forceinline__ WaveShare wave_share(uint64_t c0, int wave, uint64_t items) {
  constexpr uint32_t kWaveItems = CHUNK / kSortWaves;
  const uint64_t i0 = c0 + static_cast<uint64_t>(wave) * kWaveItems;
  return {i0, i0 + kWaveItems < items ? i0 + kWaveItems : items};
}

// Scatter (A), one item per lane, called by the whole wave for each 64 of its
// share in item order (peers: digit_peers of d): ranks the item among the
// share's items of bin d in the wave's row and returns (d, rank) in one
// register for held_pos, kSortNoItem for an inactive lane.  A share has fewer
// than 2^(32 - kSortBinLg) - 1 items.
__device__ __forceinline__ uint32_t rank_held(uint32_t* row, uint32_t d, bool active, uint64_t peers) {
  const uint32_t below = lanes_below(peers);
  const uint32_t loc = active ? row[d] + below : 0;
  __builtin_amdgcn_wave_barrier();
  if (active && below == 0) row[d] = loc + static_cast<uint32_t>(__builtin_popcountll(peers));
  __builtin_amdgcn_wave_barrier();
  return active ? (d | (loc << kSortBinLg)) : kSortNoItem;
}

// Scatter (C): the output position of a held item (row: the wave's row of
// start positions from (B)).
__device__ __forceinline__ uint64_t held_pos(uint32_t held, const uint32_t* row, const uint64_t* start) {
  const uint32_t d = held & (kSortBins - 1u);
  return start[d] + row[d] + (held >> kSortBinLg);
}

#endif  // __HIPCC__

}  // namespace dlsm
