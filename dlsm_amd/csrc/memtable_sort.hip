// dlsm_amd/csrc/memtable_sort.hip -- one batch of pairs in arrival order into a
// sorted run, what a flush drops dropped, keys and values packed
// (dlsm_memtable_sort_dev): the memtable's job at flush time.  The order, the
// record and the drop rule are compaction_merge.h's, the geometry is
// memtable_sort.h's; this file is the work split.  2 * passes + 4 launches,
// passes = ceil(log2(ceil(n / kMsTile))), ordered by the stream alone: no
// counter is shared between workgroups, nothing looks back, no result depends
// on an atomic.
//
// Tile sort (ms_tile_sort_kernel): a workgroup of kCmTileLanes lanes owns
// kMsTile consecutive input pairs (and, like the record pass it stands in for,
// cpw consecutive tiles one after the other).  A lane builds the records of its
// kCmLane consecutive pairs straight from the keys (cm_record_key: two 16-byte
// loads of a key of 16 bytes or more), sorts them in registers with a fixed
// stable network and writes them to LDS.  log2(kCmTileLanes) rounds follow: in
// round r the tile is sorted segments of kCmLane * 2^r records, a lane takes
// the kCmLane outputs at its own place of the merge of the two neighbouring
// segments it lies in -- a diagonal search in LDS (cm_path_split), a serial
// merge into registers (cm_merge_lane) -- then barrier, write-back, barrier:
// one 32 KiB buffer, the scheme of a merge pass's tile.  The last tile is
// short: a lane past n holds no record and the segments are clipped, nothing is
// padded.  The sorted tile leaves as coalesced 16-byte stores: 32 B written per
// pair, the key's bytes (and 8 or 16 B of offsets) read, no record read from
// HBM.  A tile with a key shorter than 8 bytes is not sorted; the workgroup's
// bit goes to the workspace and the next launch reduces it, as behind the
// merge's record pass.
//
// Global passes: pass p merges neighbouring segments of 2^p tiles, ping-pong
// between the two record arrays.  The partition (one thread per tile, a
// diagonal search in global memory) and the merge (a workgroup per tile) are
// the bodies of merge_pass.h with ms_pair's arithmetic in the place of the
// compaction merge's pair table: 64 B per pair and pass.
//
// Decide, offsets and gather are the compaction merge's own kernels
// (launch_compaction_merge_tail) over the array the last pass wrote, the batch
// being run 0 of the table.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"
#include "memtable_sort.h"
#include "merge_pass.h"
#include "sort_pass.h"

namespace dlsm {
namespace {

__global__ __launch_bounds__(kCmTileLanes) void ms_tile_sort_kernel(CmDev a) {
  __shared__ cm_u32x4 s[2 * kMsTile];
  CmRec* sr = reinterpret_cast<CmRec*>(s);
  const CmRun* runs = a.tab->runs;
  const CmRun run = runs[0];  // (by value: the same for every lane)
  cm_u32x4* out = reinterpret_cast<cm_u32x4*>(a.rec[0]);
  const uint32_t o0 = threadIdx.x * kCmLane;
  int shortk = 0;
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * a.cpw;
  for (uint64_t t = t0; t < t0 + a.cpw; t++) {
    const uint64_t g0 = t * kMsTile;
    if (g0 >= a.n) break;  // (the same for every lane)
    const uint32_t cnt = a.n - g0 < kMsTile ? static_cast<uint32_t>(a.n - g0) : kMsTile;
    const uint32_t c = o0 < cnt ? (cnt - o0 < kCmLane ? cnt - o0 : kCmLane) : 0;
    CmRec o[kCmLane];
    bool sk = false;
#pragma unroll
    for (uint32_t k = 0; k < kCmLane; k++) {
      if (k < c) {
        bool q;
        o[k] = cm_record(run, 0, g0 + o0 + k, &q);
        sk |= q;
      }
    }
    // (the barrier also keeps the tile before, still leaving LDS, from the writes below)
    if (__syncthreads_or(sk)) {
      shortk = 1;
      continue;
    }
    ms_sort_lane(o, c, [&](const CmRec& x, const CmRec& y) { return cm_rec_cmp(x, y, runs) < 0; });
#pragma unroll
    for (uint32_t k = 0; k < kCmLane; k++)
      if (k < c) sr[o0 + k] = o[k];
    __syncthreads();
    for (uint32_t w = kCmLane; w < kMsTile; w <<= 1) {
      // the lane's two segments [base, a1) and [a1, b1), clipped to the tile's records
      const uint32_t base = o0 & ~(2 * w - 1);
      const uint32_t a1 = base + w < cnt ? base + w : cnt, b1 = base + 2 * w < cnt ? base + 2 * w : cnt;
      // (without a right side the lane's records stay where they are, in o[] and in LDS)
      const bool merge = c != 0 && b1 > a1;
      if (merge) cm_merge_lane(sr + base, a1 - base, sr + a1, b1 - a1, o0 - base, c, o, runs);
      __syncthreads();
      if (merge) {
#pragma unroll
        for (uint32_t k = 0; k < kCmLane; k++)
          if (k < c) sr[o0 + k] = o[k];
      }
      __syncthreads();
    }
    for (uint32_t u = threadIdx.x; u < 2 * cnt; u += kCmTileLanes) out[2 * g0 + u] = s[u];
  }
  shortk = __syncthreads_or(shortk);
  if (threadIdx.x == 0) a.wg_flags[blockIdx.x] = shortk ? kCmShortKey : 0;
}

__global__ __launch_bounds__(kCmTileLanes) void ms_partition_kernel(CmDev a, uint32_t pass, uint32_t ntiles) {
  if (cm_input_flags(a, pass == 0)) return;
  const uint32_t t = blockIdx.x * kCmTileLanes + threadIdx.x;
  if (t >= ntiles) return;
  cm_partition_tile<false>(a, pass, ms_pair(a.n, pass, t), t);
}

__global__ __launch_bounds__(kCmTileLanes) void ms_merge_kernel(CmDev a, uint32_t pass) {
  __shared__ cm_u32x4 s[2 * kCmTile];
  if (cm_input_flags(a, false)) return;
  cm_merge_tile<false>(a, pass, ms_pair(a.n, pass, blockIdx.x), blockIdx.x, s);
}

}  // namespace

hipError_t launch_memtable_sort(const CmDev& a, hipEvent_t* ev, hipStream_t s) {
  if (a.nwg == 0 || a.nwg > kSortMaxWgs || a.cpw == 0 || a.copy_wgs == 0 || a.n_runs != 1 || a.n > 0xffffffffull ||
      a.n_passes != ms_passes(a.n) || static_cast<uint64_t>(a.nwg) * a.cpw < ms_tiles(a.n))
    return hipErrorInvalidValue;
  hipError_t e;
  int marks = 0;
  auto mark = [&]() { return ev ? hipEventRecord(ev[marks++], s) : hipSuccess; };
  if ((e = mark()) != hipSuccess) return e;
  ms_tile_sort_kernel<<<a.nwg, kCmTileLanes, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark()) != hipSuccess) return e;
  const uint32_t nt = ms_tiles(a.n);  // (a pass has two tiles or more)
  for (uint32_t p = 0; p < a.n_passes; p++) {
    ms_partition_kernel<<<(nt + kCmTileLanes - 1) / kCmTileLanes, kCmTileLanes, 0, s>>>(a, p, nt);
    if ((e = hipGetLastError()) != hipSuccess || (e = mark()) != hipSuccess) return e;
    ms_merge_kernel<<<nt, kCmTileLanes, 0, s>>>(a, p);
    if ((e = hipGetLastError()) != hipSuccess || (e = mark()) != hipSuccess) return e;
  }
  return launch_compaction_merge_tail(a, ev ? ev + marks : nullptr, s);
}

}  // namespace dlsm
