// dlsm_amd/csrc/merge_pass.h -- one two-way merge-path pass over 32-byte
// records, as the kernels of compaction_merge.hip and memtable_sort.hip run it:
// the partition's search for one tile and the merge of one tile in LDS.  Which
// pair a tile belongs to is the caller's business -- a table lookup in the
// compaction merge (runs of any length), arithmetic in the memtable sort
// (uniform segments).  Device code; the order itself is compaction_merge.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "bloom_internal.h"

namespace dlsm {

typedef uint32_t cm_u32x4 __attribute__((ext_vector_type(4)));

// The first launch's bits, in every thread (called by the whole workgroup).
// The first launch behind the record pass (or the tile sort) -- pass 0's
// partition, or the decide pass where there is no merge pass -- ORs the
// workgroups' words (`reduce`) and its workgroup 0 leaves the result in tot[3];
// every later launch reads that one word.
// A table record pass has kCmTableMismatch where the packed one has
// kCmShortKey.
template <bool D = false>
__device__ __forceinline__ uint64_t cm_input_flags(const CmDev& a, bool reduce) {
  if (!reduce) return a.tot[3];
  constexpr uint64_t kFirst = D ? kCmTableMismatch : kCmShortKey;
  int shortk = 0, unsorted = 0;
  for (uint32_t j = threadIdx.x; j < a.nwg; j += blockDim.x) {
    const uint64_t f = a.wg_flags[j];
    shortk |= (f & kFirst) != 0;
    unsorted |= (f & kCmUnsorted) != 0;
  }
  shortk = __syncthreads_or(shortk);
  unsorted = __syncthreads_or(unsorted);
  const uint64_t flags = (shortk ? kFirst : 0) | (unsorted ? kCmUnsorted : 0);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.tot[3] = flags;
  return flags;
}

// (a select, not an index: indexing the kernel's argument by a run-time value
// would put the whole descriptor into scratch)
__device__ __forceinline__ CmRec* cm_buf(const CmDev& a, uint32_t which) { return which ? a.rec[1] : a.rec[0]; }

// The partition of tile t of pair p: the left segment's share of the outputs in
// front of the tile.
template <bool D>
__device__ __forceinline__ void cm_partition_tile(const CmDev& a, uint32_t pass, const CmPair& p, uint32_t t) {
  const uint32_t na = p.b0 - p.a0, nb = p.b1 - p.b0;
  const uint64_t d = static_cast<uint64_t>(t - p.tile0) * kCmTile;
  const uint32_t diag = d < static_cast<uint64_t>(na) + nb ? static_cast<uint32_t>(d) : na + nb;
  const CmRec* in = cm_buf(a, pass & 1);
  a.split[t] = cm_path_split<D>(in + p.a0, na, in + p.b0, nb, diag, a.tab->runs);
}

// Tile t of pair p, by a workgroup of kCmTileLanes lanes: its two sub-ranges
// staged in s (2 * kCmTile units of LDS), a diagonal search and kCmLane serial
// outputs per lane, the records back to LDS in output order, coalesced 16-byte
// stores.
template <bool D>
__device__ __forceinline__ void cm_merge_tile(const CmDev& a, uint32_t pass, const CmPair& p, uint32_t t, cm_u32x4* s) {
  const uint32_t na_all = p.b0 - p.a0, nb_all = p.b1 - p.b0, len = na_all + nb_all;
  const uint64_t d64 = static_cast<uint64_t>(t - p.tile0) * kCmTile;
  if (d64 >= len) return;
  const uint32_t d0 = static_cast<uint32_t>(d64);
  const uint32_t d1 = len - d0 > kCmTile ? d0 + kCmTile : len;
  const uint32_t a_lo = a.split[t], a_hi = d1 == len ? na_all : a.split[t + 1];
  // (sorted segments give ascending splits; anything else would index outside the tile)
  if (a_lo > d0 || a_hi < a_lo || a_hi > na_all || a_hi > d1 || d1 - a_hi > nb_all || d0 - a_lo > d1 - a_hi) return;
  const uint32_t b_lo = d0 - a_lo, na = a_hi - a_lo, cnt = d1 - d0, nb = cnt - na;
  const cm_u32x4* in = reinterpret_cast<const cm_u32x4*>(cm_buf(a, pass & 1));
  cm_u32x4* out = reinterpret_cast<cm_u32x4*>(cm_buf(a, (pass & 1) ^ 1));
  for (uint32_t u = threadIdx.x; u < 2 * cnt; u += kCmTileLanes) {
    const uint32_t e = u >> 1;
    const uint64_t r = e < na ? static_cast<uint64_t>(p.a0) + a_lo + e : static_cast<uint64_t>(p.b0) + b_lo + (e - na);
    s[u] = in[2 * r + (u & 1)];
  }
  __syncthreads();
  CmRec* sr = reinterpret_cast<CmRec*>(s);
  CmRec o[kCmLane];
  const uint32_t o0 = threadIdx.x * kCmLane;
  const uint32_t c = o0 < cnt ? (cnt - o0 < kCmLane ? cnt - o0 : kCmLane) : 0;
  if (c) cm_merge_lane<D>(sr, na, sr + na, nb, o0, c, o, a.tab->runs);
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < kCmLane; k++)
    if (k < c) sr[o0 + k] = o[k];
  __syncthreads();
  const uint64_t o64 = 2 * (static_cast<uint64_t>(p.a0) + d0);
  for (uint32_t u = threadIdx.x; u < 2 * cnt; u += kCmTileLanes) out[o64 + u] = s[u];
}

}  // namespace dlsm
