// dlsm_amd/csrc/compaction_merge.hip -- R sorted runs of pairs into one sorted
// run, hidden entries dropped, keys and values packed (dlsm_compaction_merge_dev).
// The order, the record and the drop rule are the DLSM_HD functions of
// compaction_merge.h; this file is the work split.  2 * ceil(log2 R) + 4
// launches ordered by the stream alone: no counter is shared between
// workgroups, nothing looks back, no result depends on an atomic.
//
// Record (cm_record_kernel): one thread per input pair, kCmChunk pairs per
// chunk, a workgroup takes cpw consecutive chunks.  The thread finds its run in
// the bases staged in LDS, builds the pair's 32-byte record (two 16-byte loads
// of the key) and its predecessor's, and compares the two for the strict ascent
// of the run; the workgroup's short-key and unsorted bits go to the workspace.
// The next launch ORs those bits (at most kSortMaxWgs words) into one word;
// every later kernel reads it and does nothing where a bit is set, except that
// the offsets pass writes `merged`.
//
// ceil(log2 R) two-way merge-path passes over the records, ping-pong between
// two arrays; pass p merges neighbouring segments of 2^p runs (CmTable's
// pairs), an unpaired segment is a pair with an empty right side.  Output-
// centric: a pair's output is cut into tiles of kCmTile records whatever the
// two sides hold, so skew cannot unbalance a pass.
//   Partition (cm_partition_kernel): one thread per tile does the diagonal
//   search (cm_path_split) over the two segments in global memory.
//   Merge (cm_merge_kernel): a workgroup stages its tile's two sub-ranges in
//   LDS with 16-byte loads (32 KiB: two workgroups and more share a CU), each
//   lane searches its own diagonal in LDS and merges kCmLane records serially
//   into registers (cm_merge_lane), the records go back to LDS in output order
//   and leave as coalesced 16-byte stores.  Key bytes are read only where two
//   user keys longer than 16 bytes share their first 16.
//
// Decide (cm_decide_kernel): one thread per merged position applies rule (A)
// to records i - 1 and i and leaves the kept pair's key and value lengths
// (0, 0 for a dropped one; a kept key has 8 bytes or more) in the workspace,
// the workgroup's kept pairs and bytes beside them.
//
// Offsets (cm_offsets_kernel): the same grid; the two-level scan of
// tb_offsets_kernel over (kept, key bytes, value bytes): the sums of the
// workgroups below, then a scan per chunk.  Writes key_off / value_off / src
// below the pair cap, and the uncapped offsets and the pairs' source addresses
// for the gather.  Workgroup 0 writes the totals and `merged`.
//
// Gather (cm_gather_kernel): the packed keys, then the packed values, on one
// persistent grid: each stream's bytes below min(total, cap) in spans of
// kCmSpan, a run of spans per workgroup; a window of offsets and sources staged
// in LDS, each lane owns whole 16-byte units (kv_copy_unit: no header, so the
// value read's unit serves), aligned non-temporal stores, no byte read outside
// the input keys and values.
//
// Runs that are files of opened tables (dlsm_compaction_merge_tables_dev) take
// the same launches with table_scan.hip's record pass in the first one's place:
// every kernel that reads a pair through its run is instantiated per run form
// (D: the descriptor form), so the packed forms' kernels are the ones they were.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"
#include "merge_pass.h"
#include "sort_pass.h"
#include "wg_scan.h"

namespace dlsm {
namespace {

constexpr int kCmBlock = 1024;  // threads of the record, decide, offsets and gather kernels
constexpr int kCmWaves = kCmBlock / 64;
static_assert(kCmChunk == kCmBlock, "a thread per pair of a chunk");
static_assert(kCmWindow + 1 == kCmBlock, "a thread stages one offset of the window");
static_assert(kCmSpan % (16 * kCmBlock) == 0, "every lane owns the same number of units of a span");
static_assert(kCmMaxRuns + 1 <= kCmBlock, "a thread stages one base");
constexpr int kCmUnits = kCmSpan / (16 * kCmBlock);  // units per lane and span

struct CmAt {
  const uint64_t* p;
  __device__ uint64_t at(uint64_t i) const { return p[i]; }
};

// The exclusive scans of v[0..3) over the workgroup, in place; all[q]: the
// sums.  The waves' totals are scanned by the first wave, so a thread reads two
// words per scan instead of sixteen (three scans of sixteen spilled).
__device__ __forceinline__ void block_scan3(uint64_t* v, uint64_t (*sh)[kCmWaves + 1], uint64_t* all) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t inc[3];
#pragma unroll
  for (int q = 0; q < 3; q++) {
    inc[q] = v[q];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t up = __shfl_up(inc[q], d, 64);
      inc[q] += lane >= static_cast<uint32_t>(d) ? up : 0;
    }
  }
  __syncthreads();  // sh may still be read from the call before
  if (lane == 63)
    for (int q = 0; q < 3; q++) sh[q][wave] = inc[q];
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const uint64_t t = lane < kCmWaves ? sh[q][lane] : 0;
      uint64_t s = t;
#pragma unroll
      for (int d = 1; d < kCmWaves; d <<= 1) {
        const uint64_t up = __shfl_up(s, d, 64);
        s += lane >= static_cast<uint32_t>(d) ? up : 0;
      }
      if (lane < kCmWaves) sh[q][lane] = s - t;
      if (lane == kCmWaves - 1) sh[q][kCmWaves] = s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 3; q++) {
    v[q] = sh[q][wave] + inc[q] - v[q];
    all[q] = sh[q][kCmWaves];
  }
}

__device__ __forceinline__ void cm_store_rec(CmRec* dst, const CmRec& r) {
  cm_u32x4* d = reinterpret_cast<cm_u32x4*>(dst);
  d[0] = cm_u32x4{static_cast<uint32_t>(r.hi), static_cast<uint32_t>(r.hi >> 32), static_cast<uint32_t>(r.lo),
                  static_cast<uint32_t>(r.lo >> 32)};
  d[1] = cm_u32x4{static_cast<uint32_t>(r.inv), static_cast<uint32_t>(r.inv >> 32), static_cast<uint32_t>(r.ref),
                  static_cast<uint32_t>(r.ref >> 32)};
}

__global__ __launch_bounds__(kCmBlock) void cm_record_kernel(CmDev a) {
  __shared__ uint64_t sbase[kCmMaxRuns + 1];
  if (threadIdx.x <= a.n_runs) sbase[threadIdx.x] = a.tab->base[threadIdx.x];
  __syncthreads();
  const CmRun* runs = a.tab->runs;
  const CmAt base{sbase};
  int shortk = 0, unsorted = 0;
  const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    const uint64_t g = c * kCmChunk + threadIdx.x;
    if (g >= a.n) break;
    const uint32_t r = static_cast<uint32_t>(tb_last_le(base, a.n_runs, g));  // base[0] = 0 <= g < base[n_runs]
    const uint64_t idx = g - sbase[r];
    bool sk, sp;
    const CmRec cur = cm_record(runs[r], r, idx, &sk);
    shortk |= sk;
    if (!sk && idx > 0) {
      const CmRec prev = cm_record(runs[r], r, idx - 1, &sp);
      unsorted |= !sp && cm_rec_cmp(prev, cur, runs) >= 0;
    }
    cm_store_rec(a.rec[0] + g, cur);
  }
  shortk = __syncthreads_or(shortk);
  unsorted = __syncthreads_or(unsorted);
  if (threadIdx.x == 0) a.wg_flags[blockIdx.x] = (shortk ? kCmShortKey : 0) | (unsorted ? kCmUnsorted : 0);
}

// The pair of pass `pass` that tile t belongs to: the last one that starts at
// or before it (a pair without records has no tile).
__device__ __forceinline__ CmPair cm_pair_of(const CmTable* tab, uint32_t pass, uint32_t t) {
  const uint32_t p0 = tab->pair0[pass], p1 = tab->pair0[pass + 1];
  uint32_t k = p0;
  for (uint32_t q = p0 + 1; q < p1; q++) k = tab->pairs[q].tile0 <= t ? q : k;
  return tab->pairs[k];
}

template <bool D>
__global__ __launch_bounds__(kCmTileLanes) void cm_partition_kernel(CmDev a, uint32_t pass, uint32_t ntiles) {
  if (cm_input_flags<D>(a, pass == 0)) return;
  const uint32_t t = blockIdx.x * kCmTileLanes + threadIdx.x;
  if (t >= ntiles) return;
  cm_partition_tile<D>(a, pass, cm_pair_of(a.tab, pass, t), t);
}

template <bool D>
__global__ __launch_bounds__(kCmTileLanes) void cm_merge_kernel(CmDev a, uint32_t pass) {
  __shared__ cm_u32x4 s[2 * kCmTile];
  if (cm_input_flags(a, false)) return;
  cm_merge_tile<D>(a, pass, cm_pair_of(a.tab, pass, blockIdx.x), blockIdx.x, s);
}

// The four u64[n] arrays in the record buffer the last pass did not write.
struct CmScratch {
  uint64_t *klen, *vlen, *ksrc, *vsrc;
};
__device__ __forceinline__ CmScratch cm_scratch(const CmDev& a) {
  uint64_t* p = reinterpret_cast<uint64_t*>(cm_buf(a, (a.n_passes & 1) ^ 1));
  return {p, p + a.n, p + 2 * a.n, p + 3 * a.n};
}

template <bool D>
__global__ __launch_bounds__(kCmBlock) void cm_decide_kernel(CmDev a) {
  __shared__ uint64_t sh[kCmWaves];
  if (cm_input_flags<D>(a, a.n_passes == 0)) return;
  const CmRun* runs = a.tab->runs;
  const CmRec* rec = cm_buf(a, a.n_passes & 1);
  const CmScratch w = cm_scratch(a);
  uint64_t cnt = 0, kb = 0, vb = 0;
  const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    const uint64_t i = c * kCmChunk + threadIdx.x;
    if (i >= a.n) break;
    const CmRec cur = rec[i];
    const bool drop = a.policy != 0 && i > 0 && cm_hidden<D>(rec[i - 1], cur, a.snapshot, runs);
    const CmRun& r = runs[cm_run(cur)];
    uint64_t ks = 0, vs = 0;
    if (D) {  // one load for both lengths
      const CmDesc d = drop ? CmDesc{0, 0, 0} : r.desc[cm_index(cur)];
      ks = d.key_size;
      vs = d.value_size;
    } else {
      ks = drop ? 0 : r.key_size(cm_index(cur));
      vs = drop ? 0 : r.value_size(cm_index(cur));
    }
    w.klen[i] = ks;
    w.vlen[i] = vs;
    cnt += drop ? 0 : 1;
    kb += ks;
    vb += vs;
  }
  cnt = block_sum<kCmWaves>(cnt, sh);
  kb = block_sum<kCmWaves>(kb, sh);
  vb = block_sum<kCmWaves>(vb, sh);
  if (threadIdx.x == 0) {
    a.wg_cnt[blockIdx.x] = cnt;
    a.wg_kb[blockIdx.x] = kb;
    a.wg_vb[blockIdx.x] = vb;
  }
}

template <bool D>
__global__ __launch_bounds__(kCmBlock) void cm_offsets_kernel(CmDev a) {
  __shared__ uint64_t sh[kCmWaves];
  __shared__ uint64_t sh3[3][kCmWaves + 1];
  const uint64_t bad = cm_input_flags(a, false);
  if (bad) {  // only n_in and the flags are specified
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      a.merged[0] = a.n;
      a.merged[1] = a.merged[2] = a.merged[3] = 0;
      a.merged[4] = bad;
    }
    return;
  }
  uint64_t rc = 0, rk = 0, rv = 0;
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += kCmBlock) {
    rc += a.wg_cnt[j];
    rk += a.wg_kb[j];
    rv += a.wg_vb[j];
  }
  rc = block_sum<kCmWaves>(rc, sh);
  rk = block_sum<kCmWaves>(rk, sh);
  rv = block_sum<kCmWaves>(rv, sh);
  if (blockIdx.x == 0) {
    uint64_t tc = 0, tk = 0, tv = 0;
    for (uint32_t j = threadIdx.x; j < a.nwg; j += kCmBlock) {
      tc += a.wg_cnt[j];
      tk += a.wg_kb[j];
      tv += a.wg_vb[j];
    }
    tc = block_sum<kCmWaves>(tc, sh);
    tk = block_sum<kCmWaves>(tk, sh);
    tv = block_sum<kCmWaves>(tv, sh);
    if (threadIdx.x == 0) {
      a.wko[tc] = tk;
      a.wvo[tc] = tv;
      if (tc <= a.pair_cap) {
        a.key_off[tc] = tk;
        a.value_off[tc] = tv;
      }
      a.tot[0] = tc;
      a.tot[1] = tk;
      a.tot[2] = tv;
      a.merged[0] = a.n;
      a.merged[1] = tc;
      a.merged[2] = tk;
      a.merged[3] = tv;
      a.merged[4] = (tk > a.keys_cap ? kCmKeysCap : 0) | (tv > a.values_cap ? kCmValuesCap : 0) |
                    (tc > a.pair_cap ? kCmPairCap : 0);
    }
  }
  const CmRun* runs = a.tab->runs;
  const CmRec* rec = cm_buf(a, a.n_passes & 1);
  const CmScratch w = cm_scratch(a);
  const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    if (c * kCmChunk >= a.n) break;  // (the same for every thread)
    const uint64_t i = c * kCmChunk + threadIdx.x;
    const uint64_t ks = i < a.n ? w.klen[i] : 0;
    const bool keep = ks != 0;
    const uint64_t vs = keep ? w.vlen[i] : 0;
    uint64_t at[3] = {keep ? 1u : 0u, ks, vs}, all[3];
    block_scan3(at, sh3, all);
    const uint64_t j = rc + at[0], ko = rk + at[1], vo = rv + at[2];
    if (keep) {
      const CmRec cur = rec[i];
      const CmRun& r = runs[cm_run(cur)];
      a.wko[j] = ko;
      a.wvo[j] = vo;
      if (D) {  // the key lies behind the pair's header, the value behind the key
        const CmDesc d = r.desc[cm_index(cur)];
        w.ksrc[j] = d.addr + 8;
        w.vsrc[j] = d.addr + 8 + d.key_size;
      } else {
        w.ksrc[j] = r.key_src(cm_index(cur));
        w.vsrc[j] = r.value_src(cm_index(cur));
      }
      if (j <= a.pair_cap) {
        a.key_off[j] = ko;
        a.value_off[j] = vo;
      }
      if (a.src && j < a.pair_cap) a.src[j] = cm_src(cur);
    }
    rc += all[0];
    rk += all[1];
    rv += all[2];
  }
}

__device__ __forceinline__ void cm_copy_span(const uint64_t* off, const uint64_t* src, uint64_t n, uint64_t p0,
                                             uint64_t p1, uint8_t* __restrict__ out) {
#pragma unroll
  for (int k = 0; k < kCmUnits; k++) {
    const uint64_t u = p0 + (static_cast<uint64_t>(k) * kCmBlock + threadIdx.x) * 16;
    if (u < p1) kv_copy_unit(off, src, n, u, p1, out);
  }
}

// One stream of the gather: item j's bytes [off[j], off[j + 1]) come from
// src[j] (m >= 1 items, off[0] = 0); the bytes below limit <= off[m] are
// written.  Called by the whole workgroup.
__device__ __forceinline__ void cm_gather_stream(const uint64_t* off, const uint64_t* src, uint64_t m, uint64_t limit,
                                                 uint8_t* __restrict__ out, uint64_t* soff, uint64_t* ssrc) {
  const uint64_t spans = (limit + kCmSpan - 1) / kCmSpan;
  const uint64_t per = (spans + gridDim.x - 1) / gridDim.x;
  const uint64_t s0 = per * blockIdx.x;
  const uint64_t s1 = s0 + per < spans ? s0 + per : spans;
  if (s0 >= s1) return;
  // p < limit <= off[m] for every byte p served here
  uint64_t first = kv_last_le(off, m, s0 * kCmSpan);
  for (uint64_t s = s0; s < s1; s++) {
    const uint64_t p0 = s * kCmSpan;
    const uint64_t p1 = p0 + kCmSpan < limit ? p0 + kCmSpan : limit;
    const uint64_t idx = first + threadIdx.x;
    const uint64_t o = idx <= m ? off[idx] : ~uint64_t(0);
    soff[threadIdx.x] = o;
    if (idx < m && o < p1) ssrc[threadIdx.x] = src[idx];
    __syncthreads();
    const uint64_t last = soff[kCmWindow];
    if (last >= p1) cm_copy_span(soff, ssrc, kCmWindow, p0, p1, out);
    else cm_copy_span(off + first, src + first, m - first, p0, p1, out);
    if (s + 1 < s1)  // p1 < limit: the next span's first item
      first = last > p1 ? first + kv_last_le(soff, kCmWindow, p1) : first + kv_last_le(off + first, m - first, p1);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kCmBlock) void cm_gather_kernel(CmDev a) {
  __shared__ uint64_t soff[kCmWindow + 1];
  __shared__ uint64_t ssrc[kCmWindow + 1];
  if (cm_input_flags(a, false)) return;
  const uint64_t m = a.tot[0];
  if (m == 0) return;
  const CmScratch w = cm_scratch(a);
  const uint64_t kb = a.tot[1], vb = a.tot[2];
  cm_gather_stream(a.wko, w.ksrc, m, kb < a.keys_cap ? kb : a.keys_cap, a.keys, soff, ssrc);
  cm_gather_stream(a.wvo, w.vsrc, m, vb < a.values_cap ? vb : a.values_cap, a.values, soff, ssrc);
}

// Decide, offsets and gather over the records the last pass wrote; ev: an event
// behind each of the three, or nullptr.
template <bool D>
hipError_t cm_launch_tail(const CmDev& a, hipEvent_t* ev, hipStream_t s) {
  hipError_t e;
  int marks = 0;
  auto mark = [&]() { return ev ? hipEventRecord(ev[marks++], s) : hipSuccess; };
  cm_decide_kernel<D><<<a.nwg, kCmBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark()) != hipSuccess) return e;
  cm_offsets_kernel<D><<<a.nwg, kCmBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark()) != hipSuccess) return e;
  cm_gather_kernel<<<a.copy_wgs, kCmBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return mark();
}

template <bool D>
hipError_t cm_launch(const CmDev& a, const uint32_t* tiles, hipEvent_t* ev, hipStream_t s, const TsDev* ts) {
  hipError_t e;
  int marks = 0;
  auto mark = [&]() { return ev ? hipEventRecord(ev[marks++], s) : hipSuccess; };
  if ((e = mark()) != hipSuccess) return e;
  if (D) {
    if ((e = launch_table_record(a, *ts, s)) != hipSuccess) return e;
  } else {
    cm_record_kernel<<<a.nwg, kCmBlock, 0, s>>>(a);
  }
  if ((e = hipGetLastError()) != hipSuccess || (e = mark()) != hipSuccess) return e;
  for (uint32_t p = 0; p < a.n_passes; p++) {
    // (a pass without a tile still launches: the launch count depends on n_runs alone)
    const uint32_t nt = tiles[p] ? tiles[p] : 1;
    cm_partition_kernel<D><<<(nt + kCmTileLanes - 1) / kCmTileLanes, kCmTileLanes, 0, s>>>(a, p, tiles[p]);
    if ((e = hipGetLastError()) != hipSuccess || (e = mark()) != hipSuccess) return e;
    cm_merge_kernel<D><<<nt, kCmTileLanes, 0, s>>>(a, p);
    if ((e = hipGetLastError()) != hipSuccess || (e = mark()) != hipSuccess) return e;
  }
  return cm_launch_tail<D>(a, ev ? ev + marks : nullptr, s);
}

}  // namespace

hipError_t launch_compaction_merge_tail(const CmDev& a, hipEvent_t* ev, hipStream_t s) {
  return cm_launch_tail<false>(a, ev, s);
}

hipError_t launch_compaction_merge(const CmDev& a, const uint32_t* tiles, hipEvent_t* ev, hipStream_t s,
                                   const TsDev* ts) {
  if (a.nwg == 0 || a.nwg > kSortMaxWgs || a.cpw == 0 || a.copy_wgs == 0 || a.n_runs == 0 || a.n_runs > kCmMaxRuns ||
      a.n_passes > kCmMaxPasses)
    return hipErrorInvalidValue;
  return ts ? cm_launch<true>(a, tiles, ev, s, ts) : cm_launch<false>(a, tiles, ev, s, nullptr);
}

}  // namespace dlsm
