// dlsm_amd/csrc/table_build.hip -- the data region and the index block of a
// table from its pairs (dlsm_table_build_dev).  The format's rules are the
// DLSM_HD functions of table_build.h; this file is the work split.  Four
// launches ordered by the stream alone (the seal's two crc launches follow in
// bloom_capi.hip): no counter is shared between workgroups and nothing looks
// back.
//
// Size (tb_size_kernel): one thread per pair, kTbChunk pairs per chunk, a
// workgroup takes cpw consecutive chunks; the workgroup's sum of pair sizes and
// its malformed-input bits go to the workspace.
//
// Offsets (tb_offsets_kernel): the same grid.  A workgroup sums the sums of the
// workgroups below it, scans its chunks' pair sizes into off[], and -- an
// entry's length needs only its own pair's offset -- scans the entry lengths of
// the same chunk in the same pass: the entry starts relative to the workgroup
// and the workgroup's entry bytes go to the workspace.  Workgroup 0 also adds up
// the total and the bits.
//
// Region (tb_region_kernel), three kinds of workgroup in one launch, none of
// which waits for another:
//   0            adds up the entry bytes, walks the chunk chain and writes
//                `built`: one wave, a 64-ary search of off[] per hop (three
//                dependent loads for a flush's 153,846 pairs), while the others
//                copy.  Its time is linear in the chunk count (about 0.7 us a
//                hop); malformed input is not walked;
//   1 .. nwg     add the entry bytes of the workgroups below to the relative
//                entry starts: es[] (u32, the restart array's values);
//   the rest     the region write, output-centric so skewed value lengths cannot
//                unbalance it: the bytes below min(total, data_cap) are cut into
//                spans of kTbSpan bytes, a persistent grid takes a run of spans
//                per workgroup, stages the next kTbWindow pairs' offsets, key and
//                value addresses and key lengths in LDS, and each lane owns whole
//                16-byte units (tb_region_unit).  A span with more pairs than the
//                window holds has its lanes search off[] where it lies.
//
// Index (tb_index_kernel): the contents below min(total, index_cap) in spans of
// kTbIndexSpan bytes on a persistent grid.  A span's entries (at most 632: an
// entry is 13 bytes or more) are built in an LDS tile: entry j's owner lane
// writes its header and handle varints, then half a wave per entry copies the
// key bytes; the tile leaves as aligned 16-byte units.  Units of the restart
// array come straight from es[] (tb_index_unit).
#include <hip/hip_runtime.h>

#include "bloom_internal.h"
#include "sort_pass.h"
#include "wg_scan.h"

namespace dlsm {
namespace {

constexpr int kTbBlock = 1024;  // threads of every kernel here
constexpr int kTbWaves = kTbBlock / 64;
static_assert(kTbChunk == kTbBlock, "a thread per pair of a chunk");
static_assert(kTbWindow + 1 == kTbBlock, "a thread stages one offset of the window");
static_assert(kTbSpan % (16 * kTbBlock) == 0, "every lane owns the same number of units of a span");
static_assert(kTbIndexSpan / 16 <= kTbBlock && kTbIndexWindow <= kTbBlock, "a thread per unit and per entry of an index span");
constexpr int kTbUnits = kTbSpan / (16 * kTbBlock);  // units per lane and span

__global__ __launch_bounds__(kTbBlock) void tb_size_kernel(TbDev a) {
  __shared__ uint64_t sh[kTbWaves];
  uint64_t sum = 0;
  int shortk = 0, big = 0;
  const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    const uint64_t i = c * kTbChunk + threadIdx.x;
    if (i >= a.n) break;
    const uint64_t ks = a.src.key_size(i), vs = a.src.value_size(i), p = tb_pair_size(ks, vs);
    shortk |= ks < 8;
    big |= ks > 0xffffffffull || vs > 0xffffffffull || p > 0xffffffffull;
    sum += p;
  }
  sum = block_sum<kTbWaves>(sum, sh);
  shortk = __syncthreads_or(shortk);
  big = __syncthreads_or(big);
  if (threadIdx.x == 0) {
    a.wg_sum[blockIdx.x] = sum;
    a.wg_flags[blockIdx.x] = (shortk ? kTbShortKey : 0) | (big ? kTbPairTooBig : 0);
  }
}

__global__ __launch_bounds__(kTbBlock) void tb_offsets_kernel(TbDev a) {
  __shared__ uint64_t sh[kTbWaves];
  uint64_t below = 0;
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += kTbBlock) below += a.wg_sum[j];
  uint64_t run = block_sum<kTbWaves>(below, sh);
  if (blockIdx.x == 0) {
    uint64_t total = 0;
    int shortk = 0, big = 0;
    for (uint32_t j = threadIdx.x; j < a.nwg; j += kTbBlock) {
      total += a.wg_sum[j];
      shortk |= (a.wg_flags[j] & kTbShortKey) != 0;
      big |= (a.wg_flags[j] & kTbPairTooBig) != 0;
    }
    total = block_sum<kTbWaves>(total, sh);
    shortk = __syncthreads_or(shortk);
    big = __syncthreads_or(big);
    if (threadIdx.x == 0) {
      const uint64_t flags = (shortk ? kTbShortKey : 0) | (big ? kTbPairTooBig : 0) | (total > a.data_cap ? kTbDataCap : 0);
      a.off[a.n] = total;
      a.built[0] = total;
      a.tot[3] = flags;
    }
  }
  uint64_t erun = 0;
  const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    if (c * kTbChunk >= a.n) break;  // (the same for every thread)
    const uint64_t i = c * kTbChunk + threadIdx.x;
    const bool in = i < a.n;
    const uint64_t ks = in ? a.src.key_size(i) : 0, p = in ? tb_pair_size(ks, a.src.value_size(i)) : 0;
    uint64_t all, eall;
    const uint64_t o = run + block_scan<uint64_t, kTbWaves>(p, sh, &all);
    const uint64_t e = in ? tb_entry_len(ks, o, p) : 0;
    const uint64_t r = erun + block_scan<uint64_t, kTbWaves>(e, sh, &eall);
    if (in) {
      a.off[i] = o;
      a.erel[i] = r;
    }
    run += all;
    erun += eall;
  }
  if (threadIdx.x == 0) a.wg_esum[blockIdx.x] = erun;
}

// Workgroup 0 of the region launch: the entry bytes, the chunk chain, `built`.
__device__ __forceinline__ void tb_finish(const TbDev& a, uint64_t* sh) {
  uint64_t E = 0;
  for (uint32_t j = threadIdx.x; j < a.nwg; j += kTbBlock) E += a.wg_esum[j];
  E = block_sum<kTbWaves>(E, sh);
  if (threadIdx.x >= 64) return;  // one wave walks the chain
  const bool lane0 = threadIdx.x == 0;
  const uint64_t n = a.n, total = a.built[0];
  const uint64_t* off = a.src.off;
  uint64_t flags = a.tot[3];
  const uint64_t ctot = E + 4 * n + 4;
  if (ctot > 0xffffffffull) flags |= kTbIndexTooBig;
  if (ctot + 5 > a.index_cap) flags |= kTbIndexCap;
  const bool bad = (flags & kTbMalformed) != 0;
  uint64_t nch = 0;
  if (bad) {
    // only `built` is specified: the chain is not walked, no chunk is counted
  } else if (n == 0 || a.chunk_bytes == 0) {
    if (lane0 && a.chunk_cap) a.chunk_end[0] = total;
    nch = 1;
  } else {
    for (uint64_t at = 0; at < n; nch++) {
      const uint64_t lim = tb_chunk_limit(off[at], a.chunk_bytes);
      uint64_t next = at + 1;
      if (off[at + 1] > lim) flags |= kTbOversizePair;
      else next += wave_last_le([&](uint64_t i) { return off[at + 1 + i]; }, n - at, lim);
      if (lane0 && nch < a.chunk_cap) a.chunk_end[nch] = off[next];
      at = next;
    }
  }
  if (nch > a.chunk_cap) flags |= kTbChunkCap;
  if (lane0) {
    a.built[1] = ctot + 5;
    a.built[2] = nch;
    a.built[3] = flags;
    a.tot[0] = E;
    a.tot[1] = (!bad && ctot + 5 <= a.index_cap) ? ctot : 0;  // the seal's length: 0, nothing to seal
    a.es[n] = static_cast<uint32_t>(n);
    a.es[n + 1] = 0;
  }
}

// Workgroups 1 .. nwg: the entry starts of offsets-pass workgroup w.
__device__ __forceinline__ void tb_starts(const TbDev& a, uint32_t w, uint64_t* sh) {
  uint64_t below = 0;
  for (uint32_t j = threadIdx.x; j < w; j += kTbBlock) below += a.wg_esum[j];
  const uint64_t base = block_sum<kTbWaves>(below, sh);
  const uint64_t c0 = static_cast<uint64_t>(w) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    const uint64_t i = c * kTbChunk + threadIdx.x;
    if (i >= a.n) break;
    a.es[i] = static_cast<uint32_t>(base + a.erel[i]);
  }
}

template <class A>
__device__ __forceinline__ void tb_region_span(const A& v, uint64_t n, uint64_t p0, uint64_t p1, uint8_t* __restrict__ out) {
#pragma unroll
  for (int k = 0; k < kTbUnits; k++) {
    const uint64_t u = p0 + (static_cast<uint64_t>(k) * kTbBlock + threadIdx.x) * 16;
    if (u < p1) tb_region_unit(v, n, u, p1, out + u);
  }
}

__global__ __launch_bounds__(kTbBlock) void tb_region_kernel(TbDev a) {
  __shared__ uint64_t sh[kTbWaves];
  __shared__ uint64_t soff[kTbWindow + 1];
  __shared__ uint64_t sks[kTbWindow + 1];
  __shared__ uint64_t svs[kTbWindow + 1];
  __shared__ uint32_t skl[kTbWindow + 1];
  if (blockIdx.x == 0) return tb_finish(a, sh);
  if (blockIdx.x <= a.nwg) return tb_starts(a, blockIdx.x - 1, sh);
  const uint32_t wg = blockIdx.x - 1 - a.nwg;
  const uint64_t n = a.n;
  // (tot[3] holds the bits known before this launch; kTbIndexTooBig is found by
  // workgroup 0 beside us, so with that bit the region is still written -- only
  // `built` is specified then, and the region's writes do not depend on it)
  if (n == 0 || (a.tot[3] & kTbMalformed)) return;
  const uint64_t* off = a.src.off;
  const uint64_t total = off[n];
  const uint64_t limit = total < a.data_cap ? total : a.data_cap;
  const uint64_t spans = (limit + kTbSpan - 1) / kTbSpan;
  const uint64_t per = (spans + a.copy_wgs - 1) / a.copy_wgs;
  const uint64_t s0 = per * wg;
  const uint64_t s1 = s0 + per < spans ? s0 + per : spans;
  if (s0 >= s1) return;
  auto at = [&](uint64_t i) { return off[i]; };
  // p < limit <= off[n] for every byte p served here, and off[0] = 0
  uint64_t first = wave_last_le(at, n, s0 * kTbSpan);
  const TbWindowView win{soff, sks, svs, skl};
  for (uint64_t s = s0; s < s1; s++) {
    const uint64_t p0 = s * kTbSpan;
    const uint64_t p1 = p0 + kTbSpan < limit ? p0 + kTbSpan : limit;
    const uint64_t idx = first + threadIdx.x;
    const uint64_t o = idx <= n ? off[idx] : ~uint64_t(0);
    soff[threadIdx.x] = o;
    if (idx < n && o < p1) {
      sks[threadIdx.x] = a.src.key_src(idx);
      svs[threadIdx.x] = a.src.value_src(idx);
      skl[threadIdx.x] = static_cast<uint32_t>(a.src.key_size(idx));
    }
    __syncthreads();
    const uint64_t last = soff[kTbWindow];
    if (last >= p1) tb_region_span(win, kTbWindow, p0, p1, a.data);
    else tb_region_span(a.src, n, p0, p1, a.data);
    if (s + 1 < s1)  // p1 < limit: the next span's first pair
      first = last > p1 ? first + tb_last_le(win, kTbWindow, p1) : wave_last_le(at, n, p1);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kTbBlock) void tb_index_kernel(TbDev a) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTbIndexSpan];
  __shared__ int64_t wat[kTbIndexWindow];   // the entry's first byte relative to the span
  __shared__ uint64_t wsrc[kTbIndexWindow];  // its key
  __shared__ uint32_t wkl[kTbIndexWindow];   // ... and the key's length
  __shared__ uint32_t whd[kTbIndexWindow];   // the bytes in front of the key
  constexpr int64_t kNone = INT64_MAX;
  if (a.built[3] & kTbMalformed) return;
  const uint64_t n = a.n, E = a.tot[0], ctot = E + 4 * n + 4;
  const uint64_t limit = ctot < a.index_cap ? ctot : a.index_cap;
  const uint64_t spans = (limit + kTbIndexSpan - 1) / kTbIndexSpan;
  const uint64_t per = (spans + gridDim.x - 1) / gridDim.x;
  const uint64_t s0 = per * blockIdx.x;
  const uint64_t s1 = s0 + per < spans ? s0 + per : spans;
  const uint32_t* es = a.es;
  const uint64_t* off = a.src.off;
  for (uint64_t s = s0; s < s1; s++) {
    const uint64_t q0 = s * kTbIndexSpan;
    const uint64_t q1 = q0 + kTbIndexSpan < limit ? q0 + kTbIndexSpan : limit;
    if (q0 < E) {  // (n >= 1) the span's entries into the tile
      const uint64_t qe = q1 < E ? q1 : E;
      const int64_t len = static_cast<int64_t>(qe - q0);
      const uint64_t first = wave_last_le([&](uint64_t i) { return static_cast<uint64_t>(es[i]); }, n, q0);
      if (threadIdx.x < kTbIndexWindow) {
        const uint64_t idx = first + threadIdx.x;
        int64_t at = kNone;
        if (idx < n && es[idx] < qe) {
          const uint64_t ks = a.src.key_size(idx), o = off[idx], size = off[idx + 1] - o;
          at = static_cast<int64_t>(es[idx]) - static_cast<int64_t>(q0);
          tb_entry_write(tile, len, at, ks, o, size);
          wsrc[threadIdx.x] = a.src.key_src(idx);
          wkl[threadIdx.x] = static_cast<uint32_t>(ks);
          whd[threadIdx.x] = tb_entry_head(ks);
        }
        wat[threadIdx.x] = at;
      }
      __syncthreads();
      const uint32_t l = threadIdx.x & 31;
      for (uint32_t j = threadIdx.x >> 5; j < kTbIndexWindow; j += kTbBlock / 32) {
        const int64_t at = wat[j];
        if (at == kNone) break;  // the starts ascend: none follows
        const int64_t k0 = at + whd[j];
        const uint32_t kl = wkl[j];
        const kv_src1 key = reinterpret_cast<kv_src1>(wsrc[j]);
        for (uint32_t b = l; b < kl; b += 32) {
          const int64_t pos = k0 + b;
          if (pos >= 0 && pos < len) tile[pos] = key[b];
        }
      }
      __syncthreads();
    }
    if (threadIdx.x < kTbIndexSpan / 16) {
      const uint64_t q = q0 + 16 * threadIdx.x;
      if (q < q1) tb_index_unit(tile, q0, es, E, ctot, q, limit, a.index + q);
    }
    __syncthreads();  // the tile is rewritten by the next span
  }
}

}  // namespace

hipError_t launch_table_build(const TbDev& a, uint32_t index_wgs, hipEvent_t* ev, hipStream_t s) {
  if (a.nwg == 0 || a.nwg > kSortMaxWgs || a.cpw == 0 || a.copy_wgs == 0 || index_wgs == 0) return hipErrorInvalidValue;
  hipError_t e;
  auto mark = [&](int j) { return ev ? hipEventRecord(ev[j], s) : hipSuccess; };
  if ((e = mark(0)) != hipSuccess) return e;
  tb_size_kernel<<<a.nwg, kTbBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(1)) != hipSuccess) return e;
  tb_offsets_kernel<<<a.nwg, kTbBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(2)) != hipSuccess) return e;
  tb_region_kernel<<<1 + a.nwg + a.copy_wgs, kTbBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(3)) != hipSuccess) return e;
  tb_index_kernel<<<index_wgs, kTbBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return mark(4);
}

}  // namespace dlsm
