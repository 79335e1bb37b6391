// dlsm_amd/csrc/kv_read.hip -- the value read of a seeked Get batch
// (dlsm_kv_read_dev): (state, handle) per item in, a packed value buffer with
// offsets out.  The format's rules are the DLSM_HD functions of kv_read.h; this
// file is the work split.  Three launches ordered by the stream alone: no
// counter is shared between workgroups and nothing looks back.
//
// Size (kv_size_kernel): one thread per item, kKvChunk items per chunk, a
// workgroup takes cpw consecutive chunks.  A FOUND item's thread finds the
// chunk of its handle (a branchless search of the file's chunk ends; one chunk
// per file is the common case), loads the pair's header and key and runs
// kv_pair_decide; it leaves the value's length and source address in the
// workspace, so the copy needs no second lookup.  The workgroup's length sum
// and corrupt count go to the workspace.
//
// Offsets (kv_offsets_kernel): the same grid.  A workgroup sums the length sums
// of the workgroups below it (at most kSortMaxWgs of them), then scans its
// chunks' lengths into value_off; workgroup 0 also adds up the corrupt counts.
//
// Copy (kv_copy_kernel): output-centric, so a skewed length distribution cannot
// unbalance it.  The output bytes below min(total, values_cap) are cut into
// spans of kKvSpan bytes and a persistent grid takes a contiguous run of spans
// per workgroup.  The first item of a workgroup's first span comes from one
// uniform binary search of value_off; per span the workgroup stages the next
// kKvWindow items' offsets and source addresses in LDS, each lane owns whole
// 16-byte destination units and finds its unit's item in the window.  A unit
// inside one value is one unaligned 16-byte load and one aligned 16-byte
// non-temporal store; a unit that holds the boundary of two values of 16 bytes
// or more is two such loads, a shift and one store; any other boundary or the
// cut at the end is assembled per byte and written once (the last partial unit
// by byte stores).  A span with more items than the window holds (1-byte or empty
// values) has its lanes search value_off where it lies.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"
#include "sort_pass.h"

namespace dlsm {
namespace {

constexpr int kKvBlock = 1024;  // threads of every kernel here
constexpr int kKvWaves = kKvBlock / 64;
static_assert(kKvChunk == kKvBlock, "a thread per item of a chunk");
static_assert(kKvWindow + 1 == kKvBlock, "a thread stages one offset of the window");
static_assert(kKvSpan % (16 * kKvBlock) == 0, "every lane owns the same number of units of a span");
constexpr int kKvUnits = kKvSpan / (16 * kKvBlock);  // units per lane and span

__device__ __forceinline__ uint64_t kv_item_count(const KvReadDev& a) {
  const uint64_t c = a.count ? *a.count : a.cap;
  return c < a.cap ? c : a.cap;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// The sum of v over the workgroup, in every thread.  sh: kKvWaves slots.
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* sh) {
  v = wave_sum(v);
  __syncthreads();  // sh may still be read from the call before
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = 0;
#pragma unroll
  for (int w = 0; w < kKvWaves; w++) t += sh[w];
  return t;
}

__global__ __launch_bounds__(kKvBlock) void kv_size_kernel(KvReadDev a) {
  __shared__ uint64_t sh[kKvWaves];
  const uint64_t m = kv_item_count(a);
  const KeyDesc& kd = a.keys;
  uint64_t sum = 0, bad = 0;
  const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    const uint64_t i = c * kKvChunk + threadIdx.x;
    if (i >= m) break;
    const uint8_t* value = nullptr;
    uint32_t len = 0;
    if (a.state[i] == kGetFound) {
      const uint64_t g = a.gets ? a.gets[i] : i;
      uint8_t st = kGetCorrupt;
      if (g < kd.n) {
        uint64_t s, l;
        if (kd.offsets) {
          s = kd.offsets[g];
          l = kd.offsets[g + 1] - s;
        } else {
          s = g * kd.key_len;
          l = kd.key_len;
        }
        l = l > kd.suffix ? l - kd.suffix : 0;  // ExtractUserKey
        st = kv_item_decide(a.tables, a.handle[i], kd.bytes + s, static_cast<uint32_t>(l), &value, &len);
      }
      if (st != kGetFound) a.state[i] = st;
      bad += st == kGetCorrupt ? 1u : 0u;
    }
    a.len[i] = len;
    a.src[i] = reinterpret_cast<uint64_t>(value);
    sum += len;
  }
  sum = block_sum(sum, sh);
  bad = block_sum(bad, sh);
  if (threadIdx.x == 0) {
    a.wg_sum[blockIdx.x] = sum;
    a.wg_bad[blockIdx.x] = bad;
  }
}

__global__ __launch_bounds__(kKvBlock) void kv_offsets_kernel(KvReadDev a) {
  __shared__ uint64_t sh[kKvWaves];
  const uint64_t m = kv_item_count(a);
  // the exclusive scan of the workgroup sums, this workgroup's entry of it
  uint64_t below = 0;
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += kKvBlock) below += a.wg_sum[j];
  uint64_t run = block_sum(below, sh);
  if (blockIdx.x == 0) {
    uint64_t bad = 0;
    for (uint32_t j = threadIdx.x; j < a.nwg; j += kKvBlock) bad += a.wg_bad[j];
    bad = block_sum(bad, sh);
    if (threadIdx.x == 0) {
      if (a.n_corrupt) *a.n_corrupt = bad;
      if (m == 0) a.value_off[0] = 0;
    }
  }
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    if (c * kKvChunk >= m) break;  // (the same for every thread)
    const uint64_t i = c * kKvChunk + threadIdx.x;
    const uint64_t l = i < m ? a.len[i] : 0;
    uint64_t inc = l;  // the wave's inclusive scan
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t up = __shfl_up(inc, d, 64);
      inc += lane >= static_cast<uint32_t>(d) ? up : 0;
    }
    __syncthreads();
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kKvWaves; w++) {
      const uint64_t t = sh[w];
      before += static_cast<uint32_t>(w) < wave ? t : 0;
      all += t;
    }
    if (i < m) {
      a.value_off[i] = run + before + inc - l;
      if (i + 1 == m) a.value_off[m] = run + before + inc;
    }
    run += all;
  }
}

// The units of one span, off / src addressed from the span's first item:
// off[0] <= p0 and off[n] >= p1 (n >= 1 items).
__device__ __forceinline__ void kv_copy_span(const uint64_t* off, const uint64_t* src, uint64_t n, uint64_t p0,
                                             uint64_t p1, uint8_t* __restrict__ values) {
#pragma unroll
  for (int k = 0; k < kKvUnits; k++) {
    const uint64_t u = p0 + (static_cast<uint64_t>(k) * kKvBlock + threadIdx.x) * 16;
    if (u < p1) kv_copy_unit(off, src, n, u, p1, values);
  }
}

__global__ __launch_bounds__(kKvBlock) void kv_copy_kernel(KvReadDev a) {
  __shared__ uint64_t soff[kKvWindow + 1];
  __shared__ uint64_t ssrc[kKvWindow + 1];
  const uint64_t m = kv_item_count(a);
  if (m == 0) return;
  const uint64_t total = a.value_off[m];
  const uint64_t limit = total < a.values_cap ? total : a.values_cap;
  const uint64_t spans = (limit + kKvSpan - 1) / kKvSpan;
  const uint64_t per = (spans + gridDim.x - 1) / gridDim.x;
  const uint64_t s0 = per * blockIdx.x;
  const uint64_t s1 = s0 + per < spans ? s0 + per : spans;
  if (s0 >= s1) return;
  // p < limit <= value_off[m] for every byte p served here, and value_off[0] = 0
  uint64_t first = kv_last_le(a.value_off, m, s0 * kKvSpan);
  for (uint64_t s = s0; s < s1; s++) {
    const uint64_t p0 = s * kKvSpan;
    const uint64_t p1 = p0 + kKvSpan < limit ? p0 + kKvSpan : limit;
    const uint64_t idx = first + threadIdx.x;
    const uint64_t o = idx <= m ? a.value_off[idx] : ~uint64_t(0);
    soff[threadIdx.x] = o;
    if (idx < m && o < p1) ssrc[threadIdx.x] = a.src[idx];
    __syncthreads();
    const uint64_t last = soff[kKvWindow];
    if (last >= p1) kv_copy_span(soff, ssrc, kKvWindow, p0, p1, a.values);
    else kv_copy_span(a.value_off + first, a.src + first, m - first, p0, p1, a.values);
    if (s + 1 < s1)  // p1 < limit: the next span's first item
      first = last > p1 ? first + kv_last_le(soff, kKvWindow, p1) : first + kv_last_le(a.value_off + first, m - first, p1);
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_kv_read(const KvReadDev& a, uint32_t copy_wgs, hipEvent_t* ev, hipStream_t s) {
  if (a.cap == 0 || a.nwg == 0) return hipSuccess;
  if (a.nwg > kSortMaxWgs || a.cpw == 0 || copy_wgs == 0) return hipErrorInvalidValue;
  hipError_t e;
  auto mark = [&](int j) { return ev ? hipEventRecord(ev[j], s) : hipSuccess; };
  if ((e = mark(0)) != hipSuccess) return e;
  kv_size_kernel<<<a.nwg, kKvBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(1)) != hipSuccess) return e;
  kv_offsets_kernel<<<a.nwg, kKvBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(2)) != hipSuccess) return e;
  kv_copy_kernel<<<copy_wgs, kKvBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return mark(3);
}

}  // namespace dlsm
