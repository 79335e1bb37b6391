// dlsm_amd/csrc/shard_route.hip -- the shard route of a Get batch
// (dlsm_shard_route_dev): DBImpl_Sharding::Get_Target_Shard for every Get, and
// each shard's Gets as one contiguous, aligned run.
//
// One pass of sort_pass.h over the Gets with the shard as the bin (the shards
// and the "no shard" bin).  The count searches each Get's shard (route_shard,
// the bounds' prefixes in LDS) and leaves it as a u16 in ids[] for the scatter;
// the scan rounds each bin's start up to kRouteAlign (shard_off, shard_cnt);
// the scatter writes each Get's index (and its key).  Gets are walked in
// ascending order, so each bin's run comes out strictly ascending.
//
// Keys: a fixed-stride keyset whose length is a multiple of 4 (<=
// kRouteStageKeyMax) at a 16-byte-aligned base is read 64 keys at a time with
// coalesced 16-byte loads into the wave's LDS area (64 keys start at a multiple
// of 256 bytes); each lane then takes its key's dwords from there.  Everything
// else (other lengths, other bases, offsets, the last partial 64) goes through
// the byte loader.  The lanes of a wave that share a bin hold consecutive
// destinations, so their dword stores of gets_dev and of the keys fill whole
// runs.
//
// Bytes per Get of 20-byte keys: count 20 B in + 2 B out, scatter 2 B + 20 B in,
// 4 B + 20 B out: 68 B with keys_out, 28 B without (the scatter then reads no
// key).
#include <hip/hip_runtime.h>

#include "bloom_internal.h"

namespace dlsm {
namespace {

static_assert(kRouteStageKeyMax % 4 == 0, "staged keys are whole dwords");

constexpr uint32_t kStageUnits = 64u * kRouteStageKeyMax / 16u;  // uint4 per wave: 64 keys of the longest staged length
enum : int { kKeysNone = 0, kKeysStaged = 1, kKeysBytes = 2 };

__device__ __forceinline__ uint32_t bin_bits(uint32_t bins) {  // bins >= 2
  return 32u - static_cast<uint32_t>(__builtin_clz(bins - 1u));
}

// The staged keysets (launch_shard_route): fixed stride, whole dwords, short
// enough for the wave's LDS area, 16-byte aligned base -- 64 keys are then
// 4 x key_len whole 16-byte units.  The 64 keys from g0 (a multiple of 64, g0 + 64 <= n) into the wave's LDS
// area: 4 x key_len <= 2 x 64 units, both loads in flight before the stores.
__device__ __forceinline__ void stage_keys64(const KeyDesc& kd, uint64_t g0, uint4* area, int lane) {
  const uint4* src = reinterpret_cast<const uint4*>(kd.bytes + g0 * kd.key_len);
  const uint32_t units = 4u * kd.key_len;  // <= kStageUnits
  const uint32_t u0 = lane, u1 = lane + 64u;
  uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0;
  if (u0 < units) v0 = src[u0];
  if (u1 < units) v1 = src[u1];
  __builtin_amdgcn_wave_barrier();  // (the wave's earlier reads of the area come first)
  if (u0 < units) area[u0] = v0;
  if (u1 < units) area[u1] = v1;
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ RoutePrefix prefix_words(const uint32_t* w) {
  RoutePrefix q;
  q.hi = (static_cast<uint64_t>(__builtin_bswap32(w[0])) << 32) | __builtin_bswap32(w[1]);
  q.lo = (static_cast<uint64_t>(__builtin_bswap32(w[2])) << 32) | __builtin_bswap32(w[3]);
  return q;
}

// Count: ids[g] = Get g's bin; cnt[bin * nwg + w] = workgroup w's Gets per bin.
template <bool STAGED>
__global__ __launch_bounds__(kSortBlock, 8) void route_count_kernel(ShardRouteDev a) {
  __shared__ RoutePrefix spre[kSortBins];
  __shared__ uint32_t hist[kSortBins];
  __shared__ uint4 stage[STAGED ? kSortWaves * kStageUnits : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t w = blockIdx.x;
  for (uint32_t d = tid; d < kSortBins; d += kSortBlock) {
    hist[d] = 0;
    if (d < a.bounds.n) spre[d] = a.bounds.pre[d];
  }
  __syncthreads();
  RouteBounds B = a.bounds;
  B.pre = spre;
  const KeyDesc& kd = a.keys;
  const uint64_t n = kd.n;
  const uint32_t bits = bin_bits(a.bins);
  uint4* area = stage + (STAGED ? wave * kStageUnits : 0);
  for (uint64_t c = static_cast<uint64_t>(w) * a.cpw; c < static_cast<uint64_t>(w + 1) * a.cpw; c++) {
    const uint64_t c0 = c * kRouteChunk;
    if (c0 >= n) break;
    const WaveShare sh = wave_share<kRouteChunk>(c0, wave, n);
    for (uint64_t r = sh.i0; r < sh.i1; r += 64) {
      const uint64_t g = r + lane;
      const bool ok = g < sh.i1;
      const bool whole = STAGED && r + 64 <= sh.i1;  // the same in every lane
      uint32_t bin = 0;
      if (whole) {
        stage_keys64(kd, r, area, lane);
        const uint32_t* kw = reinterpret_cast<const uint32_t*>(area) + lane * (kd.key_len / 4u);
        const uint64_t ul = kd.key_len - kd.suffix;  // ExtractUserKey (key_len >= suffix: validate_keyset)
        const uint8_t* kp = reinterpret_cast<const uint8_t*>(kw);
        const RoutePrefix q = ul >= 16 ? prefix_words(kw) : route_prefix(kp, ul);
        bin = route_shard(B, q, kp, ul);
      } else if (ok) {
        uint64_t s, l;
        if (kd.offsets) {
          s = kd.offsets[g];
          l = kd.offsets[g + 1] - s;
        } else {
          s = g * kd.key_len;
          l = kd.key_len;
        }
        l = l > kd.suffix ? l - kd.suffix : 0;
        const uint8_t* kp = kd.bytes + s;
        bin = route_shard(B, route_prefix(kp, l), kp, l);
      }
      if (ok) a.ids[g] = static_cast<uint16_t>(bin);  // g < n; bin <= bounds.n < bins
      hist_add(hist, bin, ok, digit_peers(__ballot(ok), bin, bits));
    }
  }
  __syncthreads();
  hist_flush(hist, a.bins, a.cnt, a.nwg, w, tid);
}

// Scan: shard_cnt[b] = the sum of bin b's counts; shard_off[b] = the previous
// bin's end rounded up to kRouteAlign; off[b * nwg + w] = shard_off[b] + the
// counts of b's workgroups before w.
__global__ __launch_bounds__(kSortScanBlock) void route_scan_kernel(ShardRouteDev a) {
  __shared__ uint64_t tot[kSortBins];
  __shared__ uint64_t begin[kSortBins];
  __shared__ uint64_t wsum[kSortScanBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t nwg = a.nwg, bins = a.bins;
  for (uint32_t b = wave; b < bins; b += kSortScanBlock / 64) {
    uint64_t s = 0;
    for (uint32_t j = lane; j < nwg; j += 64) s += a.cnt[b * nwg + j];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) tot[b] = s;
  }
  __syncthreads();
  // exclusive sums of the padded totals: a bin's start is a multiple of
  // kRouteAlign, so its end rounded up is its start plus its padded total
  const uint64_t t = static_cast<uint32_t>(tid) < bins ? tot[tid] : 0;
  const uint64_t padded = (t + kRouteAlign - 1) & ~static_cast<uint64_t>(kRouteAlign - 1);
  uint64_t inc = padded;
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t u = __shfl_up(inc, d, 64);
    if (lane >= d) inc += u;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint64_t wpre = 0;
  for (int k = 0; k < wave; k++) wpre += wsum[k];
  if (static_cast<uint32_t>(tid) < bins) {
    const uint64_t o = wpre + inc - padded;
    begin[tid] = o;
    a.shard_off[tid] = o;
    a.shard_cnt[tid] = t;
  }
  __syncthreads();
  for (uint32_t b = wave; b < bins; b += kSortScanBlock / 64) {
    uint64_t carry = begin[b];
    for (uint32_t j0 = 0; j0 < nwg; j0 += 64) {
      const uint32_t j = j0 + lane;
      const uint64_t c = j < nwg ? a.cnt[b * nwg + j] : 0;
      uint64_t x = c;
      for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = __shfl_up(x, d, 64);
        if (lane >= d) x += u;
      }
      if (j < nwg) a.off[b * nwg + j] = carry + x - c;
      carry += __shfl(x, 63, 64);
    }
  }
}

// Scatter (sort_pass.h, (A) to (C)): a wave holds its share of a chunk, and (C)
// places the Gets and their keys.
template <int KEYS>
__global__ __launch_bounds__(kSortBlock, 8) void route_scatter_kernel(ShardRouteDev a) {
  __shared__ uint32_t tab[kSortWaves][kSortBins];  // (A) a wave's Gets per bin, (C) its first position in the chunk's bin
  __shared__ uint64_t start[kSortBins];            // the chunk's first position per bin
  __shared__ uint4 stage[KEYS == kKeysStaged ? kSortWaves * kStageUnits : 1];
  static_assert(sizeof(tab) + sizeof(start) + sizeof(uint4) * kSortWaves * kStageUnits <= 80 * 1024,
                "scatter LDS: two workgroups per CU");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t w = blockIdx.x;
  const KeyDesc& kd = a.keys;
  const uint64_t n = kd.n;
  const uint32_t bits = bin_bits(a.bins);
  const uint32_t kl = kd.key_len;
  uint4* area = stage + (KEYS == kKeysStaged ? wave * kStageUnits : 0);
  uint64_t next = 0;  // thread d < bins: bin d's first position of the next chunk
  if (static_cast<uint32_t>(tid) < a.bins) next = a.off[static_cast<uint32_t>(tid) * a.nwg + w];
  for (uint64_t c = static_cast<uint64_t>(w) * a.cpw; c < static_cast<uint64_t>(w + 1) * a.cpw; c++) {
    const uint64_t c0 = c * kRouteChunk;
    if (c0 >= n) break;
    for (uint32_t q = lane; q < kSortBins; q += 64) tab[wave][q] = 0;  // the wave's own row
    __builtin_amdgcn_wave_barrier();
    const uint64_t i0 = wave_share<kRouteChunk>(c0, wave, n).i0;
    uint32_t held[kRouteHold];
#pragma unroll
    for (int q = 0; q < kRouteHold; q++) {  // the share's ids, all in flight
      const uint64_t j = i0 + 64u * q + lane;
      held[q] = j < n ? a.ids[j] : kSortNoItem;
    }
#pragma unroll
    for (int q = 0; q < kRouteHold; q++) {
      const bool ok = held[q] != kSortNoItem;
      const uint32_t d = ok ? held[q] : 0u;
      held[q] = rank_held(tab[wave], d, ok, digit_peers(__ballot(ok), d, bits));
    }
    __syncthreads();
    if (static_cast<uint32_t>(tid) < a.bins) {  // (B)
      uint32_t run = 0;  // <= kRouteChunk
      for (int v = 0; v < kSortWaves; v++) {
        const uint32_t t = tab[v][tid];
        tab[v][tid] = run;
        run += t;
      }
      start[tid] = next;
      next += run;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kRouteHold; q++) {
      const uint64_t r = i0 + 64u * q;
      if (r >= n) break;  // the same in every lane
      const uint64_t j = r + lane;
      const bool whole = KEYS == kKeysStaged && r + 64 <= n;
      if (whole) stage_keys64(kd, r, area, lane);
      if (held[q] == kSortNoItem) continue;
      const uint64_t pos = held_pos(held[q], tab[wave], start);
      if (pos >= a.cap) continue;  // (never: cap >= dlsm_shard_route_cap)
      a.gets[pos] = static_cast<uint32_t>(j);
      if (KEYS == kKeysStaged) {
        // whole dwords; the source is the wave's LDS area or, for the batch's
        // last partial 64, the key where it lies (4-byte aligned)
        const uint32_t kw = kl / 4u;  // <= 8
        const uint32_t* src = whole ? reinterpret_cast<const uint32_t*>(area) + lane * kw
                                    : reinterpret_cast<const uint32_t*>(kd.bytes + j * kl);
        uint32_t* dst = reinterpret_cast<uint32_t*>(a.keys_out + pos * kl);
#pragma unroll 1
        for (uint32_t x = 0; x < kw; x++) dst[x] = src[x];
      } else if (KEYS == kKeysBytes) {
        const uint8_t* src = kd.bytes + j * kl;
        uint8_t* dst = a.keys_out + pos * kl;
        for (uint32_t x = 0; x < kl; x++) dst[x] = src[x];
      }
    }
  }
}

}  // namespace

hipError_t launch_shard_route(const ShardRouteDev& a, hipStream_t s) {
  if (a.nwg == 0 || a.nwg > kSortMaxWgs || a.cpw == 0 || a.bins < 2 || a.bins > kSortBins ||
      a.bounds.n + 1 != a.bins)
    return hipErrorInvalidValue;
  const dim3 grid(a.nwg), block(kSortBlock);
  const bool staged = a.keys.offsets == nullptr && a.keys.key_len >= 4 && a.keys.key_len <= kRouteStageKeyMax &&
                      a.keys.key_len % 4 == 0 && (reinterpret_cast<uintptr_t>(a.keys.bytes) & 15u) == 0;
  if (staged) hipLaunchKernelGGL((route_count_kernel<true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((route_count_kernel<false>), grid, block, 0, s, a);
  hipLaunchKernelGGL(route_scan_kernel, dim3(1), dim3(kSortScanBlock), 0, s, a);
  if (!a.keys_out) hipLaunchKernelGGL((route_scatter_kernel<kKeysNone>), grid, block, 0, s, a);
  else if (staged && (reinterpret_cast<uintptr_t>(a.keys_out) & 3u) == 0)
    hipLaunchKernelGGL((route_scatter_kernel<kKeysStaged>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((route_scatter_kernel<kKeysBytes>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace dlsm
