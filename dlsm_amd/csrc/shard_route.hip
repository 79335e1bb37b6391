// dlsm_amd/csrc/shard_route.hip -- the shard route of a Get batch
// (dlsm_shard_route_dev): DBImpl_Sharding::Get_Target_Shard for every Get, and
// each shard's Gets as one contiguous, aligned run.
//
// One stable counting-sort pass of the Gets by shard (the bins: the shards and
// the "no shard" bin, at most kRouteBins, in LDS), built like a digit pass of
// the read plan (read_plan.hip).  Three launches, ordered by the stream alone
// (no counter is shared between workgroups, nothing inside a launch waits for
// another workgroup):
//   count    workgroup w walks its cpw chunks of kRouteChunk Gets, searches each
//            Get's shard (route_shard, the bounds' prefixes in LDS), writes it
//            as a u16 to ids[] and its count per bin to cnt[bin * nwg + w];
//   scan     one workgroup sums every bin, rounds each bin's start up to
//            kRouteAlign (shard_off, shard_cnt) and turns cnt into off[], the
//            first output position of every (bin, workgroup);
//   scatter  workgroup w reads its ids again and writes each Get's index (and
//            its key) to off[bin * nwg + w] + (its rank among w's Gets of the
//            bin).
// Ranks follow item order, never the arrival order of atomics: inside a wave by
// ballots over the bin's bits, across waves by the wave's number (each wave owns
// a contiguous share of the chunk and a row of LDS counts), across chunks and
// workgroups by the tables.  Gets are walked in ascending order, so each bin's
// run comes out strictly ascending.
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
// key).  The tables are (n_shards + 1) x nwg <= 512 x 512 entries whatever n is.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"

namespace dlsm {
namespace {

static_assert(kRouteBlock == 64 * kRouteWaves, "wave64");
static_assert(static_cast<uint64_t>(kRouteBins) * kRouteMaxWgs <= 0xffffffffull / 8, "table index in u32");
static_assert(kRouteScanBlock == 1024 && kRouteBins <= kRouteScanBlock, "scan: thread d < kRouteBins owns bin d");
static_assert(kRouteStageKeyMax % 4 == 0, "staged keys are whole dwords");

constexpr uint32_t kStageUnits = 64u * kRouteStageKeyMax / 16u;  // uint4 per wave: 64 keys of the longest staged length
constexpr uint32_t kNoItem = 0xffffffffu;
enum : int { kKeysNone = 0, kKeysStaged = 1, kKeysBytes = 2 };

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
}

// The active lanes of the wave whose bin equals this lane's (bits: the bins'
// width, the same in every lane).
__device__ __forceinline__ uint64_t route_peers(uint32_t d, bool active, uint32_t bits) {
  uint64_t peers = __ballot(active);
  for (uint32_t b = 0; b < bits; b++) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bb = __ballot(bit);
    peers &= bit ? bb : ~bb;
  }
  return peers;
}

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
__global__ __launch_bounds__(kRouteBlock, 8) void route_count_kernel(ShardRouteDev a) {
  __shared__ RoutePrefix spre[kRouteBins];
  __shared__ uint32_t hist[kRouteBins];
  __shared__ uint4 stage[STAGED ? kRouteWaves * kStageUnits : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t w = blockIdx.x;
  for (uint32_t d = tid; d < kRouteBins; d += kRouteBlock) {
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
    const uint64_t i0 = c0 + static_cast<uint64_t>(wave) * kRouteWaveItems;
    const uint64_t i1 = i0 + kRouteWaveItems < n ? i0 + kRouteWaveItems : n;
    for (uint64_t r = i0; r < i1; r += 64) {
      const uint64_t g = r + lane;
      const bool ok = g < i1;
      const bool whole = STAGED && r + 64 <= i1;  // the same in every lane
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
      const uint64_t peers = route_peers(bin, ok, bits);
      if (ok && lanes_below(peers) == 0) atomicAdd(&hist[bin], static_cast<uint32_t>(__builtin_popcountll(peers)));
    }
  }
  __syncthreads();
  for (uint32_t d = tid; d < a.bins; d += kRouteBlock) a.cnt[d * a.nwg + w] = hist[d];  // < bins * nwg
}

// Scan: shard_cnt[b] = the sum of bin b's counts; shard_off[b] = the previous
// bin's end rounded up to kRouteAlign; off[b * nwg + w] = shard_off[b] + the
// counts of b's workgroups before w.
__global__ __launch_bounds__(kRouteScanBlock) void route_scan_kernel(ShardRouteDev a) {
  __shared__ uint64_t tot[kRouteBins];
  __shared__ uint64_t begin[kRouteBins];
  __shared__ uint64_t wsum[kRouteScanBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t nwg = a.nwg, bins = a.bins;
  for (uint32_t b = wave; b < bins; b += kRouteScanBlock / 64) {
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
  for (uint32_t b = wave; b < bins; b += kRouteScanBlock / 64) {
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

// Scatter: every Get to off[bin * nwg + w] + its rank among workgroup w's Gets
// of the bin.  Per chunk: (A) each wave ranks its share per bin in its own LDS
// row, holding (bin, rank inside the share) in registers, (B) thread d turns
// bin d's wave counts into the waves' start positions inside the chunk (the
// chunk's own start after the chunks before is kept in its register), (C) each
// wave places its Gets (and their keys).
template <int KEYS>
__global__ __launch_bounds__(kRouteBlock, 8) void route_scatter_kernel(ShardRouteDev a) {
  __shared__ uint32_t tab[kRouteWaves][kRouteBins];  // (A) a wave's Gets per bin, (C) its first position in the chunk's bin
  __shared__ uint64_t start[kRouteBins];             // the chunk's first position per bin
  __shared__ uint4 stage[KEYS == kKeysStaged ? kRouteWaves * kStageUnits : 1];
  static_assert(sizeof(tab) + sizeof(start) + sizeof(uint4) * kRouteWaves * kStageUnits <= 80 * 1024,
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
    for (uint32_t q = lane; q < kRouteBins; q += 64) tab[wave][q] = 0;  // the wave's own row
    __builtin_amdgcn_wave_barrier();
    const uint64_t i0 = c0 + static_cast<uint64_t>(wave) * kRouteWaveItems;
    uint32_t held[kRouteHold];
#pragma unroll
    for (int q = 0; q < kRouteHold; q++) {  // the share's ids, all in flight
      const uint64_t j = i0 + 64u * q + lane;
      held[q] = j < n ? a.ids[j] : kNoItem;
    }
#pragma unroll
    for (int q = 0; q < kRouteHold; q++) {
      const bool ok = held[q] != kNoItem;
      const uint32_t d = ok ? held[q] : 0u;
      const uint64_t peers = route_peers(d, ok, bits);
      const uint32_t below = lanes_below(peers);
      const uint32_t loc = ok ? tab[wave][d] + below : 0;
      __builtin_amdgcn_wave_barrier();
      if (ok && below == 0) tab[wave][d] = loc + static_cast<uint32_t>(__builtin_popcountll(peers));
      __builtin_amdgcn_wave_barrier();
      held[q] = ok ? (d | (loc << kRouteBinLg)) : kNoItem;
    }
    __syncthreads();
    if (static_cast<uint32_t>(tid) < a.bins) {  // (B)
      uint32_t run = 0;  // <= kRouteChunk
      for (int v = 0; v < kRouteWaves; v++) {
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
      if (held[q] == kNoItem) continue;
      const uint32_t d = held[q] & (kRouteBins - 1u);
      const uint64_t pos = start[d] + tab[wave][d] + (held[q] >> kRouteBinLg);
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
  if (a.nwg == 0 || a.nwg > kRouteMaxWgs || a.cpw == 0 || a.bins < 2 || a.bins > kRouteBins ||
      a.bounds.n + 1 != a.bins)
    return hipErrorInvalidValue;
  const dim3 grid(a.nwg), block(kRouteBlock);
  const bool staged = a.keys.offsets == nullptr && a.keys.key_len >= 4 && a.keys.key_len <= kRouteStageKeyMax &&
                      a.keys.key_len % 4 == 0 && (reinterpret_cast<uintptr_t>(a.keys.bytes) & 15u) == 0;
  if (staged) hipLaunchKernelGGL((route_count_kernel<true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((route_count_kernel<false>), grid, block, 0, s, a);
  hipLaunchKernelGGL(route_scan_kernel, dim3(1), dim3(kRouteScanBlock), 0, s, a);
  if (!a.keys_out) hipLaunchKernelGGL((route_scatter_kernel<kKeysNone>), grid, block, 0, s, a);
  else if (staged && (reinterpret_cast<uintptr_t>(a.keys_out) & 3u) == 0)
    hipLaunchKernelGGL((route_scatter_kernel<kKeysStaged>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((route_scatter_kernel<kKeysBytes>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace dlsm
