// dlsm_amd/csrc/wg_scan.h -- sums, scans and a search over a workgroup of
// kWaves whole waves (wave64): the two-level passes of table_build.hip,
// compaction_output.hip, compaction_merge.hip, compaction_filters.hip and
// kv_read.hip, each with its own wave count.  Every function is called by the
// whole workgroup; sh is an LDS slot per wave and may be handed to the next call
// as it is.
//
// compaction_merge.hip's block_scan3 is the deliberate exception and stays with
// its kernel: three of these scans side by side spilled, so it scans the waves'
// totals in the first wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dlsm {

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// The sum of v over the workgroup, in every thread.
template <int kWaves>
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* sh) {
  v = wave_sum(v);
  __syncthreads();  // sh may still be read from the call before
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) t += sh[w];
  return t;
}

// The exclusive scan of v over the workgroup; *all: the sum.
template <class T, int kWaves>
__device__ __forceinline__ T block_scan(T v, T* sh, T* all) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(inc, d, 64);
    inc += lane >= static_cast<uint32_t>(d) ? up : 0;
  }
  __syncthreads();  // sh may still be read from the call before
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  T before = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) {
    const T x = sh[w];
    before += static_cast<uint32_t>(w) < wave ? x : 0;
    sum += x;
  }
  *all = sum;
  return before + inc - v;
}

// The last i in [0, n) with f(i) <= p, given f(0) <= p (n >= 1) and f
// ascending: a 64-ary search, every lane of the (whole, converged) wave probing
// one point per step.  The same answer in every lane.
template <class F>
__device__ __forceinline__ uint64_t wave_last_le(F f, uint64_t n, uint64_t p) {
  const uint64_t lane = threadIdx.x & 63;
  uint64_t lo = 0;
  for (uint64_t len = n; len > 1;) {
    const uint64_t step = (len + 63) >> 6;
    const bool ok = lane * step < len && f(lo + lane * step) <= p;
    const uint64_t k = static_cast<uint64_t>(__popcll(__ballot(ok))) - 1;  // lane 0's point is f(lo) <= p
    lo += k * step;
    len = len - k * step < step ? len - k * step : step;
  }
  return lo;
}

}  // namespace dlsm
