// dlsm_amd/csrc/read_plan.hip -- the read plan of a probed batch
// (dlsm_version_read_plan_dev): the version probe's answers grouped by file.
//
// A stable counting sort of the (Get, file) tasks by the caller's file index,
// one pass of sort_pass.h per digit of kSortBinLg bits, least significant
// first.  Items are in ascending Get order in pass 0 and every pass is stable,
// so each file's Gets come out strictly ascending.  The histogram of pass 0
// also counts the dropped tasks; the scan writes file_begin when one pass
// covers the files (bin == file), else plan_bounds_kernel finds it in the
// sorted ids.
//
// Sources of a pass: the masks and picks (pass 0; ALL in both launches), the
// per-Get file ids the histogram leaves (pass 0, FIRST: the scatter), the
// pairs of the pass before (later passes).
//
// Bytes per Get, DLSM_PLAN_FIRST, one pass (db_bench's 426 files): the
// histogram reads the 8-B mask (16-byte loads) and, for a task on levels 1-5
// only, its 4-B pick (of a 20-B row), and writes the task's 4-B file id; the
// scatter reads that id and writes the 4-B Get index: 20 B + the pick per Get
// (24 B with the word alone, 40 B when the whole row's sectors are fetched),
// against 8 + 4 B twice without the id array.  DLSM_PLAN_ALL decodes the masks
// and picks in both launches (a Get has several tasks: 2 x (8 B + picks) +
// 4 B per task).  Every further pass reads 4 B (histogram) + 8 B (scatter) and
// writes 8 B per task.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"

namespace dlsm {
namespace {

struct PlanPassDev {
  uint32_t shift, cpw, nwg;
  uint32_t* keys_in;         // pass 0, FIRST: the per-Get file ids (the histogram writes them)
  const uint32_t* vals_in;
  uint32_t* keys_out;
  uint32_t* vals_out;
};

enum : int { kSrcMasks = 0, kSrcIds = 1, kSrcPairs = 2 };

// The active lanes of the wave whose digit equals this lane's.  same: the
// caller knows that every active lane holds one file (a level-0 slot).
__device__ __forceinline__ uint64_t plan_peers(uint32_t d, bool active, bool same) {
  const uint64_t among = __ballot(active);
  return same ? among : digit_peers(among, d, kSortBinLg);
}

// Task (Get g, slot s) -> the caller's file index, or kPlanNoFile (dropped).
__device__ __forceinline__ uint32_t plan_decode(const ReadPlanDev& a, uint64_t g, uint32_t s) {
  uint32_t pick = 0;
  if (s >= a.shape.n_l0 && s < a.shape.n_slots && a.pick) pick = a.pick[g * kPlanLevels + (s - a.shape.n_l0)];
  const uint32_t f = plan_task_file(a.shape, s, pick);  // < n_files or kPlanNoFile
  return f == kPlanNoFile || f >= a.n_files ? kPlanNoFile : a.order[f];
}

// Wave walk over Gets [i0, i1) (i0 a multiple of 128), 128 at a time: lane L
// takes Get r + L, then Get r + 64 + L, so items stay in Get order.  f(key, val,
// ok, same) is called by the whole wave (key kPlanNoFile: no item in this lane;
// same: every item of this call has one file).  ALL walks the 64 Gets slot by
// slot: a file has one slot, so each file's items still come in Get order.
template <bool ALL, class F>
__device__ __forceinline__ void walk_masks(const ReadPlanDev& a, uint64_t i0, uint64_t i1, int lane,
                                           uint64_t& dropped, F&& f) {
  const bool al16 = (reinterpret_cast<uintptr_t>(a.mask) & 15u) == 0;
  const uint32_t ns = a.shape.n_slots;
  for (uint64_t r = i0; r < i1; r += 128) {
    uint64_t m[2];
    if (al16 && r + 128 <= i1) {
      // one 16-byte load per lane (Gets r + 2L, r + 2L + 1), then to Get order
      const ulonglong2 v = reinterpret_cast<const ulonglong2*>(a.mask + r)[lane];
#pragma unroll
      for (int sub = 0; sub < 2; sub++) {
        const int src = 32 * sub + (lane >> 1);
        const uint64_t x = __shfl(v.x, src, 64), y = __shfl(v.y, src, 64);
        m[sub] = (lane & 1) ? y : x;
      }
    } else {
#pragma unroll
      for (int sub = 0; sub < 2; sub++) {
        const uint64_t g = r + 64u * sub + lane;
        m[sub] = g < i1 ? a.mask[g] : 0;
      }
    }
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      if (r + 64u * sub >= i1) break;
      const uint64_t g = r + 64u * sub + lane;
      const bool ok = g < i1;
      const uint64_t mm = m[sub];
      if (!ALL) {
        uint32_t key = kPlanNoFile;
        if (mm) {
          key = plan_decode(a, g, static_cast<uint32_t>(__builtin_ctzll(mm)));
          if (key == kPlanNoFile) dropped++;
        }
        f(key, static_cast<uint32_t>(g), ok, false);
      } else {
        if (ns < 64) dropped += static_cast<uint32_t>(__builtin_popcountll(mm >> ns));
        // the level tasks' picks and files first, all in flight at once
        uint32_t lk[kPlanLevels];
#pragma unroll
        for (int lv = 0; lv < kPlanLevels; lv++) {
          const uint32_t s = a.shape.n_l0 + lv;  // <= 63
          lk[lv] = kPlanNoFile;
          if ((mm >> s) & 1u) {
            lk[lv] = plan_decode(a, g, s);
            if (lk[lv] == kPlanNoFile) dropped++;
          }
        }
        for (uint32_t s = 0; s < a.shape.n_l0; s++) {  // level-0 slots: one file per slot
          const bool bit = (mm >> s) & 1u;
          if (__ballot(bit) == 0) continue;  // no lane has a task in this slot
          uint32_t key = kPlanNoFile;
          if (bit) {
            key = plan_decode(a, g, s);
            if (key == kPlanNoFile) dropped++;
          }
          f(key, static_cast<uint32_t>(g), ok, true);
        }
#pragma unroll
        for (int lv = 0; lv < kPlanLevels; lv++) {
          const bool bit = (mm >> (a.shape.n_l0 + lv)) & 1u;
          if (__ballot(bit) == 0) continue;
          f(lk[lv], static_cast<uint32_t>(g), ok, false);
        }
      }
    }
  }
}

// Wave walk over items [i0, i1) of a (file id, Get index) array.
template <bool PAIRS, class F>
__device__ __forceinline__ void walk_keys(const uint32_t* keys, const uint32_t* vals, uint64_t i0, uint64_t i1,
                                          int lane, F&& f) {
  for (uint64_t r = i0; r < i1; r += 64) {
    const uint64_t j = r + lane;
    const bool ok = j < i1;
    const uint32_t key = ok ? keys[j] : kPlanNoFile;
    const uint32_t val = PAIRS ? (ok ? vals[j] : 0u) : static_cast<uint32_t>(j);
    f(key, val, ok, false);
  }
}

template <int SRC, bool ALL, class F>
__device__ __forceinline__ void walk(const ReadPlanDev& a, const PlanPassDev& p, uint64_t i0, uint64_t i1, int lane,
                                     uint64_t& dropped, F&& f) {
  if (SRC == kSrcMasks) walk_masks<ALL>(a, i0, i1, lane, dropped, f);
  else walk_keys<SRC == kSrcPairs>(p.keys_in, p.vals_in, i0, i1, lane, f);
}

template <int SRC>
__device__ __forceinline__ uint64_t pass_items(const ReadPlanDev& a) {
  if (SRC != kSrcPairs) return a.n;
  const uint64_t t = *a.total;
  return t < a.pair_items ? t : a.pair_items;
}

// Histogram: cnt[bin * nwg + w] = workgroup w's items per bin.  From the masks
// (pass 0) it also counts the dropped tasks and, in FIRST mode, writes each
// Get's file id (kPlanNoFile: none) for the scatter.
template <int SRC, bool ALL>
__global__ __launch_bounds__(kSortBlock, 8) void plan_hist_kernel(ReadPlanDev a, PlanPassDev p) {
  __shared__ uint32_t hist[kSortBins];
  __shared__ unsigned long long sdrop;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t w = blockIdx.x;
  for (uint32_t d = tid; d < kSortBins; d += kSortBlock) hist[d] = 0;
  if (tid == 0) sdrop = 0;
  __syncthreads();
  const uint64_t items = pass_items<SRC>(a);
  uint64_t dropped = 0;
  auto count = [&](uint32_t key, uint32_t val, bool ok, bool same) {
    const bool active = key != kPlanNoFile;
    const uint32_t d = plan_digit(key, p.shift);  // < kSortBins
    const uint64_t peers = plan_peers(d, active, same);
    hist_add(hist, d, active, peers);
    if (SRC == kSrcMasks && !ALL && ok) p.keys_in[val] = key;  // val = the Get, < n
  };
  for (uint64_t c = static_cast<uint64_t>(w) * p.cpw; c < static_cast<uint64_t>(w + 1) * p.cpw; c++) {
    const uint64_t c0 = c * kPlanChunk;
    if (c0 >= items) break;
    const WaveShare sh = wave_share<kPlanChunk>(c0, wave, items);
    walk<SRC, ALL>(a, p, sh.i0, sh.i1, lane, dropped, count);
  }
  if (SRC == kSrcMasks) {
    for (int d = 32; d > 0; d >>= 1) dropped += __shfl_xor(dropped, d, 64);
    if (lane == 0 && dropped) atomicAdd(&sdrop, static_cast<unsigned long long>(dropped));
  }
  __syncthreads();
  hist_flush(hist, kSortBins, a.cnt, p.nwg, w, tid);
  if (SRC == kSrcMasks && tid == 0) a.drop[w] = sdrop;
}

// Scan: off[] = exclusive prefix sums of cnt[0, kSortBins * nwg); *total; with
// write_begin (one pass covers the files: bin == file) file_begin; with
// write_drop the sum of the workgroups' dropped tasks.
__global__ __launch_bounds__(kSortScanBlock) void plan_scan_kernel(ReadPlanDev a, uint32_t nwg, int write_begin,
                                                                   int write_drop) {
  __shared__ uint64_t wsum[kSortScanBlock / 64];
  constexpr uint32_t kPer = 16;  // entries per thread and tile: four 16-byte loads in flight
  static_assert(kSortBins % kPer == 0, "a tile never ends inside a thread's entries");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t entries = kSortBins * nwg;  // a multiple of kPer
  uint64_t carry = 0;
  for (uint32_t base = 0; base < entries; base += kPer * kSortScanBlock) {
    const uint32_t e = base + kPer * tid;
    uint32_t c[kPer];
#pragma unroll
    for (uint32_t q = 0; q < kPer; q += 4) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (e < entries) v = *reinterpret_cast<const uint4*>(a.cnt + e + q);
      c[q] = v.x, c[q + 1] = v.y, c[q + 2] = v.z, c[q + 3] = v.w;
    }
    uint64_t s = 0;
#pragma unroll
    for (uint32_t q = 0; q < kPer; q++) s += c[q];
    uint64_t inc = s;
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint64_t wpre = 0, tile = 0;
    for (int k = 0; k < kSortScanBlock / 64; k++) {
      const uint64_t v = wsum[k];
      if (k < wave) wpre += v;
      tile += v;
    }
    if (e < entries) {
      uint64_t o = carry + wpre + inc - s;
#pragma unroll
      for (uint32_t q = 0; q < kPer; q += 2) {
        const uint64_t o1 = o + c[q];
        *reinterpret_cast<ulonglong2*>(a.off + e + q) = make_ulonglong2(o, o1);
        if (write_begin) {
          const uint32_t f0 = (e + q) / nwg, f1 = (e + q + 1) / nwg;
          if ((e + q) - f0 * nwg == 0 && f0 < a.n_files) a.file_begin[f0] = o;
          if ((e + q + 1) - f1 * nwg == 0 && f1 < a.n_files) a.file_begin[f1] = o1;
        }
        o = o1 + c[q + 1];
      }
    }
    carry += tile;
    __syncthreads();
  }
  if (tid == 0) {
    *a.total = carry;
    if (write_begin) a.file_begin[a.n_files] = carry;
  }
  if (write_drop && a.dropped) {
    uint64_t d = 0;
    for (uint32_t q = tid; q < nwg; q += kSortScanBlock) d += a.drop[q];
    for (int k = 32; k > 0; k >>= 1) d += __shfl_xor(d, k, 64);
    if (lane == 0) wsum[wave] = d;
    __syncthreads();
    if (tid == 0) {
      uint64_t t = 0;
      for (int k = 0; k < kSortScanBlock / 64; k++) t += wsum[k];
      *a.dropped = t;
    }
  }
}

// Scatter (sort_pass.h, (A) to (C)).  From the masks (A) counts each wave's
// share per bin and (C) walks the share again, ranking as it places; items from
// an array are ranked once and held.
template <int SRC, bool ALL, bool LAST>
__global__ __launch_bounds__(kSortBlock, 8) void plan_scatter_kernel(ReadPlanDev a, PlanPassDev p) {
  __shared__ uint32_t cnt[kSortWaves][kSortBins];  // (A) a wave's items per bin; zero between chunks
  __shared__ uint32_t off[kSortWaves][kSortBins];  // (C) the wave's next position in the bin, from start[]
  __shared__ uint64_t start[kSortBins];            // the chunk's first position per bin
  static_assert(sizeof(cnt) + sizeof(off) + sizeof(start) <= 80 * 1024, "scatter LDS: two workgroups per CU");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t w = blockIdx.x;
  uint64_t next = 0;  // thread d < kSortBins: bin d's first position of the next chunk
  if (tid < static_cast<int>(kSortBins)) next = a.off[static_cast<uint32_t>(tid) * p.nwg + w];
  for (uint32_t q = tid; q < kSortWaves * kSortBins; q += kSortBlock) (&cnt[0][0])[q] = 0;
  __syncthreads();
  const uint64_t items = pass_items<SRC>(a);
  uint64_t unused = 0;
  auto count = [&](uint32_t key, uint32_t, bool, bool same) {
    const bool active = key != kPlanNoFile;
    const uint32_t d = plan_digit(key, p.shift);
    const uint64_t peers = plan_peers(d, active, same);
    if (active && lanes_below(peers) == 0) cnt[wave][d] += static_cast<uint32_t>(__builtin_popcountll(peers));
    __builtin_amdgcn_wave_barrier();
  };
  auto place = [&](uint32_t key, uint32_t val, bool, bool same) {
    const bool active = key != kPlanNoFile;
    const uint32_t d = plan_digit(key, p.shift);
    const uint64_t peers = plan_peers(d, active, same);
    const uint32_t below = lanes_below(peers);
    const uint32_t o = active ? off[wave][d] : 0;
    __builtin_amdgcn_wave_barrier();
    if (active && below == 0) off[wave][d] = o + static_cast<uint32_t>(__builtin_popcountll(peers));
    __builtin_amdgcn_wave_barrier();
    if (!active) return;
    const uint64_t pos = start[d] + o + below;
    if (LAST) {
      if (pos < a.cap) a.gets[pos] = val;
      if (p.keys_out && pos < a.pair_items) p.keys_out[pos] = key;
    } else if (pos < a.pair_items) {
      p.keys_out[pos] = key;
      p.vals_out[pos] = val;
    }
  };
  auto spread = [&]() {  // (B)
    if (tid < static_cast<int>(kSortBins)) {
      uint32_t run = 0;  // <= kPlanChunk x 64 tasks
      for (int v = 0; v < kSortWaves; v++) {
        const uint32_t t = cnt[v][tid];
        cnt[v][tid] = 0;
        off[v][tid] = run;
        run += t;
      }
      start[tid] = next;
      next += run;
    }
  };
  if (SRC != kSrcMasks) {
    // Items from an array: a wave holds its kHold x 64 items of a sub-chunk in
    // registers as (digit, rank inside the wave's share) between (A) and (C),
    // so (C) neither reads them again nor repeats the ballots.
    constexpr int kHold = 8;
    constexpr uint32_t kSub = kHold * 64u * kSortWaves;  // items per sub-chunk
    static_assert(kPlanChunk % kSub == 0, "sub-chunks tile the workgroup's chunks");
    static_assert(kHold * 64u <= (1u << (32 - kSortBinLg)) - 1u, "rank and digit share a register");
    const uint64_t w0 = static_cast<uint64_t>(w) * p.cpw * kPlanChunk;
    uint64_t w1 = w0 + static_cast<uint64_t>(p.cpw) * kPlanChunk;
    if (w1 > items) w1 = items;
    for (uint64_t c0 = w0; c0 < w1; c0 += kSub) {
      const uint64_t i0 = c0 + static_cast<uint64_t>(wave) * (kHold * 64u);
      uint32_t held[kHold];
#pragma unroll
      for (int q = 0; q < kHold; q++) {
        const uint64_t j = i0 + 64u * q + lane;
        const uint32_t key = j < w1 ? p.keys_in[j] : kPlanNoFile;
        const uint32_t d = plan_digit(key, p.shift);
        const bool active = key != kPlanNoFile;
        held[q] = rank_held(cnt[wave], d, active, plan_peers(d, active, false));
      }
      __syncthreads();
      spread();
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kHold; q++) {
        if (held[q] == kSortNoItem) continue;
        const uint64_t j = i0 + 64u * q + lane;
        const uint64_t pos = held_pos(held[q], off[wave], start);
        const uint32_t val = SRC == kSrcPairs ? p.vals_in[j] : static_cast<uint32_t>(j);
        if (LAST) {
          if (pos < a.cap) a.gets[pos] = val;
          if (p.keys_out && pos < a.pair_items) p.keys_out[pos] = p.keys_in[j];
        } else if (pos < a.pair_items) {
          p.keys_out[pos] = p.keys_in[j];
          p.vals_out[pos] = val;
        }
      }
    }
    return;
  }
  for (uint64_t c = static_cast<uint64_t>(w) * p.cpw; c < static_cast<uint64_t>(w + 1) * p.cpw; c++) {
    const uint64_t c0 = c * kPlanChunk;
    if (c0 >= items) break;
    const WaveShare sh = wave_share<kPlanChunk>(c0, wave, items);
    walk<SRC, ALL>(a, p, sh.i0, sh.i1, lane, unused, count);
    __syncthreads();
    spread();
    __syncthreads();
    walk<SRC, ALL>(a, p, sh.i0, sh.i1, lane, unused, place);
  }
}

// file_begin of a plan of several passes: thread f finds the first position
// of the sorted file ids that holds an id >= f.
__global__ __launch_bounds__(kBlock) void plan_bounds_kernel(ReadPlanDev a, const uint32_t* keys) {
  const uint64_t f = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (f > a.n_files) return;
  uint64_t total = *a.total;
  if (total > a.pair_items) total = a.pair_items;
  uint64_t lo = 0, hi = total;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < f) lo = mid + 1;
    else hi = mid;
  }
  a.file_begin[f] = lo;
}

// mask[i] = hit[i] ? 0 : mask[i] & (mask[i] - 1); two Gets per thread (16 B).
__global__ __launch_bounds__(kBlock) void masks_advance_kernel(uint64_t* mask, const uint8_t* hit, uint64_t n) {
  const uint64_t i = 2 * (static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x);
  if (i >= n) return;
  if (i + 1 < n && (reinterpret_cast<uintptr_t>(mask) & 15u) == 0) {
    ulonglong2 m = *reinterpret_cast<ulonglong2*>(mask + i);
    m.x = hit[i] ? 0 : m.x & (m.x - 1);
    m.y = hit[i + 1] ? 0 : m.y & (m.y - 1);
    *reinterpret_cast<ulonglong2*>(mask + i) = m;
    return;
  }
  for (uint64_t j = i; j < n && j < i + 2; j++) {
    const uint64_t m = mask[j];
    mask[j] = hit[j] ? 0 : m & (m - 1);
  }
}

}  // namespace

hipError_t launch_read_plan_pass(const ReadPlanDev& a, int pass, int passes, uint32_t shift, uint32_t cpw,
                                 uint32_t nwg, uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out,
                                 uint32_t* vals_out, hipStream_t s) {
  if (nwg == 0 || nwg > kSortMaxWgs || cpw == 0) return hipErrorInvalidValue;
  const PlanPassDev p{shift, cpw, nwg, keys_in, vals_in, keys_out, vals_out};
  const bool last = pass + 1 == passes;
  const dim3 grid(nwg), block(kSortBlock);
  if (pass == 0) {
    if (a.all) hipLaunchKernelGGL((plan_hist_kernel<kSrcMasks, true>), grid, block, 0, s, a, p);
    else hipLaunchKernelGGL((plan_hist_kernel<kSrcMasks, false>), grid, block, 0, s, a, p);
  } else {
    hipLaunchKernelGGL((plan_hist_kernel<kSrcPairs, false>), grid, block, 0, s, a, p);
  }
  hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(kSortScanBlock), 0, s, a, nwg, passes == 1 ? 1 : 0,
                     pass == 0 ? 1 : 0);
#define DLSM_PLAN_SCATTER(SRC, ALL)                                                                   \
  do {                                                                                                \
    if (last) hipLaunchKernelGGL((plan_scatter_kernel<SRC, ALL, true>), grid, block, 0, s, a, p);     \
    else hipLaunchKernelGGL((plan_scatter_kernel<SRC, ALL, false>), grid, block, 0, s, a, p);         \
  } while (0)
  if (pass > 0) DLSM_PLAN_SCATTER(kSrcPairs, false);
  else if (a.all) DLSM_PLAN_SCATTER(kSrcMasks, true);
  else DLSM_PLAN_SCATTER(kSrcIds, false);
#undef DLSM_PLAN_SCATTER
  return hipGetLastError();
}

hipError_t launch_read_plan_bounds(const ReadPlanDev& a, const uint32_t* keys_sorted, hipStream_t s) {
  const uint64_t threads = static_cast<uint64_t>(a.n_files) + 1;
  hipLaunchKernelGGL(plan_bounds_kernel, dim3(static_cast<uint32_t>((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     s, a, keys_sorted);
  return hipGetLastError();
}

hipError_t launch_masks_advance(uint64_t* mask, const uint8_t* hit, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t threads = (n + 1) / 2;
  hipLaunchKernelGGL(masks_advance_kernel, dim3(static_cast<uint32_t>((threads + kBlock - 1) / kBlock)), dim3(kBlock),
                     0, s, mask, hit, n);
  return hipGetLastError();
}

}  // namespace dlsm
