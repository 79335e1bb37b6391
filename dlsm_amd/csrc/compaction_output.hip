// dlsm_amd/csrc/compaction_output.hip -- every output table of a compaction from
// the run its merge left on the device (dlsm_compaction_output_dev).  The rules
// are the DLSM_HD functions of compaction_output.h and table_build.h; this file
// is the work split.  Eight launches whatever the run and the file count are,
// ordered by the stream alone: the pair count is read from `merged` on the
// device, no counter is shared between workgroups and nothing looks back.
//
// Size, offsets (co_size_kernel, co_offsets_kernel): the table build's passes on
// a grid sized by pair_cap; off[] runs over the whole run.
//
// Cut (co_cut_kernel): one workgroup.  Wave 0 walks the cut chain, a 64-ary
// search of off[] per file; then the workgroup scans the files' padded lengths
// into data_base[] and the files' span counts into the region write's span
// table.  The cut table (u32 first pair per file) goes to the workspace.
//
// Entries (co_entries_kernel), two kinds of workgroup:
//   walkers      a wave per file counts that file's chunks: the F chains run
//                side by side, each linear in its own file's chunks;
//   the rest     a thread per pair: the file from a search of the cut table in
//                LDS, the entry length with the handle relative to the file's
//                start, scanned per workgroup.
//
// Region (co_region_kernel), four kinds:
//   0            per file: entry bytes from the scanned lengths at the cuts,
//                index_base / chunk_base / span and seal part tables, the file
//                records, `built`;
//   starts       es[], the restart values, relative to the file's first entry;
//   walkers      the chains again, now writing chunk_end at chunk_base[f];
//   the rest     the region write: a persistent grid over the files' spans of
//                kTbSpan bytes.  A span belongs to one file (files are MiBs, a
//                span 64 KiB: per-file spans lose under one span per file and
//                keep tb_region_unit's window unchanged, with offsets relative
//                to the file).  Keys and values of one length each take the
//                pair of a byte from a division and stage nothing.
//
// Index (co_index_kernel): tb_index_kernel's tile over the files' spans of
// kTbIndexSpan content bytes.
//
// Seal (co_seal_parts_kernel, co_seal_finish_kernel): crc32c of every block
// that fits (crc32c_dev.h), their 32 KiB parts one flat list found through the
// part table the region launch left; a thread per file folds its parts and
// writes the trailer.
//
// The workgroup sums, scans and the 64-ary search are wg_scan.h's.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"
#include "crc32c_dev.h"
#include "sort_pass.h"
#include "wg_scan.h"

namespace dlsm {
namespace {

constexpr int kCoBlock = 1024;  // threads of every kernel here but the seal's
constexpr int kCoWaves = kCoBlock / 64;
constexpr uint32_t kCoWalkWgs = kCoMaxFiles / kCoWaves;  // a wave per file
constexpr int kCoUnits = kTbSpan / (16 * kCoBlock);      // units per lane and span
constexpr int kCoSealBlock = 256;
constexpr int kCoSealPasses = kCoSealPieces / kCoSealBlock;
static_assert(kTbChunk == kCoBlock && kTbWindow + 1 == kCoBlock, "a thread per pair of a chunk and per offset of a window");
static_assert(kTbSpan % (16 * kCoBlock) == 0, "every lane owns the same number of units of a span");
static_assert(kTbIndexSpan / 16 <= kCoBlock && kTbIndexWindow <= kCoBlock, "a thread per unit and per entry of an index span");
static_assert(kCoMaxFiles % kCoBlock == 0 && kSortMaxWgs <= kCoBlock, "the per-file and per-workgroup scans");
static_assert(kCoSealPieces % kCoSealBlock == 0, "whole passes per part");

// tot[]: what the launches hand on
enum { kTotN, kTotFlags, kTotFiles, kTotNf, kTotData, kTotRegionSpans, kTotIndexSpans, kTotParts, kTotFinal };

// The run's pair count as `merged` on the device gives it; 0 and *flagged where
// the run is not a whole run or does not fit the grids.
__device__ __forceinline__ uint64_t co_pairs(const CoDev& a, bool* flagged) {
  const uint64_t n_out = a.merged[1], flags = a.merged[4];
  *flagged = flags != 0 || n_out > a.pair_cap;
  return *flagged ? 0 : n_out;
}

__global__ __launch_bounds__(kCoBlock) void co_size_kernel(CoDev a) {
  __shared__ uint64_t sh[kCoWaves];
  bool flagged;
  const uint64_t n = co_pairs(a, &flagged);
  uint64_t sum = 0;
  int shortk = 0, big = 0;
  const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    const uint64_t i = c * kTbChunk + threadIdx.x;
    if (i >= n) break;
    const uint64_t ks = a.src.key_size(i), vs = a.src.value_size(i), p = tb_pair_size(ks, vs);
    shortk |= ks < 8;
    big |= ks > 0xffffffffull || vs > 0xffffffffull || p > 0xffffffffull;
    sum += p;
  }
  sum = block_sum<kCoWaves>(sum, sh);
  shortk = __syncthreads_or(shortk);
  big = __syncthreads_or(big);
  if (threadIdx.x == 0) {
    a.wg_sum[blockIdx.x] = sum;
    a.wg_flags[blockIdx.x] = (shortk ? kTbShortKey : 0) | (big ? kTbPairTooBig : 0);
  }
}

__global__ __launch_bounds__(kCoBlock) void co_offsets_kernel(CoDev a) {
  __shared__ uint64_t sh[kCoWaves];
  bool flagged;
  const uint64_t n = co_pairs(a, &flagged);
  uint64_t below = 0;
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += kCoBlock) below += a.wg_sum[j];
  uint64_t run = block_sum<kCoWaves>(below, sh);
  if (blockIdx.x == 0) {
    uint64_t total = 0;
    int shortk = 0, big = 0;
    for (uint32_t j = threadIdx.x; j < a.nwg; j += kCoBlock) {
      total += a.wg_sum[j];
      shortk |= (a.wg_flags[j] & kTbShortKey) != 0;
      big |= (a.wg_flags[j] & kTbPairTooBig) != 0;
    }
    total = block_sum<kCoWaves>(total, sh);
    shortk = __syncthreads_or(shortk);
    big = __syncthreads_or(big);
    if (threadIdx.x == 0) {
      a.off[n] = total;
      a.tot[kTotN] = n;
      a.tot[kTotFlags] = (shortk ? kTbShortKey : 0) | (big ? kTbPairTooBig : 0) | (flagged ? kCoInputFlagged : 0);
    }
  }
  const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    if (c * kTbChunk >= n) break;  // (the same for every thread)
    const uint64_t i = c * kTbChunk + threadIdx.x;
    const uint64_t p = i < n ? tb_pair_size(a.src.key_size(i), a.src.value_size(i)) : 0;
    uint64_t all;
    const uint64_t o = run + block_scan<uint64_t, kCoWaves>(p, sh, &all);
    if (i < n) a.off[i] = o;
    run += all;
  }
}

__global__ __launch_bounds__(kCoBlock) void co_cut_kernel(CoDev a) {
  __shared__ uint64_t sh[kCoWaves];
  __shared__ uint32_t scut[kCoMaxFiles + 1];
  __shared__ uint64_t sinfo[2];  // the file count, the padded bytes of the files past the table
  const uint64_t n = a.tot[kTotN];
  const uint64_t* off = a.off;
  if (threadIdx.x < 64) {  // one wave walks the chain
    uint64_t files = 0, extra = 0;
    if (!(a.tot[kTotFlags] & (kTbMalformed | kCoInputFlagged))) {
      for (uint64_t at = 0; at < n; files++) {
        uint64_t next = n;
        if (a.max_file_bytes) {
          const uint64_t lim = co_cut_limit(off[at], a.max_file_bytes);
          next = at + 1 + wave_last_le([&](uint64_t i) { return off[at + i]; }, n - at + 1, lim - 1);
          next = next < n ? next : n;
        }
        if (files <= kCoMaxFiles) {
          if (threadIdx.x == 0) scut[files] = static_cast<uint32_t>(at);
        }
        if (files >= kCoMaxFiles) extra += co_pad16(off[next] - off[at]);
        at = next;
      }
      if (files <= kCoMaxFiles && threadIdx.x == 0) scut[files] = static_cast<uint32_t>(n);
    }
    if (threadIdx.x == 0) {
      sinfo[0] = files;
      sinfo[1] = extra;
    }
  }
  __syncthreads();
  const uint64_t files = sinfo[0];
  const uint32_t nf = static_cast<uint32_t>(files < kCoMaxFiles ? files : kCoMaxFiles);
  uint64_t drun = 0, srun = 0;
  for (uint32_t f0 = 0; f0 < nf; f0 += kCoBlock) {
    const uint32_t f = f0 + threadIdx.x;
    const uint64_t bytes = f < nf ? off[scut[f + 1]] - off[scut[f]] : 0;
    uint64_t dall, sall;
    const uint64_t base = drun + block_scan<uint64_t, kCoWaves>(co_pad16(bytes), sh, &dall);
    const uint64_t lim = bytes < co_left(a.data_cap, base) ? bytes : co_left(a.data_cap, base);
    const uint64_t sp = srun + block_scan<uint64_t, kCoWaves>((lim + kTbSpan - 1) / kTbSpan, sh, &sall);
    if (f < nf) {
      a.cut[f] = scut[f];
      a.data_base[f] = base;
      a.rspan[f] = static_cast<uint32_t>(sp);
    }
    drun += dall;
    srun += sall;
  }
  if (threadIdx.x == 0) {
    a.cut[nf] = nf ? scut[nf] : 0;
    a.data_base[nf] = drun;
    a.rspan[nf] = static_cast<uint32_t>(srun);
    a.tot[kTotFiles] = files;
    a.tot[kTotNf] = nf;
    a.tot[kTotData] = drun + sinfo[1];
    a.tot[kTotRegionSpans] = srun;
  }
}

// File f's chunk chain in one wave (tb_finish's walk between the file's cuts,
// the ends relative to the file's start).  Ends go to chunk_end[base + c] below
// chunk_cap where write is set.  Returns the chunk count.
__device__ __forceinline__ uint64_t co_chain(const CoDev& a, uint32_t f, bool write, uint64_t base, bool* oversize) {
  const uint64_t* off = a.off;
  const uint64_t b = a.cut[f], e = a.cut[f + 1], ob = off[b];
  const bool lane0 = (threadIdx.x & 63) == 0;
  *oversize = false;
  if (a.chunk_bytes == 0) {
    if (write && lane0 && base < a.chunk_cap) a.chunk_end[base] = off[e] - ob;
    return 1;
  }
  uint64_t nch = 0;
  for (uint64_t at = b; at < e; nch++) {
    const uint64_t lim = tb_chunk_limit(off[at], a.chunk_bytes);
    uint64_t next = at + 1;
    if (off[at + 1] > lim) *oversize = true;
    else next += wave_last_le([&](uint64_t i) { return off[at + 1 + i]; }, e - at, lim);
    if (write && lane0 && base + nch < a.chunk_cap) a.chunk_end[base + nch] = off[next] - ob;
    at = next;
  }
  return nch;
}

// The cut table into LDS: nf + 1 values.
__device__ __forceinline__ void co_stage_cut(const CoDev& a, uint32_t nf, uint32_t* scut) {
  for (uint32_t f = threadIdx.x; f <= nf; f += kCoBlock) scut[f] = a.cut[f];
  __syncthreads();
}

__global__ __launch_bounds__(kCoBlock) void co_entries_kernel(CoDev a) {
  __shared__ uint64_t sh[kCoWaves];
  __shared__ uint32_t scut[kCoMaxFiles + 1];
  const uint32_t nf = static_cast<uint32_t>(a.tot[kTotNf]);
  if (blockIdx.x < kCoWalkWgs) {
    const uint32_t f = blockIdx.x * kCoWaves + (threadIdx.x >> 6);
    if (f >= nf) return;
    bool oversize;
    const uint64_t nch = co_chain(a, f, false, 0, &oversize);
    if ((threadIdx.x & 63) == 0) {
      a.nch[f] = static_cast<uint32_t>(nch);
      a.fflag[f] = oversize ? static_cast<uint32_t>(kTbOversizePair) : 0;
    }
    return;
  }
  const uint32_t w = blockIdx.x - kCoWalkWgs;
  co_stage_cut(a, nf, scut);
  const uint64_t n = nf ? scut[nf] : 0;  // the pairs that have a file
  const uint64_t* off = a.off;
  uint64_t erun = 0;
  const uint64_t c0 = static_cast<uint64_t>(w) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    if (c * kTbChunk >= n) break;  // (the same for every thread)
    const uint64_t i = c * kTbChunk + threadIdx.x;
    uint64_t e = 0;
    if (i < n) {
      const uint64_t o = off[i], ob = off[scut[co_file_of(scut, nf, i)]];
      e = tb_entry_len(a.src.key_size(i), o - ob, off[i + 1] - o);
    }
    uint64_t eall;
    const uint64_t r = erun + block_scan<uint64_t, kCoWaves>(e, sh, &eall);
    if (i < n) a.erel[i] = r;
    erun += eall;
  }
  if (threadIdx.x == 0) a.wg_esum[w] = erun;
}

// The entry bytes of the workgroups below each entries workgroup into swg; the
// sum of all in every thread.
__device__ __forceinline__ uint64_t co_stage_esum(const CoDev& a, uint64_t* swg, uint64_t* sh) {
  uint64_t all;
  const uint64_t x = block_scan<uint64_t, kCoWaves>(threadIdx.x < a.nwg ? a.wg_esum[threadIdx.x] : 0, sh, &all);
  if (threadIdx.x < a.nwg) swg[threadIdx.x] = x;
  __syncthreads();
  return all;
}

// Workgroup 0 of the region launch: the per-file tables, the records, `built`.
__device__ __forceinline__ void co_finish(const CoDev& a, uint64_t* sh, uint32_t* scut, uint64_t* swg) {
  const uint32_t nf = static_cast<uint32_t>(a.tot[kTotNf]);
  const uint64_t files = a.tot[kTotFiles];
  uint64_t flags = a.tot[kTotFlags];
  const uint64_t E_all = co_stage_esum(a, swg, sh);
  co_stage_cut(a, nf, scut);
  const uint64_t n = nf ? scut[nf] : 0, per = static_cast<uint64_t>(a.cpw) * kTbChunk;
  const uint64_t* off = a.off;
  auto G = [&](uint64_t i) { return i >= n ? E_all : swg[i / per] + a.erel[i]; };  // the entry bytes in front of pair i
  uint64_t irun = 0, crun = 0, srun = 0, prun = 0;
  int toobig = 0, oversize = 0;
  for (uint32_t f0 = 0; f0 < nf; f0 += kCoBlock) {
    const uint32_t f = f0 + threadIdx.x;
    const bool in = f < nf;
    const uint64_t b = in ? scut[f] : 0, e = in ? scut[f + 1] : 0, fn = e - b;
    const uint64_t E = in ? G(e) - G(b) : 0, ctot = E + 4 * fn + 4, ib = ctot + 5;
    const uint64_t nch = in ? a.nch[f] : 0;
    uint64_t iall, call, sall, pall;
    const uint64_t ibase = irun + block_scan<uint64_t, kCoWaves>(in ? co_pad16(ib) : 0, sh, &iall);
    const uint64_t cbase = crun + block_scan<uint64_t, kCoWaves>(nch, sh, &call);
    const uint64_t left = co_left(a.index_cap, ibase), lim = ctot < left ? ctot : left;
    const bool fits = in && ib <= left;
    const uint64_t sp = srun + block_scan<uint64_t, kCoWaves>(in ? (lim + kTbIndexSpan - 1) / kTbIndexSpan : 0, sh, &sall);
    const uint64_t pt = prun + block_scan<uint64_t, kCoWaves>(fits ? co_seal_parts(ctot) : 0, sh, &pall);
    if (in) {
      const uint32_t ff = a.fflag[f];
      toobig |= ctot > 0xffffffffull;
      oversize |= ff != 0;
      a.fE[f] = E;
      a.index_base[f] = ibase;
      a.ispan[f] = static_cast<uint32_t>(sp);
      a.part0[f] = static_cast<uint32_t>(pt);
      a.seal_len[f] = fits ? ctot : 0;
      a.es[co_es_base(b, f) + fn] = static_cast<uint32_t>(fn);
      a.es[co_es_base(b, f) + fn + 1] = 0;
      if (f < a.file_cap)
        a.files[f] = CoFile{b, fn, a.data_base[f], off[e] - off[b], ibase, ib, cbase, nch, ff};
    }
    irun += iall;
    crun += call;
    srun += sall;
    prun += pall;
  }
  toobig = __syncthreads_or(toobig);
  oversize = __syncthreads_or(oversize);
  if (threadIdx.x) return;
  const uint64_t data = a.tot[kTotData];
  if (toobig) flags |= kTbIndexTooBig;
  const bool bad = (flags & (kTbMalformed | kCoInputFlagged)) != 0;
  if (!bad) {
    flags |= (oversize ? kTbOversizePair : 0) | (data > a.data_cap ? kTbDataCap : 0) | (irun > a.index_cap ? kTbIndexCap : 0) |
             (crun > a.chunk_cap ? kTbChunkCap : 0) | (files > a.file_cap || files > kCoMaxFiles ? kCoFileCap : 0);
  }
  a.ispan[nf] = static_cast<uint32_t>(srun);
  a.part0[nf] = static_cast<uint32_t>(prun);
  a.tot[kTotIndexSpans] = bad ? 0 : srun;
  a.tot[kTotParts] = bad ? 0 : prun;
  a.tot[kTotFinal] = flags;
  a.built[0] = bad ? 0 : files;
  a.built[1] = bad ? 0 : data;
  a.built[2] = bad ? 0 : irun;
  a.built[3] = bad ? 0 : crun;
  a.built[4] = flags;
}

// Workgroups 1 .. nwg: the restart values of entries workgroup w's pairs.
__device__ __forceinline__ void co_starts(const CoDev& a, uint32_t w, uint64_t* sh, uint32_t* scut, uint64_t* swg) {
  const uint32_t nf = static_cast<uint32_t>(a.tot[kTotNf]);
  co_stage_esum(a, swg, sh);
  co_stage_cut(a, nf, scut);
  const uint64_t n = nf ? scut[nf] : 0, per = static_cast<uint64_t>(a.cpw) * kTbChunk;
  const uint64_t c0 = static_cast<uint64_t>(w) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    const uint64_t i = c * kTbChunk + threadIdx.x;
    if (i >= n) break;
    const uint32_t f = co_file_of(scut, nf, i);
    const uint64_t b = scut[f];
    a.es[co_es_base(b, f) + (i - b)] = static_cast<uint32_t>(swg[w] + a.erel[i] - (swg[b / per] + a.erel[b]));
  }
}

// The last f in [0, nf) with t[f] <= s (t[0] = 0): the file of span or part s.
__device__ __forceinline__ uint32_t co_table_file(const uint32_t* t, uint32_t nf, uint64_t s) {
  return co_file_of(t, nf, s);
}

template <class A>
__device__ __forceinline__ void co_region_span(const A& v, uint64_t n, uint64_t p0, uint64_t p1, uint8_t* __restrict__ out) {
#pragma unroll
  for (int k = 0; k < kCoUnits; k++) {
    const uint64_t u = p0 + (static_cast<uint64_t>(k) * kCoBlock + threadIdx.x) * 16;
    if (u < p1) tb_region_unit(v, n, u, p1, out + u);
  }
}

template <bool kFixed>
__global__ __launch_bounds__(kCoBlock) void co_region_kernel(CoDev a) {
  __shared__ uint64_t sh[kCoWaves];
  __shared__ uint32_t scut[kCoMaxFiles + 1];
  __shared__ uint64_t swg[kSortMaxWgs];
  __shared__ uint64_t soff[kTbWindow + 1];
  __shared__ uint64_t sks[kTbWindow + 1];
  __shared__ uint64_t svs[kTbWindow + 1];
  __shared__ uint32_t skl[kTbWindow + 1];
  if (blockIdx.x == 0) return co_finish(a, sh, scut, swg);
  if (blockIdx.x <= a.nwg) return co_starts(a, blockIdx.x - 1, sh, scut, swg);
  const uint32_t nf = static_cast<uint32_t>(a.tot[kTotNf]);
  if (blockIdx.x <= a.nwg + kCoWalkWgs) {
    const uint32_t f = (blockIdx.x - 1 - a.nwg) * kCoWaves + (threadIdx.x >> 6);
    if (f >= nf) return;
    uint64_t below = 0;
    for (uint32_t j = threadIdx.x & 63; j < f; j += 64) below += a.nch[j];
    bool oversize;
    co_chain(a, f, true, wave_sum(below), &oversize);
    return;
  }
  const uint32_t wg = blockIdx.x - 1 - a.nwg - kCoWalkWgs;
  const uint64_t spans = a.tot[kTotRegionSpans];
  const uint64_t per = (spans + a.copy_wgs - 1) / a.copy_wgs;
  const uint64_t s0 = per * wg;
  const uint64_t s1 = s0 + per < spans ? s0 + per : spans;
  if (s0 >= s1) return;
  const uint64_t* off = a.off;
  uint32_t f = co_table_file(a.rspan, nf, s0);
  bool fresh = true;  // the file's values below are to be loaded
  uint64_t b = 0, fn = 0, ob = 0, limit = 0, first = 0;
  uint8_t* out = nullptr;
  const TbWindowView win{soff, sks, svs, skl};
  for (uint64_t s = s0; s < s1; s++) {
    while (s >= a.rspan[f + 1]) {  // (s < spans = rspan[nf]: f stays below nf)
      f++;
      fresh = true;
    }
    if (fresh) {
      b = a.cut[f];
      fn = a.cut[f + 1] - b;
      ob = off[b];
      const uint64_t bytes = off[b + fn] - ob, base = a.data_base[f], left = co_left(a.data_cap, base);
      limit = bytes < left ? bytes : left;
      out = a.data + base;
    }
    const uint64_t p0 = (s - a.rspan[f]) * kTbSpan;
    const uint64_t p1 = p0 + kTbSpan < limit ? p0 + kTbSpan : limit;
    if (kFixed) {
#pragma unroll
      for (int k = 0; k < kCoUnits; k++) {
        const uint64_t u = p0 + (static_cast<uint64_t>(k) * kCoBlock + threadIdx.x) * 16;
        if (u < p1) co_region_unit_fixed(a.src, b, u, p1, out + u);
      }
      fresh = false;
      continue;
    }
    const CoFileView view{a.src, b, ob};
    auto at = [&](uint64_t i) { return view.at(i); };
    if (fresh) first = wave_last_le(at, fn, p0);  // p0 < limit <= at(fn), at(0) = 0
    fresh = false;
    const uint64_t idx = first + threadIdx.x;
    const uint64_t o = idx <= fn ? view.at(idx) : ~uint64_t(0);
    soff[threadIdx.x] = o;
    if (idx < fn && o < p1) {
      sks[threadIdx.x] = view.key_src(idx);
      svs[threadIdx.x] = view.value_src(idx);
      skl[threadIdx.x] = static_cast<uint32_t>(view.key_size(idx));
    }
    __syncthreads();
    const uint64_t last = soff[kTbWindow];
    if (last >= p1) co_region_span(win, kTbWindow, p0, p1, out);
    else co_region_span(view, fn, p0, p1, out);
    if (p1 < limit)  // the file's next span: its first pair
      first = last > p1 ? first + tb_last_le(win, kTbWindow, p1) : wave_last_le(at, fn, p1);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kCoBlock) void co_index_kernel(CoDev a) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTbIndexSpan];
  __shared__ int64_t wat[kTbIndexWindow];   // the entry's first byte relative to the span
  __shared__ uint64_t wsrc[kTbIndexWindow];  // its key
  __shared__ uint32_t wkl[kTbIndexWindow];   // ... and the key's length
  __shared__ uint32_t whd[kTbIndexWindow];   // the bytes in front of the key
  constexpr int64_t kNone = INT64_MAX;
  const uint64_t spans = a.tot[kTotIndexSpans];  // (0 with a malformed bit)
  const uint32_t nf = static_cast<uint32_t>(a.tot[kTotNf]);
  const uint64_t per = (spans + gridDim.x - 1) / gridDim.x;
  const uint64_t s0 = per * blockIdx.x;
  const uint64_t s1 = s0 + per < spans ? s0 + per : spans;
  if (s0 >= s1) return;
  const uint64_t* off = a.off;
  uint32_t f = co_table_file(a.ispan, nf, s0);
  for (uint64_t s = s0; s < s1; s++) {
    while (s >= a.ispan[f + 1]) f++;  // (s < spans = ispan[nf])
    const uint64_t b = a.cut[f], n = a.cut[f + 1] - b, ob = off[b], E = a.fE[f], ctot = E + 4 * n + 4;
    const uint64_t base = a.index_base[f], left = co_left(a.index_cap, base);
    const uint64_t limit = ctot < left ? ctot : left;
    const uint32_t* es = a.es + co_es_base(b, f);
    uint8_t* out = a.index + base;
    const uint64_t q0 = (s - a.ispan[f]) * kTbIndexSpan;
    const uint64_t q1 = q0 + kTbIndexSpan < limit ? q0 + kTbIndexSpan : limit;
    if (q0 < E) {  // the span's entries into the tile
      const uint64_t qe = q1 < E ? q1 : E;
      const int64_t len = static_cast<int64_t>(qe - q0);
      const uint64_t first = wave_last_le([&](uint64_t i) { return static_cast<uint64_t>(es[i]); }, n, q0);
      if (threadIdx.x < kTbIndexWindow) {
        const uint64_t idx = first + threadIdx.x;
        int64_t at = kNone;
        if (idx < n && es[idx] < qe) {
          const uint64_t ks = a.src.key_size(b + idx), o = off[b + idx], size = off[b + idx + 1] - o;
          at = static_cast<int64_t>(es[idx]) - static_cast<int64_t>(q0);
          tb_entry_write(tile, len, at, ks, o - ob, size);
          wsrc[threadIdx.x] = a.src.key_src(b + idx);
          wkl[threadIdx.x] = static_cast<uint32_t>(ks);
          whd[threadIdx.x] = tb_entry_head(ks);
        }
        wat[threadIdx.x] = at;
      }
      __syncthreads();
      const uint32_t l = threadIdx.x & 31;
      for (uint32_t j = threadIdx.x >> 5; j < kTbIndexWindow; j += kCoBlock / 32) {
        const int64_t at = wat[j];
        if (at == kNone) break;  // the starts ascend: none follows
        const int64_t k0 = at + whd[j];
        const uint32_t kl = wkl[j];
        const kv_src1 key = reinterpret_cast<kv_src1>(wsrc[j]);
        for (uint32_t x = l; x < kl; x += 32) {
          const int64_t pos = k0 + x;
          if (pos >= 0 && pos < len) tile[pos] = key[x];
        }
      }
      __syncthreads();
    }
    if (threadIdx.x < kTbIndexSpan / 16) {
      const uint64_t q = q0 + 16 * threadIdx.x;
      if (q < q1) tb_index_unit(tile, q0, es, E, ctot, q, limit, out + q);
    }
    __syncthreads();  // the tile is rewritten by the next span
  }
}

// ---- the seal --------------------------------------------------------------
// Part g of the flat list: the raw crc of kCoSealPieces 16-byte pieces of one
// block's contents, zero pieces in front of a block's first part.
__global__ __launch_bounds__(kCoSealBlock) void co_seal_parts_kernel(CoDev a, crc32c::XPow xp) {
  __shared__ uint32_t T[1024];
  __shared__ uint32_t wv[kCoSealBlock / 64];
  const uint32_t g = blockIdx.x;
  if (g >= a.tot[kTotParts]) return;
  const uint32_t nf = static_cast<uint32_t>(a.tot[kTotNf]);
  const uint32_t f = co_table_file(a.part0, nf, g);
  const uint32_t part = g - a.part0[f];
  const uint64_t ctot = a.seal_len[f];
  const int64_t pieces = static_cast<int64_t>(ctot / 16);
  const int64_t lead = static_cast<int64_t>(co_seal_parts(ctot)) * kCoSealPieces - pieces;
  const uint8_t* src = a.index + a.index_base[f];
  {  // the slice-by-4 tables (the header's table build, written out like the fold below)
    uint32_t c = threadIdx.x;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ crc32c::kPoly : (c >> 1);
    T[threadIdx.x] = c;
    __syncthreads();
    for (int t = 1; t < 4; t++) {
      const uint32_t prev = T[256 * (t - 1) + threadIdx.x];
      T[256 * t + threadIdx.x] = (prev >> 8) ^ T[prev & 0xffu];
      __syncthreads();
    }
  }
  uint4 v[kCoSealPasses];
#pragma unroll
  for (int i = 0; i < kCoSealPasses; i++) {
    const int64_t q = static_cast<int64_t>(part) * kCoSealPieces + i * kCoSealBlock + threadIdx.x - lead;
    v[i] = q < 0 ? make_uint4(0, 0, 0, 0) : *reinterpret_cast<const uint4*>(src + 16 * q);  // q < pieces
  }
  // crc32c::part_fold, written out: through the shared functions the seal of a
  // hundred files measured one percent slower (crc32c_dev.h)
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < kCoSealPasses; i++) {
    uint32_t r = crc32c::raw_word(0, v[i].x, T);
    r = crc32c::raw_word(r, v[i].y, T);
    r = crc32c::raw_word(r, v[i].z, T);
    r = crc32c::raw_word(r, v[i].w, T);
    acc = crc32c::mulmod(acc, xp.p[15]) ^ r;  // a pass is 4 KiB = 2^15 bits
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; k++) {  // level k joins neighbours of 16 * 2^k bytes
    const uint32_t other = __shfl_xor(acc, 1 << k, 64);
    if ((lane & (1 << k)) == 0) acc = crc32c::mulmod(acc, xp.p[k + 7]) ^ other;
  }
  if (lane == 0) wv[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int q2 = 0; q2 < kCoSealBlock / 64; q2++) s = crc32c::mulmod(s, xp.p[13]) ^ wv[q2];  // a wave is 1 KiB
    a.partial[g] = s;
  }
}
static_assert(kCoSealBlock == 256 && kCoSealPasses * kCoSealBlock * 16 == 32768, "the seal's fold constants");

// A thread per file: fold the parts, append the bytes behind the last piece and
// the type byte, write the trailer.
__global__ void co_seal_finish_kernel(CoDev a, crc32c::XPow xp) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (a.tot[kTotParts] == 0 || f >= a.tot[kTotNf]) return;
  const uint64_t ctot = a.seal_len[f];
  if (ctot == 0) return;  // the block does not fit: no trailer
  uint8_t* blk = a.index + a.index_base[f];
  uint32_t raw = 0;
  for (uint32_t p = a.part0[f]; p < a.part0[f + 1]; p++) raw = crc32c::mulmod(raw, xp.p[18]) ^ a.partial[p];  // 32 KiB
  for (uint64_t d = ctot / 16 * 16; d < ctot; d++) raw = crc32c::raw_byte(raw, blk[d]);
  raw = crc32c::raw_byte(raw, 0);  // kNoCompression
  // crc32c::value and store_trailer, written out as the parts kernel's fold is
  uint32_t xn = 0x80000000u;  // x^(8 (ctot + 1))
  uint64_t bits = (ctot + 1) << 3;
  for (int k = 0; bits; k++, bits >>= 1)
    if (bits & 1u) xn = crc32c::mulmod(xn, xp.p[k]);
  const uint32_t m = crc32c::mask(~(crc32c::mulmod(0xffffffffu, xn) ^ raw));
  blk[ctot] = 0;
  blk[ctot + 1] = static_cast<uint8_t>(m);
  blk[ctot + 2] = static_cast<uint8_t>(m >> 8);
  blk[ctot + 3] = static_cast<uint8_t>(m >> 16);
  blk[ctot + 4] = static_cast<uint8_t>(m >> 24);
}

}  // namespace

hipError_t launch_compaction_output(const CoDev& a, uint32_t index_wgs, uint32_t seal_wgs, hipEvent_t* ev, hipStream_t s) {
  if (a.nwg == 0 || a.nwg > kSortMaxWgs || a.cpw == 0 || a.copy_wgs == 0 || index_wgs == 0 || seal_wgs == 0)
    return hipErrorInvalidValue;
  static const crc32c::XPow xp = crc32c::make_xpow();
  const bool fixed = !a.src.koff && !a.src.voff;
  hipError_t e;
  auto mark = [&](int j) { return ev ? hipEventRecord(ev[j], s) : hipSuccess; };
  if ((e = mark(0)) != hipSuccess) return e;
  co_size_kernel<<<a.nwg, kCoBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(1)) != hipSuccess) return e;
  co_offsets_kernel<<<a.nwg, kCoBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(2)) != hipSuccess) return e;
  co_cut_kernel<<<1, kCoBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(3)) != hipSuccess) return e;
  co_entries_kernel<<<kCoWalkWgs + a.nwg, kCoBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(4)) != hipSuccess) return e;
  const uint32_t grid = 1 + a.nwg + kCoWalkWgs + a.copy_wgs;
  if (fixed) co_region_kernel<true><<<grid, kCoBlock, 0, s>>>(a);
  else co_region_kernel<false><<<grid, kCoBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(5)) != hipSuccess) return e;
  co_index_kernel<<<index_wgs, kCoBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(6)) != hipSuccess) return e;
  co_seal_parts_kernel<<<seal_wgs, kCoSealBlock, 0, s>>>(a, xp);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  co_seal_finish_kernel<<<kCoMaxFiles / kCoSealBlock, kCoSealBlock, 0, s>>>(a, xp);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return mark(7);
}

}  // namespace dlsm
