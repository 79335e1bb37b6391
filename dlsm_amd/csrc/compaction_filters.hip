// dlsm_amd/csrc/compaction_filters.hip -- the sealed filter block of every file
// a compaction output cut out of a merged run (dlsm_compaction_filters_dev).
// The file boundaries and the duplicate-lowered line counts are known to the
// device alone, so nothing here is planned per file on the host: five launches
// whatever the run and the file count are, sized by pair_cap and file_cap,
// ordered by the stream alone.  No counter is shared between workgroups; the
// only atomics are LDS ranks and ds_or, and no byte written depends on their
// order.
//
// Hash (cf_hash_kernel): a workgroup per chunk of kCfChunk pairs, in four
// sub-tiles of a pair per thread.  A sub-tile's key bytes are one contiguous
// range of the run: it is streamed into LDS in 16-byte units at the alignment
// of its global address, then every lane hashes its key's user part from LDS
// through aligned dword reads and a funnel shift by the key's byte phase.  Keys
// of one length that is a whole number of dwords read whole words at a stride
// of klen / 4 (7 for 28-byte keys: conflict-free).  A sub-tile whose bytes pass
// the tile is hashed from global memory, lane by lane.  The pair's file comes
// from the cut table in LDS: one search per wave, then a walk.  Per pair the
// hash is written; per chunk the count of pairs that count -- a file's first
// pair, or a hash that differs from the pair's before it (the pair across the
// chunk edge is hashed again) -- and per file the count in front of its first
// pair inside that pair's chunk, so the plan needs no recount.
//
// Plan (cf_plan_kernel): one workgroup.  The chunk counts are scanned; file f's
// distinct count is the difference of two (scan + in-chunk count) values; from
// it L, the fastmod magic, the block's length, its base (scan of the padded
// lengths), its slice count and the flat slice prefix sums; the records and
// `built`.
//
// Partition (cf_partition_kernel): a workgroup per chunk.  line = h % L of the
// pair's file, bucketed by flat slice id; the chunk's bins are one contiguous
// id range (cf_bins_bound), ranked through an LDS histogram, each bin padded to
// whole 16-byte units.
//
// Slice (cf_slice_kernel): a workgroup per flat slice.  The file by a uniform
// search of the prefix sums, the slice zeroed in LDS, the file's own chunk
// range walked a wave per chunk, bits set with ds_or (a straight-line unit for
// k = 6), the slice streamed out with 16-byte stores, and its raw crc32c taken
// from LDS (crc32c_dev.h).
//
// Finish (cf_finish_kernel): a thread per file folds its slices' crcs, appends
// the filter's trailer and the type byte and writes both trailers.
//
// The workgroup scans are wg_scan.h's.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"
#include "crc32c_dev.h"
#include "wg_scan.h"

namespace dlsm {
namespace {

constexpr int kCfBlock = 1024;
constexpr int kCfWaves = kCfBlock / 64;
constexpr int kCfSub = kCfChunk / kCfBlock;  // sub-tiles of a chunk: a pair per thread each
constexpr uint32_t kCfTile = 40960;          // key bytes of a sub-tile staged in LDS (40 per key)
constexpr int kCfBinsPer = (kCfMaxBins + kCfBlock) / kCfBlock;  // bins per thread of the partition's scan
constexpr int kCfSliceBlock = 256;
constexpr int kCfSliceWaves = kCfSliceBlock / 64;
static_assert(kCfChunk % kCfBlock == 0 && kCoMaxFiles % kCfSliceBlock == 0, "whole sub-tiles, whole finish workgroups");
static_assert(kCfBinsPer * kCfBlock > kCfMaxBins, "the scan covers every bin");
static_assert(kCfRegion / 4 <= 0xffff, "a chunk's units fit the u16 table");
static_assert(kCfMinLgR >= 6 && (64u << kCfMaxLgR) <= 32768, "the slice's crc split and its LDS");

enum { kTotN, kTotNf, kTotSlices };  // tot[]: what the plan hands on

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The inputs as the device gives them: the cut table into scut (nf + 1 values,
// scut[nf] = n).  False where the run is flagged, does not fit the grids, or
// the records are not the nf files of [0, n) back to back: then nothing of the
// run is touched.
__device__ __forceinline__ bool cf_stage(const CfDev& a, uint32_t* scut, uint64_t* n, uint32_t* nf) {
  const uint64_t n_out = a.merged[1], files = a.built_in[0];
  const bool flagged = a.merged[4] != 0 || n_out > a.pair_cap || (a.built_in[4] & ~kCfBuiltOk) != 0 || files > a.file_cap;
  const uint32_t F = flagged ? 0 : static_cast<uint32_t>(files);
  int broken = flagged || (F == 0 && n_out != 0);
  for (uint32_t f = threadIdx.x; f < F; f += kCfBlock) {
    const uint64_t first = a.files[f].first, cnt = a.files[f].n;
    const uint64_t next = f + 1 < F ? a.files[f + 1].first : n_out;
    broken |= first >= n_out || cnt == 0 || cnt > n_out || first + cnt != next || (f == 0 && first != 0);
    scut[f] = static_cast<uint32_t>(first);
  }
  if (threadIdx.x == 0) scut[F] = static_cast<uint32_t>(n_out);
  broken = __syncthreads_or(broken);
  *n = n_out;
  *nf = F;
  return !broken;
}

// BloomHash of ulen bytes at tile + off in LDS: aligned dwords, shifted by the
// key's byte phase.  The dword behind the last whole word is read too; the
// key's trailer lies there.
__device__ __forceinline__ uint32_t cf_hash_lds(const uint8_t* tile, uint32_t off, uint32_t ulen) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(tile) + (off >> 2);
  const uint32_t sh = (off & 3u) * 8u, nw = ulen >> 2;
  uint32_t h = hash_init(ulen, kBloomSeed);
  if (sh == 0) {
    for (uint32_t j = 0; j < nw; j++) h = hash_word(h, w[j]);
  } else {
    uint32_t lo = w[0];
    for (uint32_t j = 0; j < nw; j++) {
      const uint32_t hi = w[j + 1];
      h = hash_word(h, (lo >> sh) | (hi << (32u - sh)));
      lo = hi;
    }
  }
  const uint8_t* p = tile + off + 4 * nw;
  uint32_t tail = 0;
  for (uint32_t j = 0; j < (ulen & 3u); j++) tail |= static_cast<uint32_t>(p[j]) << (8 * j);
  return hash_tail(h, tail, ulen & 3u);
}

// The same from global memory, byte by byte: a key range too long for the tile
// and the pair in front of a chunk.
__device__ __forceinline__ uint32_t cf_hash_global(const uint8_t* p, uint32_t ulen) {
  uint32_t h = hash_init(ulen, kBloomSeed);
  uint32_t i = 0;
  for (; i + 4 <= ulen; i += 4)
    h = hash_word(h, uint32_t(p[i]) | (uint32_t(p[i + 1]) << 8) | (uint32_t(p[i + 2]) << 16) | (uint32_t(p[i + 3]) << 24));
  uint32_t tail = 0;
  for (uint32_t j = i; j < ulen; j++) tail |= static_cast<uint32_t>(p[j]) << (8 * (j - i));
  return hash_tail(h, tail, ulen - i);
}

template <bool kFixed>
__device__ __forceinline__ uint64_t cf_key_at(const CfDev& a, uint64_t i) {
  return kFixed ? i * a.klen : a.koff[i];
}
// ExtractUserKey's length; a key shorter than its trailer hashes as the empty user key.
__device__ __forceinline__ uint32_t cf_user_len(uint64_t len) { return len >= 8 ? static_cast<uint32_t>(len - 8) : 0; }

template <bool kFixed>
__global__ __launch_bounds__(kCfBlock) void cf_hash_kernel(CfDev a) {
  __shared__ uint32_t scut[kCoMaxFiles + 1];
  __shared__ __attribute__((aligned(16))) uint8_t tile[kCfTile + 48];
  __shared__ uint32_t hh[kCfBlock + 1];  // hh[1 + t]: thread t's hash; hh[0]: the pair's in front of the sub-tile
  __shared__ uint32_t sh[kCfWaves];
  uint64_t n;
  uint32_t nf;
  if (!cf_stage(a, scut, &n, &nf)) return;
  const uint64_t i00 = static_cast<uint64_t>(blockIdx.x) * kCfChunk;
  if (i00 >= n) return;
  const uint32_t t = threadIdx.x;
  if (t == 0) {
    uint32_t before = 0;
    if (i00 > 0) {
      const uint64_t b = cf_key_at<kFixed>(a, i00 - 1);
      before = cf_hash_global(a.kbytes + b, cf_user_len(cf_key_at<kFixed>(a, i00) - b));
    }
    hh[0] = before;
  }
  uint32_t run = 0;  // the chunk's counting pairs in front of the sub-tile
  for (int s = 0; s < kCfSub; s++) {
    const uint64_t i0 = i00 + static_cast<uint64_t>(s) * kCfBlock;
    if (i0 >= n) break;  // (the same for every thread)
    const uint64_t i1 = i0 + kCfBlock < n ? i0 + kCfBlock : n;
    const uint64_t i = i0 + t;
    const bool in = i < i1;
    const uint64_t b0 = cf_key_at<kFixed>(a, i0), b1 = cf_key_at<kFixed>(a, i1);
    const uint64_t kb = in ? cf_key_at<kFixed>(a, i) : b1, ke = in ? cf_key_at<kFixed>(a, i + 1) : b1;
    const uint32_t ulen = cf_user_len(ke - kb);
    uint32_t h = 0;
    if (b1 - b0 <= kCfTile) {  // (the same for every thread)
      const uintptr_t g0 = reinterpret_cast<uintptr_t>(a.kbytes + b0), g1 = reinterpret_cast<uintptr_t>(a.kbytes + b1);
      const uintptr_t u0 = g0 & ~uintptr_t(15);
      const uint32_t units = static_cast<uint32_t>((g1 - u0 + 15) >> 4);
      for (uint32_t u = t; u < units; u += kCfBlock) {
        const uintptr_t p = u0 + 16 * static_cast<uintptr_t>(u);
        uint4 v;
        if (p >= g0 && p + 16 <= g1) {
          const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
          v = make_uint4(x.x, x.y, x.z, x.w);
        } else {  // the range's first and last unit: only the bytes inside it
          uint32_t d[4] = {0, 0, 0, 0};
          for (uint32_t j = 0; j < 16; j++)
            if (p + j >= g0 && p + j < g1) d[j >> 2] |= static_cast<uint32_t>(*reinterpret_cast<const uint8_t*>(p + j)) << (8 * (j & 3));
          v = make_uint4(d[0], d[1], d[2], d[3]);
        }
        *reinterpret_cast<uint4*>(tile + 16 * u) = v;
      }
      __syncthreads();
      if (in) h = cf_hash_lds(tile, static_cast<uint32_t>(g0 - u0 + (kb - b0)), ulen);
    } else if (in) {
      h = cf_hash_global(a.kbytes + kb, ulen);
    }
    hh[t + 1] = h;
    __syncthreads();
    const uint32_t prev = hh[t], last = hh[kCfBlock];
    uint32_t f = 0;
    if (i0 + (t & ~63u) < i1) {  // the wave has a pair: search for its first, walk to the lane's
      f = co_file_of(scut, nf, i0 + (t & ~63u));
      while (in && f + 1 < nf && scut[f + 1] <= i) f++;
    }
    const bool start = in && scut[f] == i;
    const uint32_t counts = in && (start || h != prev);
    if (in) a.hash[i] = h;
    uint32_t all;
    const uint32_t pre = block_scan<uint32_t, kCfWaves>(counts, sh, &all);
    if (start) a.gpre[f] = run + pre;
    run += all;
    if (t == 0) hh[0] = last;  // (every prev was read in front of the scan's barriers)
  }
  if (t == 0) a.ccnt[blockIdx.x] = run;
}

__global__ __launch_bounds__(kCfBlock) void cf_plan_kernel(CfDev a) {
  __shared__ uint32_t scut[kCoMaxFiles + 1];
  __shared__ uint64_t sh[kCfWaves];
  uint64_t n;
  uint32_t nf;
  const bool ok = cf_stage(a, scut, &n, &nf);
  const uint32_t t = threadIdx.x;
  if (!ok) {
    if (t == 0) {
      a.tot[kTotN] = a.tot[kTotNf] = a.tot[kTotSlices] = 0;
      a.built[0] = a.built[1] = 0;
      a.built[2] = kCfInputFlagged;
    }
    return;
  }
  const uint32_t nch = static_cast<uint32_t>((n + kCfChunk - 1) / kCfChunk);
  uint64_t total = 0;
  for (uint32_t c0 = 0; c0 < nch; c0 += kCfBlock) {
    const uint32_t c = c0 + t;
    uint64_t all;
    const uint64_t x = total + block_scan<uint64_t, kCfWaves>(c < nch ? a.ccnt[c] : 0, sh, &all);
    if (c < nch) a.cscan[c] = static_cast<uint32_t>(x);
    total += all;
  }
  __syncthreads();  // cscan is read back below
  uint64_t brun = 0, srun = 0;
  int many = 0;
  for (uint32_t f0 = 0; f0 < nf; f0 += kCfBlock) {
    const uint32_t f = f0 + t;
    const bool in = f < nf;
    uint64_t D = 0;
    if (in) {
      const uint32_t b = scut[f], e = scut[f + 1];
      const uint64_t gb = static_cast<uint64_t>(a.cscan[b / kCfChunk]) + a.gpre[f];
      const uint64_t ge = f + 1 < nf ? static_cast<uint64_t>(a.cscan[e / kCfChunk]) + a.gpre[f + 1] : total;
      D = ge - gb;
    }
    const uint32_t L = in ? full_num_lines(D, a.bpk, nullptr) : 0;
    const uint64_t bytes = cf_block_bytes(L);
    const uint32_t ns = cf_slices(L, a.lgR);
    const bool over = in && ns > kCfMaxSlices;
    uint64_t ball, sall;
    const uint64_t base = brun + block_scan<uint64_t, kCfWaves>(in ? co_pad16(bytes) : 0, sh, &ball);
    const bool fits = in && !over && base + bytes <= a.filters_cap;
    const uint64_t sl = srun + block_scan<uint64_t, kCfWaves>(fits ? ns : 0, sh, &sall);
    if (in) {
      a.cut[f] = scut[f];
      a.fL[f] = L;
      a.fmagic[f] = fastmod_magic(L ? L : 1);
      a.fsl0[f] = static_cast<uint32_t>(sl);
      a.fbase[f] = base;
      a.recs[f] = CfRec{base, bytes, D, L};
    }
    many |= over;
    brun += ball;
    srun += sall;
  }
  many = __syncthreads_or(many);
  if (t) return;
  a.cut[nf] = static_cast<uint32_t>(n);
  a.fsl0[nf] = static_cast<uint32_t>(srun);
  a.tot[kTotN] = n;
  a.tot[kTotNf] = nf;
  a.tot[kTotSlices] = srun;
  a.built[0] = nf;
  a.built[1] = brun;
  a.built[2] = (brun > a.filters_cap ? kCfCap : 0) | (many ? kCfTooManyLines : 0);
}

__global__ __launch_bounds__(kCfBlock) void cf_partition_kernel(CfDev a) {
  __shared__ uint32_t scut[kCoMaxFiles + 1];
  __shared__ uint32_t hist[kCfMaxBins + 1];  // a bin's pairs, then its first unit
  __shared__ uint32_t sh[kCfWaves];
  const uint64_t n = a.tot[kTotN];
  const uint32_t nf = static_cast<uint32_t>(a.tot[kTotNf]);
  const uint64_t i00 = static_cast<uint64_t>(blockIdx.x) * kCfChunk;
  if (i00 >= n) return;
  const uint32_t t = threadIdx.x;
  for (uint32_t f = t; f <= nf; f += kCfBlock) scut[f] = a.cut[f];
  for (uint32_t j = t; j <= kCfMaxBins; j += kCfBlock) hist[j] = 0;
  __syncthreads();
  const uint64_t i_end = i00 + kCfChunk < n ? i00 + kCfChunk : n;
  const uint32_t f_lo = co_file_of(scut, nf, i00), f_hi = co_file_of(scut, nf, i_end - 1);
  const uint32_t lo_id = a.fsl0[f_lo], nb = a.fsl0[f_hi + 1] - lo_id;
  uint16_t* tab = a.tab + static_cast<uint64_t>(blockIdx.x) * (kCfMaxBins + 1);
  uint32_t* reg = a.region + static_cast<uint64_t>(blockIdx.x) * kCfRegion;
  if (nb > kCfMaxBins) {  // (never: cf_bins_bound.  The slice pass then finds no entry of this chunk)
    for (uint32_t j = t; j <= kCfMaxBins; j += kCfBlock) tab[j] = 0;
    if (t == 0) a.clo[blockIdx.x] = lo_id;
    return;
  }
  const uint32_t rmask = (1u << a.lgR) - 1;
  uint32_t bin[kCfSub], rank[kCfSub], ent[kCfSub];
#pragma unroll
  for (int s = 0; s < kCfSub; s++) {
    const uint64_t i = i00 + static_cast<uint64_t>(s) * kCfBlock + t;
    bin[s] = ~0u;
    rank[s] = ent[s] = 0;
    if (i >= i_end) continue;
    const uint32_t f = co_file_of(scut, nf, i), s0 = a.fsl0[f];
    if (a.fsl0[f + 1] == s0) continue;  // the file is not built
    const uint32_t h = a.hash[i], line = fastmod(h, a.fL[f], a.fmagic[f]);
    bin[s] = s0 - lo_id + (line >> a.lgR);
    rank[s] = atomicAdd(&hist[bin[s]], 1u);
    ent[s] = cf_entry(h, line & rmask);
  }
  __syncthreads();
  uint32_t cnt[kCfBinsPer], units = 0;
  const uint32_t j0 = t * kCfBinsPer;
#pragma unroll
  for (int q = 0; q < kCfBinsPer; q++) {
    cnt[q] = j0 + q < nb ? hist[j0 + q] : 0;
    units += (cnt[q] + 3) >> 2;
  }
  uint32_t all;
  uint32_t u = block_scan<uint32_t, kCfWaves>(units, sh, &all);  // (its barriers stand between the counts' reads and the writes below)
#pragma unroll
  for (int q = 0; q < kCfBinsPer; q++) {
    if (j0 + q >= nb) break;
    hist[j0 + q] = u;
    tab[j0 + q] = static_cast<uint16_t>(u);
    for (uint32_t x = cnt[q]; x & 3u; x++) reg[4 * u + x] = kCfPad;
    u += (cnt[q] + 3) >> 2;
  }
  if (t == 0) {
    tab[nb] = static_cast<uint16_t>(all);
    a.clo[blockIdx.x] = lo_id;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kCfSub; s++)
    if (bin[s] != ~0u) reg[4 * hist[bin[s]] + rank[s]] = ent[s];
}

// AddHash of one entry into the slice: K probes straight-line, or k in a loop (K = 0).
template <int K>
__device__ __forceinline__ void cf_add(uint32_t* sl, uint32_t e, int k) {
  if (e == kCfPad) return;
  uint32_t* line = sl + (e >> 18) * 16u;
  uint32_t bp = e & 511u;
  const uint32_t d = (e >> 9) & 511u;
  if constexpr (K > 0) {
#pragma unroll
    for (int i = 0; i < K; i++) {
      atomicOr(&line[bp >> 5], 1u << (bp & 31u));
      bp = (bp + d) & 511u;
    }
  } else {
    for (int i = 0; i < k; i++) {
      atomicOr(&line[bp >> 5], 1u << (bp & 31u));
      bp = (bp + d) & 511u;
    }
  }
}

template <int K>
__global__ __launch_bounds__(kCfSliceBlock) void cf_slice_kernel(CfDev a, crc32c::XPow xp) {
  __shared__ __attribute__((aligned(16))) uint32_t sl[(64u << kCfMaxLgR) / 4];
  __shared__ uint32_t T[1024];
  __shared__ uint32_t wv[kCfSliceWaves];
  const uint32_t s = blockIdx.x, t = threadIdx.x;
  if (s >= a.tot[kTotSlices]) return;
  const uint32_t nf = static_cast<uint32_t>(a.tot[kTotNf]);
  const uint32_t f = co_file_of(a.fsl0, nf, s);  // the last file with fsl0[f] <= s: s < fsl0[f + 1]
  const uint32_t js = s - a.fsl0[f], L = a.fL[f], R = 1u << a.lgR;
  const uint32_t lines = L - js * R < R ? L - js * R : R;
  uint4* sl4 = reinterpret_cast<uint4*>(sl);
  for (uint32_t q = t; q < lines * 4; q += kCfSliceBlock) sl4[q] = make_uint4(0, 0, 0, 0);
  crc32c::build_tables<kCfSliceBlock>(T);
  const uint32_t b = a.cut[f], e = a.cut[f + 1];
  const uint32_t lane = t & 63, wave = t >> 6;
  for (uint32_t c = b / kCfChunk + wave; c <= (e - 1) / kCfChunk; c += kCfSliceWaves) {
    const uint32_t j = s - a.clo[c];  // the slice's bin in chunk c
    if (j >= kCfMaxBins) continue;
    const uint16_t* tab = a.tab + static_cast<uint64_t>(c) * (kCfMaxBins + 1);
    const uint4* reg = reinterpret_cast<const uint4*>(a.region + static_cast<uint64_t>(c) * kCfRegion);
    const uint32_t u1 = tab[j + 1];
    for (uint32_t u = tab[j] + lane; u < u1; u += 64) {
      const uint4 e4 = reg[u];
      cf_add<K>(sl, e4.x, a.k);
      cf_add<K>(sl, e4.y, a.k);
      cf_add<K>(sl, e4.z, a.k);
      cf_add<K>(sl, e4.w, a.k);
    }
  }
  __syncthreads();
  uint8_t* out = a.filters + a.fbase[f] + static_cast<uint64_t>(js) * R * 64;
  for (uint32_t q = t; q < lines * 4; q += kCfSliceBlock) {
    const uint4 v = sl4[q];
    __builtin_nontemporal_store(u32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4*>(out + 16 * q));
  }
  // The raw crc of the slice's bytes: R * 4 pieces of 16 bytes, zero pieces in
  // front of a short slice, a run of them per thread.
  const int per = 1 << (a.lgR - 6);
  const int lead = static_cast<int>(R * 4 - lines * 4);
  uint32_t acc = 0;
  for (int i = 0; i < per; i++) {
    const int q = static_cast<int>(t) * per + i - lead;
    if (q < 0) continue;
    const uint4 v = sl4[q];
    acc = crc32c::raw_word(acc, v.x, T);
    acc = crc32c::raw_word(acc, v.y, T);
    acc = crc32c::raw_word(acc, v.z, T);
    acc = crc32c::raw_word(acc, v.w, T);
  }
  acc = crc32c::wave_fold(acc, xp, a.lgR + 1);  // level k joins neighbours of 16 * per * 2^k bytes
  if (lane == 0) wv[wave] = acc;
  __syncthreads();
  if (t == 0) {
    uint32_t r = 0;
    for (int w = 0; w < kCfSliceWaves; w++) r = crc32c::mulmod(r, xp.p[a.lgR + 7]) ^ wv[w];  // a wave is 2^(lgR + 7) bits
    a.partial[s] = r;
  }
}
static_assert(kCfSliceBlock == 256, "the slice's crc split: R * 4 pieces over 256 threads, T a value per thread");

// A thread per file: fold the slices, append the filter's trailer and the type
// byte, write the two trailers.
__global__ __launch_bounds__(kCfSliceBlock) void cf_finish_kernel(CfDev a, crc32c::XPow xp) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.tot[kTotNf]) return;
  const uint32_t s0 = a.fsl0[f], ns = a.fsl0[f + 1] - s0;
  if (ns == 0) return;  // the block is not built
  const uint32_t L = a.fL[f], R = 1u << a.lgR;
  uint32_t raw = 0;
  for (uint32_t js = 0; js + 1 < ns; js++) raw = crc32c::mulmod(raw, xp.p[a.lgR + 9]) ^ a.partial[s0 + js];  // 64 R bytes
  raw = crc32c::mulmod(raw, crc32c::xpow(xp, static_cast<uint64_t>(L - (ns - 1) * R) * kLineBits)) ^ a.partial[s0 + ns - 1];
  uint8_t tr[10] = {static_cast<uint8_t>(static_cast<int8_t>(a.k)), static_cast<uint8_t>(L), static_cast<uint8_t>(L >> 8),
                    static_cast<uint8_t>(L >> 16), static_cast<uint8_t>(L >> 24), 0 /* kNoCompression */};
  for (int j = 0; j < 6; j++) raw = crc32c::raw_byte(raw, tr[j]);
  crc32c::store_trailer(tr + 5, 0, crc32c::value(raw, 64ull * L + 6, xp));
  uint8_t* out = a.filters + a.fbase[f] + 64ull * L;
  for (int j = 0; j < 10; j++) out[j] = tr[j];
}

}  // namespace

hipError_t launch_compaction_filters(const CfDev& a, hipEvent_t* ev, hipStream_t s) {
  if (a.chunks == 0 || a.slice_wgs == 0 || a.lgR < kCfMinLgR || a.lgR > kCfMaxLgR || a.bpk < 1 || a.bpk > kCfMaxBpk ||
      a.file_cap > kCoMaxFiles)
    return hipErrorInvalidValue;
  static const crc32c::XPow xp = crc32c::make_xpow();
  // whole words at a word stride: the hash reads its key without a shift
  const bool fixed = !a.koff;
  hipError_t e;
  auto mark = [&](int j) { return ev ? hipEventRecord(ev[j], s) : hipSuccess; };
  if ((e = mark(0)) != hipSuccess) return e;
  if (fixed) cf_hash_kernel<true><<<a.chunks, kCfBlock, 0, s>>>(a);
  else cf_hash_kernel<false><<<a.chunks, kCfBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(1)) != hipSuccess) return e;
  cf_plan_kernel<<<1, kCfBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(2)) != hipSuccess) return e;
  cf_partition_kernel<<<a.chunks, kCfBlock, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(3)) != hipSuccess) return e;
  if (a.k == 6) cf_slice_kernel<6><<<a.slice_wgs, kCfSliceBlock, 0, s>>>(a, xp);
  else cf_slice_kernel<0><<<a.slice_wgs, kCfSliceBlock, 0, s>>>(a, xp);
  if ((e = hipGetLastError()) != hipSuccess || (e = mark(4)) != hipSuccess) return e;
  cf_finish_kernel<<<kCoMaxFiles / kCfSliceBlock, kCfSliceBlock, 0, s>>>(a, xp);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return mark(5);
}

}  // namespace dlsm
