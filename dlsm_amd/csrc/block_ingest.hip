// dlsm_amd/csrc/block_ingest.hip -- ReadFilterBlock (table/format.cc:380-444)
// for n ragged sealed blocks in two launches: each block
//   [content (len - 5 bytes)][type][Fixed32(crc32c::Mask(crc32c(content || type)))]
// is copied to its place in a filter arena (or left where it is), its crc32c is
// recomputed and compared, its type byte is checked and, for filter blocks, the
// content's own 5-byte tail is parsed as FullFilterBlockReader's ctor does
// (table/full_filter_block.cc:186-252).  One record per block goes back to the
// host in one copy.
//
// Work split.  The crc'd stream of a block is its first len - 4 bytes (content
// and type byte).  It is cut into 16-byte pieces counted from the START, so a
// 16-byte-aligned source gives aligned 16-byte loads whatever the length; the
// < 16 bytes left over are appended by the finish kernel.  The pieces are
// front-padded with whole zero pieces to whole parts of kPartPieces (leading
// zeros leave the raw crc unchanged; see crc32c_dev.h for the algebra), and
// the parts of all blocks form one flat list: workgroup g finds its block by a
// binary search of the parts' prefix sums.  The block index never lives in a
// grid dimension, so the block count is bounded by memory only.
//
// A part is 8 passes of 256 threads x 16 bytes (32 KiB).  A thread issues its 8
// loads first (128 bytes in flight), stores them to the arena, and folds its 8
// piece crcs with one multiply per pass (Horner in x^(8 * 4096)); the
// workgroup then runs ONE tree fold over its 256 threads (crc32c::part_fold).
// LDS: the 4 KiB slice-by-4 tables + 16 bytes.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"
#include "crc32c_dev.h"

namespace dlsm {
namespace {

constexpr int kThreads = 256;
constexpr int kPasses = 8;
constexpr uint32_t kPartPieces = kThreads * kPasses;  // 2,048 pieces = 32 KiB

static_assert(kThreads == 256 && kPasses * kThreads * 16 == 32768, "crc32c::part_fold; the finish kernel folds 32 KiB parts");

// Pieces and parts of a block of `len` bytes (len >= 5).
__host__ __device__ inline uint64_t block_pieces(uint64_t len) { return (len - 4) / 16; }
__host__ __device__ inline uint64_t block_parts(uint64_t len) {
  const uint64_t p = (block_pieces(len) + kPartPieces - 1) / kPartPieces;
  return p ? p : 1;
}

// flags
constexpr int kVerify = 1;  // compare the stored crc
constexpr int kParse = 2;   // the contents are full filters: parse their tail

__global__ __launch_bounds__(kThreads) void ingest_parts_kernel(const IngestBlock* __restrict__ blocks,
                                                                const uint32_t* __restrict__ part0,
                                                                uint32_t n, int flags, crc32c::XPow xp,
                                                                uint32_t* __restrict__ partial) {
  __shared__ uint32_t T[1024];
  __shared__ uint32_t wv[kThreads / 64];
  // the block j with part0[j] <= g < part0[j + 1] (part0 has n + 1 entries)
  const uint32_t g = blockIdx.x;
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (part0[mid] <= g) lo = mid;
    else hi = mid;
  }
  const IngestBlock B = blocks[lo];
  const uint32_t part = g - part0[lo];
  const bool store = B.dst != nullptr && B.dst != B.src;
  const bool crc = (flags & kVerify) != 0;
  if (B.len < 5 || (!store && !crc)) {
    if (threadIdx.x == 0) partial[g] = 0;
    return;
  }
  const uint64_t n_content = B.len - 5;
  const int64_t pieces = static_cast<int64_t>(block_pieces(B.len));
  const int64_t lead = static_cast<int64_t>(block_parts(B.len) * kPartPieces) - pieces;  // zero pieces in front
  const bool src16 = (reinterpret_cast<uintptr_t>(B.src) & 15u) == 0;
  const bool dst16 = (reinterpret_cast<uintptr_t>(B.dst) & 15u) == 0;
  if (crc) crc32c::build_tables<kThreads>(T);

  // piece q of pass i: stream bytes [16 q, 16 q + 16), all below len - 4
  uint4 v[kPasses];
#pragma unroll
  for (int i = 0; i < kPasses; i++) {
    const int64_t q = static_cast<int64_t>(part) * kPartPieces + i * kThreads + threadIdx.x - lead;
    v[i] = make_uint4(0, 0, 0, 0);
    if (q < 0) continue;
    const uint8_t* p = B.src + 16 * q;
    if (src16) {
      v[i] = *reinterpret_cast<const uint4*>(p);
    } else {
      uint32_t w[4];
#pragma unroll
      for (int b4 = 0; b4 < 4; b4++)
        w[b4] = uint32_t(p[4 * b4]) | (uint32_t(p[4 * b4 + 1]) << 8) | (uint32_t(p[4 * b4 + 2]) << 16) |
                (uint32_t(p[4 * b4 + 3]) << 24);
      v[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  if (store) {
#pragma unroll
    for (int i = 0; i < kPasses; i++) {
      const int64_t q = static_cast<int64_t>(part) * kPartPieces + i * kThreads + threadIdx.x - lead;
      if (q < 0) continue;
      uint8_t* d = B.dst + 16 * q;
      const uint64_t end = static_cast<uint64_t>(16 * q) + 16;
      if (end <= n_content && dst16) {
        *reinterpret_cast<uint4*>(d) = v[i];
      } else {
        // the piece that ends in the type byte keeps that byte out of the arena
        const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
        const int m = end <= n_content ? 16 : 15;
        for (int b = 0; b < m; b++) d[b] = static_cast<uint8_t>(w[b >> 2] >> (8 * (b & 3)));
      }
    }
  }
  if (!crc) {
    if (threadIdx.x == 0) partial[g] = 0;
    return;
  }
  const uint32_t s = crc32c::part_fold(v, T, xp, wv);
  if (threadIdx.x == 0) partial[g] = s;
}

// parse_tail (bloom_capi.hip) on the device: FullFilterBlockReader's ctor.
__device__ bool parse_filter_tail(const uint8_t* tail, uint64_t len64, IngestRecord* r) {
  if (len64 < 5 || len64 > 0xffffffffull) return false;
  const int k = static_cast<int>(static_cast<int8_t>(tail[0]));
  if (k < 1) return false;
  const uint32_t len = static_cast<uint32_t>(len64) - 5;
  const uint32_t L = uint32_t(tail[1]) | (uint32_t(tail[2]) << 8) | (uint32_t(tail[3]) << 16) |
                     (uint32_t(tail[4]) << 24);
  int lg;
  if (L * kCacheLineBytes == len) {
    if (L == 0 || static_cast<uint64_t>(L) * kCacheLineBytes != len) return false;
    lg = 6;
  } else if (L == 0 || len % L != 0) {
    return false;
  } else {
    lg = 0;
  }
  r->k = k;
  r->L = L;
  r->lg = lg;
  r->magic = fastmod_magic(L);
  return true;
}

// One thread per block: fold the parts, append the < 16 stream bytes behind
// the last piece (copying the content bytes among them), and make the
// reference's checks in its order.
__global__ void ingest_finish_kernel(const IngestBlock* __restrict__ blocks, const uint32_t* __restrict__ part0,
                                     uint32_t n, int flags, crc32c::XPow xp, const uint32_t* __restrict__ partial,
                                     IngestRecord* __restrict__ rec) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const IngestBlock B = blocks[j];
  IngestRecord R;
  R.status = DLSM_INGEST_OK;
  R.k = 0;
  R.L = 0;
  R.lg = 0;
  R.magic = 0;
  if (B.len < 5) {
    R.status = DLSM_INGEST_SHORT;
    rec[j] = R;
    return;
  }
  const uint64_t n_content = B.len - 5;
  const bool store = B.dst != nullptr && B.dst != B.src;
  const bool crc = (flags & kVerify) != 0;
  const uint64_t tail0 = block_pieces(B.len) * 16;
  uint32_t raw = 0;
  if (crc) {
    const uint32_t parts = part0[j + 1] - part0[j];
    for (uint32_t p = 0; p < parts; p++) raw = crc32c::mulmod(raw, xp.p[18]) ^ partial[part0[j] + p];  // 32 KiB
  }
  for (uint64_t d = tail0; d <= n_content; d++) {  // d == n_content: the type byte
    const uint8_t b = B.src[d];
    if (crc) raw = crc32c::raw_byte(raw, b);
    if (store && d < n_content) B.dst[d] = b;
  }
  const uint8_t* t = B.src + n_content;
  if (crc) {
    const uint32_t masked = crc32c::mask(crc32c::value(raw, n_content + 1, xp));
    const uint32_t stored = uint32_t(t[1]) | (uint32_t(t[2]) << 8) | (uint32_t(t[3]) << 16) | (uint32_t(t[4]) << 24);
    if (masked != stored) R.status = DLSM_INGEST_CHECKSUM;
  }
  if (R.status == DLSM_INGEST_OK && t[0] != 0) R.status = DLSM_INGEST_TYPE;
  if (R.status == DLSM_INGEST_OK && (flags & kParse)) {
    uint8_t tail[5] = {0, 0, 0, 0, 0};
    if (n_content >= 5)
      for (int b = 0; b < 5; b++) tail[b] = B.src[n_content - 5 + b];
    if (!parse_filter_tail(tail, n_content, &R)) R.status = DLSM_INGEST_FILTER;
  }
  rec[j] = R;
}

}  // namespace

uint64_t ingest_block_parts(uint64_t len) { return len < 5 ? 1 : block_parts(len); }

hipError_t launch_block_ingest(const IngestBlock* blocks, const uint32_t* part0, uint32_t n, uint32_t total_parts,
                               bool verify, bool parse, uint32_t* partial, IngestRecord* rec, hipStream_t s) {
  if (n == 0) return hipSuccess;
  static const crc32c::XPow xp = crc32c::make_xpow();
  const int flags = (verify ? kVerify : 0) | (parse ? kParse : 0);
  ingest_parts_kernel<<<total_parts, kThreads, 0, s>>>(blocks, part0, n, flags, xp, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  ingest_finish_kernel<<<(n + 127) / 128, 128, 0, s>>>(blocks, part0, n, flags, xp, partial, rec);
  return hipGetLastError();
}

}  // namespace dlsm
