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
// zeros leave the raw crc unchanged; see block_crc.hip for the algebra), and
// the parts of all blocks form one flat list: workgroup g finds its block by a
// binary search of the parts' prefix sums.  The block index never lives in a
// grid dimension, so the block count is bounded by memory only.
//
// A part is 8 passes of 256 threads x 16 bytes (32 KiB).  A thread issues its 8
// loads first (128 bytes in flight), stores them to the arena, and folds its 8
// piece crcs with one multiply per pass (Horner in x^(8 * 4096)); the
// workgroup then runs ONE tree fold over its 256 threads.  LDS: the 4 KiB
// slice-by-4 tables + 16 bytes.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"

namespace dlsm {
namespace {

constexpr uint32_t kPoly = 0x82f63b78u;  // reflected Castagnoli polynomial
constexpr int kThreads = 256;
constexpr int kPasses = 8;
constexpr uint32_t kPartPieces = kThreads * kPasses;  // 2,048 pieces = 32 KiB

// a(x) * b(x) mod P in the reflected representation (bit 31 = x^0).
__device__ __forceinline__ uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kPoly : (b >> 1);
  }
  return p;
}

struct XPow {
  uint32_t p[40];  // x^(2^k) mod P
};

__device__ __forceinline__ uint32_t x_pow_bytes(uint64_t n, const uint32_t* xpow) {
  uint32_t r = 0x80000000u;  // x^0
  n <<= 3;
  for (int k = 0; n; k++, n >>= 1)
    if (n & 1u) r = mulmod(r, xpow[k]);
  return r;
}

__device__ __forceinline__ uint32_t raw_word(uint32_t r, uint32_t w, const uint32_t* T) {
  r ^= w;
  return T[768 + (r & 0xffu)] ^ T[512 + ((r >> 8) & 0xffu)] ^ T[256 + ((r >> 16) & 0xffu)] ^ T[r >> 24];
}

__device__ __forceinline__ uint32_t raw_byte(uint32_t r, uint32_t b) {
  r ^= b;
#pragma unroll
  for (int k = 0; k < 8; k++) r = (r & 1u) ? (r >> 1) ^ kPoly : (r >> 1);
  return r;
}

__device__ void build_tables(uint32_t* T) {
  {
    uint32_t c = threadIdx.x;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ kPoly : (c >> 1);
    T[threadIdx.x] = c;
  }
  __syncthreads();
  for (int t = 1; t < 4; t++) {
    const uint32_t prev = T[256 * (t - 1) + threadIdx.x];
    T[256 * t + threadIdx.x] = (prev >> 8) ^ T[prev & 0xffu];
    __syncthreads();
  }
}
static_assert(kThreads == 256, "build_tables: one table entry per thread");

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
                                                                uint32_t n, int flags, XPow xp,
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
  if (crc) build_tables(T);

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
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < kPasses; i++) {
    uint32_t r = raw_word(0, v[i].x, T);
    r = raw_word(r, v[i].y, T);
    r = raw_word(r, v[i].z, T);
    r = raw_word(r, v[i].w, T);
    acc = mulmod(acc, xp.p[15]) ^ r;  // a pass is 4 KiB = 2^15 bits
  }
  // tree fold: level k joins neighbours of 16 * 2^k bytes
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const uint32_t other = __shfl_xor(acc, 1 << k, 64);
    if ((lane & (1 << k)) == 0) acc = mulmod(acc, xp.p[k + 7]) ^ other;
  }
  if (lane == 0) wv[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int q2 = 0; q2 < kThreads / 64; q2++) s = mulmod(s, xp.p[13]) ^ wv[q2];  // a wave is 1 KiB
    partial[g] = s;
  }
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
                                     uint32_t n, int flags, XPow xp, const uint32_t* __restrict__ partial,
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
    for (uint32_t p = 0; p < parts; p++) raw = mulmod(raw, xp.p[18]) ^ partial[part0[j] + p];  // 32 KiB
  }
  for (uint64_t d = tail0; d <= n_content; d++) {  // d == n_content: the type byte
    const uint8_t b = B.src[d];
    if (crc) raw = raw_byte(raw, b);
    if (store && d < n_content) B.dst[d] = b;
  }
  const uint8_t* t = B.src + n_content;
  if (crc) {
    const uint32_t value = ~(mulmod(0xffffffffu, x_pow_bytes(n_content + 1, xp.p)) ^ raw);
    const uint32_t masked = ((value >> 15) | (value << 17)) + 0xa282ead8u;  // crc32c::Mask
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

XPow make_xpow() {
  XPow x;
  auto mul = [](uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
      if (a & (0x80000000u >> i)) p ^= b;
      b = (b & 1u) ? (b >> 1) ^ kPoly : (b >> 1);
    }
    return p;
  };
  x.p[0] = 0x40000000u;  // x^1
  for (int k = 1; k < 40; k++) x.p[k] = mul(x.p[k - 1], x.p[k - 1]);
  return x;
}

}  // namespace

uint64_t ingest_block_parts(uint64_t len) { return len < 5 ? 1 : block_parts(len); }

hipError_t launch_block_ingest(const IngestBlock* blocks, const uint32_t* part0, uint32_t n, uint32_t total_parts,
                               bool verify, bool parse, uint32_t* partial, IngestRecord* rec, hipStream_t s) {
  if (n == 0) return hipSuccess;
  static const XPow xp = make_xpow();
  const int flags = (verify ? kVerify : 0) | (parse ? kParse : 0);
  ingest_parts_kernel<<<total_parts, kThreads, 0, s>>>(blocks, part0, n, flags, xp, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  ingest_finish_kernel<<<(n + 127) / 128, 128, 0, s>>>(blocks, part0, n, flags, xp, partial, rec);
  return hipGetLastError();
}

}  // namespace dlsm
