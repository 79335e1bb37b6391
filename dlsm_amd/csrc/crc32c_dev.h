// dlsm_amd/csrc/crc32c_dev.h -- crc32c (Castagnoli, util/crc32c.h:17-37) as the
// kernel families compute it: the algebra (host and device, so a CPU test can
// call it), the host's tables, and for the kernels the pieces of a parallel crc.
// block_crc.hip (streams in 64 KiB parts), block_ingest.hip and
// compaction_output.hip (blocks in 32 KiB parts), compaction_filters.hip (filter
// slices in LDS) and the host functions of bloom_capi.hip use it; each keeps its
// own kernels, grids and part layouts.
//
// Parallel form.  With r(D) the "raw" crc (the register starts at 0, no final
// inversion), r is GF(2)-linear and ignores leading zero bytes:
//   r(A||B) = r(A) * x^(8|B|)  xor  r(B)   (mod P),   r(0^k || D) = r(D),
// and the standard value is Value(D) = ~(0xffffffff * x^(8|D|) xor r(D)).
// So a stream is front-padded with zeros to whole parts, every thread takes the
// raw crc of its own bytes, and threads, waves, workgroups and parts fold pairs
// of neighbours with one constant x^(bits of the right neighbour) per level.
// Polynomials are in the reflected representation: bit 31 is x^0.
//
// bloom_kernels.hip is the one place with a variant of its own, and stays so:
// its crc_mulmod is a select form, its crc_word reads 16-entry nibble tables
// chosen for the fused seal's LDS bank conflicts, and its trailer code avoids
// dependent loads.  Its host tables (full_block_crc_tables) come from here.
#pragma once
#include <stdint.h>

#include "bloom_math.h"

namespace dlsm {
namespace crc32c {

constexpr uint32_t kPoly = 0x82f63b78u;       // reflected Castagnoli polynomial
constexpr uint32_t kMaskDelta = 0xa282ead8u;  // util/crc32c.h:22

// a(x) * b(x) mod P.
DLSM_HD uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kPoly : (b >> 1);
  }
  return p;
}

struct XPow {
  uint32_t p[40];  // x^(2^k) mod P, k < 40
};

// x^bits mod P, bits < 2^40 (a byte count shifted by 3).
DLSM_HD uint32_t xpow(const XPow& xp, uint64_t bits) {
  uint32_t r = 0x80000000u;  // x^0
  for (int k = 0; bits; k++, bits >>= 1)
    if (bits & 1u) r = mulmod(r, xp.p[k]);
  return r;
}

// The raw crc of one byte appended to register r.
DLSM_HD uint32_t raw_byte(uint32_t r, uint32_t b) {
  r ^= b;
#pragma unroll
  for (int k = 0; k < 8; k++) r = (r & 1u) ? (r >> 1) ^ kPoly : (r >> 1);
  return r;
}

// ... and of one little-endian word (slice-by-4).  T[0..255]: the byte table;
// T[256 t + i]: the extension tables (fill_tables, build_tables).
DLSM_HD uint32_t raw_word(uint32_t r, uint32_t w, const uint32_t* T) {
  r ^= w;
  return T[768 + (r & 0xffu)] ^ T[512 + ((r >> 8) & 0xffu)] ^ T[256 + ((r >> 16) & 0xffu)] ^ T[r >> 24];
}

// crc32c::Value of a stream of `bytes` bytes from its raw crc.
DLSM_HD uint32_t value(uint32_t raw, uint64_t bytes, const XPow& xp) {
  return ~(mulmod(0xffffffffu, xpow(xp, bytes << 3)) ^ raw);
}

// crc32c::Mask (util/crc32c.h:29-32).
DLSM_HD uint32_t mask(uint32_t crc) { return ((crc >> 15) | (crc << 17)) + kMaskDelta; }

// Host only: the table of squares, a kernel argument of every crc launch.
inline XPow make_xpow() {
  XPow x;
  x.p[0] = 0x40000000u;  // x^1
  for (int k = 1; k < 40; k++) x.p[k] = mulmod(x.p[k - 1], x.p[k - 1]);
  return x;
}

// Host only: the 1024 words of the slice-by-4 tables.
inline void fill_tables(uint32_t* T) {
  for (uint32_t i = 0; i < 256; i++) T[i] = raw_byte(i, 0);
  for (int t = 1; t < 4; t++)
    for (uint32_t i = 0; i < 256; i++) T[256 * t + i] = (T[256 * (t - 1) + i] >> 8) ^ T[T[256 * (t - 1) + i] & 0xffu];
}

#ifdef __HIPCC__

// The slice-by-4 tables into LDS, by the whole workgroup of kThreads threads:
// an entry of each table per thread, the first 256 threads of a larger group.
template <int kThreads>
__device__ __forceinline__ void build_tables(uint32_t* T) {
  static_assert(kThreads >= 256, "a table entry per thread");
  const bool mine = kThreads == 256 || threadIdx.x < 256;
  if (mine) T[threadIdx.x] = raw_byte(threadIdx.x, 0);
  __syncthreads();
  for (int t = 1; t < 4; t++) {
    if (mine) {
      const uint32_t prev = T[256 * (t - 1) + threadIdx.x];
      T[256 * t + threadIdx.x] = (prev >> 8) ^ T[prev & 0xffu];
    }
    __syncthreads();
  }
}

// The wave's fold: every lane holds the raw crc of 2^first bits, lane order is
// stream order; level k joins neighbours of 2^(first + k) bits.  The wave's raw
// crc in lane 0.  first: 7 where a lane holds 16 bytes.  block_crc.hip's
// crc_parts_kernel keeps the loop written out: called from its loop over the
// part's passes, the shared function changes the kernel's SGPR spill count.
__device__ __forceinline__ uint32_t wave_fold(uint32_t r, const XPow& xp, int first) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const uint32_t other = __shfl_xor(r, 1 << k, 64);
    if ((lane & (1 << k)) == 0) r = mulmod(r, xp.p[first + k]) ^ other;
  }
  return r;
}

// The raw crc of a 256-thread workgroup's part of kPasses passes, thread t's
// 16-byte piece of pass i in v[i] (pass-major: a pass is 4 KiB = 2^15 bits):
// Horner over the thread's pieces, one tree fold, then the waves (1 KiB each)
// in order.  wv: a slot per wave.  The result in thread 0.  (xp by value: by
// reference the kernel loads the whole table ahead of its first use.)
// block_ingest.hip's parts kernel calls it.  compaction_output.hip's seal keeps
// the table build and these lines written out in co_seal_parts_kernel, and
// value / store_trailer written out in co_seal_finish_kernel: through the
// shared functions the kernels' registers and schedule come out differently,
// and the seal of a hundred files measured one percent slower than before,
// outside the spread of the old code's own repeats.
template <int kPasses>
__device__ __forceinline__ uint32_t part_fold(const uint4 (&v)[kPasses], const uint32_t* T, const XPow xp, uint32_t* wv) {
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < kPasses; i++) {
    uint32_t r = raw_word(0, v[i].x, T);
    r = raw_word(r, v[i].y, T);
    r = raw_word(r, v[i].z, T);
    r = raw_word(r, v[i].w, T);
    acc = mulmod(acc, xp.p[15]) ^ r;
  }
  acc = wave_fold(acc, xp, 7);
  if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = acc;
  __syncthreads();
  uint32_t s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < 4; w++) s = mulmod(s, xp.p[13]) ^ wv[w];
  return s;
}

// A block's trailer at t: [type][Fixed32(Mask(value))] (table/format.cc:398-408).
__device__ __forceinline__ void store_trailer(uint8_t* t, uint8_t type, uint32_t value) {
  const uint32_t m = mask(value);
  t[0] = type;
  t[1] = static_cast<uint8_t>(m);
  t[2] = static_cast<uint8_t>(m >> 8);
  t[3] = static_cast<uint8_t>(m >> 16);
  t[4] = static_cast<uint8_t>(m >> 24);
}

#endif  // __HIPCC__

}  // namespace crc32c
}  // namespace dlsm
