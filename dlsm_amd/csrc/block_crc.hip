// dlsm_amd/csrc/block_crc.hip -- crc32c (Castagnoli) on gfx950 for the
// filter-block trailer.
//
// FinishFilterBlock (table/table_builder_computeside.cc:418-428) appends
//   [type = kNoCompression (0)][Fixed32(crc32c::Mask(crc32c::Value(filter || type)))]
// to the filter before FlushFilter RDMA-writes it; ReadFilterBlock
// (table/format.cc:398-408) re-computes the same crc.  util/crc32c.h:17-37.
//
// Parallel form (the algebra and its pieces: crc32c_dev.h).  A stream is
// front-padded with zeros to whole 64 KiB parts; each thread takes 16 bytes (one
// coalesced 16-byte load), the wave and the workgroup fold pairs of equal-length
// neighbours with one constant x^(8*16*2^k) per level, and a second kernel folds
// the parts of each stream.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"
#include "crc32c_dev.h"

namespace dlsm {
namespace {

constexpr int kCrcBlock = 1024;                      // threads per workgroup
constexpr uint32_t kCrcSub = kCrcBlock * 16u;         // 16 KiB per workgroup pass
constexpr uint32_t kCrcSubs = 4;                      // passes per part
constexpr uint64_t kCrcPart = kCrcSub * kCrcSubs;     // 64 KiB per workgroup

// One stream: `len` data bytes followed by `extra` virtual zero bytes (the
// filter block's type byte).
struct CrcStream {
  const uint8_t* data;
  const uint64_t* len_dev;  // device length (filter builds), or nullptr
  uint64_t len_host;        // used when len_dev == nullptr
  uint32_t extra;           // virtual trailing zero bytes
  uint32_t pad;
};

__device__ __forceinline__ uint64_t stream_len(const CrcStream& S) {
  return S.len_dev ? *S.len_dev : S.len_host;
}

// Pass 1: raw CRC of each 64 KiB part (front-padded stream) -> partial[j][p].
__global__ __launch_bounds__(kCrcBlock) void crc_parts_kernel(const CrcStream* __restrict__ streams,
                                                              int max_parts, crc32c::XPow xp,
                                                              uint32_t* __restrict__ partial) {
  __shared__ uint32_t T[1024];
  __shared__ uint32_t wv[kCrcBlock / 64];
  const int j = blockIdx.y;
  const uint32_t p = blockIdx.x;
  const CrcStream S = streams[j];
  const uint64_t len = stream_len(S);
  if (len == 0 && S.len_dev) {  // failed build (capacity): nothing to seal
    if (threadIdx.x == 0) partial[static_cast<uint64_t>(j) * max_parts + p] = 0;
    return;
  }
  const uint64_t total = len + S.extra;
  const uint64_t parts = (total + kCrcPart - 1) / kCrcPart;
  if (p >= parts) return;
  const uint64_t padded = parts * kCrcPart;
  const int64_t lead = static_cast<int64_t>(padded - total);  // zero bytes in front
  crc32c::build_tables<kCrcBlock>(T);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t acc = 0;
  for (uint32_t sub = 0; sub < kCrcSubs; sub++) {
    // this thread's 16 bytes: stream positions q .. q+15
    const int64_t q = static_cast<int64_t>(p * kCrcPart + sub * kCrcSub + threadIdx.x * 16u) - lead;
    uint32_t wd[4];
    if (q >= 0 && q + 16 <= static_cast<int64_t>(len) &&
        (reinterpret_cast<uintptr_t>(S.data + q) & 15u) == 0) {
      const uint4 v = *reinterpret_cast<const uint4*>(S.data + q);
      wd[0] = v.x; wd[1] = v.y; wd[2] = v.z; wd[3] = v.w;
    } else {
#pragma unroll
      for (int b4 = 0; b4 < 4; b4++) {
        uint32_t x = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const int64_t d = q + 4 * b4 + b;
          const uint32_t byte = (d >= 0 && d < static_cast<int64_t>(len)) ? S.data[d] : 0u;
          x |= byte << (8 * b);
        }
        wd[b4] = x;
      }
    }
    uint32_t r = 0;
#pragma unroll
    for (int b4 = 0; b4 < 4; b4++) r = crc32c::raw_word(r, wd[b4], T);
    // crc32c::wave_fold, written out: as the shared function it changes this
    // kernel's SGPR spills (crc32c_dev.h)
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const uint32_t other = __shfl_xor(r, 1 << k, 64);
      if ((lane & (1 << k)) == 0) r = crc32c::mulmod(r, xp.p[k + 7]) ^ other;  // x^(8*16*2^k)
    }
    if (lane == 0) wv[w] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t s = 0;
      for (int q2 = 0; q2 < kCrcBlock / 64; q2++) s = crc32c::mulmod(s, xp.p[3 + 10]) ^ wv[q2];  // 1 KiB steps
      acc = crc32c::mulmod(acc, xp.p[3 + 14]) ^ s;  // 16 KiB steps
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[static_cast<uint64_t>(j) * max_parts + p] = acc;
}

// Pass 2: fold each stream's parts, finish the standard value, and either seal
// a filter block (type byte + masked crc, length += 5) or report the value.
__global__ void crc_finish_kernel(const CrcStream* __restrict__ streams, int n, int max_parts,
                                  crc32c::XPow xp, const uint32_t* __restrict__ partial,
                                  uint8_t* const* __restrict__ seal_out,
                                  const uint64_t* __restrict__ seal_cap,
                                  uint64_t* __restrict__ seal_len, uint32_t* __restrict__ crc_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const CrcStream S = streams[j];
  const uint64_t len = stream_len(S);
  if (seal_out && len == 0) return;  // failed build keeps out_len == 0
  const uint64_t total = len + S.extra;
  const uint64_t parts = (total + kCrcPart - 1) / kCrcPart;
  uint32_t raw = 0;
  for (uint64_t p = 0; p < parts; p++)
    raw = crc32c::mulmod(raw, xp.p[3 + 16]) ^ partial[static_cast<uint64_t>(j) * max_parts + p];  // 64 KiB
  const uint32_t value = crc32c::value(raw, total, xp);
  if (crc_out) crc_out[j] = value;
  if (seal_out) {
    if (len + 5 > seal_cap[j]) {
      seal_len[j] = 0;
      return;
    }
    crc32c::store_trailer(seal_out[j] + len, 0 /* kNoCompression */, value);
    seal_len[j] = len + 5;
  }
}

}  // namespace

uint64_t crc_max_parts(uint64_t max_len_plus_extra) {
  return (max_len_plus_extra + kCrcPart - 1) / kCrcPart;
}

hipError_t launch_crc_streams(const void* streams, int n, int max_parts, uint32_t* partial,
                              uint8_t* const* seal_out, const uint64_t* seal_cap, uint64_t* seal_len,
                              uint32_t* crc_out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  static const crc32c::XPow xp = crc32c::make_xpow();
  const CrcStream* st = static_cast<const CrcStream*>(streams);
  crc_parts_kernel<<<dim3(max_parts, n), kCrcBlock, 0, s>>>(st, max_parts, xp, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  crc_finish_kernel<<<(n + 63) / 64, 64, 0, s>>>(st, n, max_parts, xp, partial, seal_out, seal_cap,
                                                 seal_len, crc_out);
  return hipGetLastError();
}

size_t crc_stream_size() { return sizeof(CrcStream); }

// Host tables of the fused seal (bloom_internal.h kCrcTabWords): slice-by-4
// tables, then powers x^(8n) mod P for the build slice's thread segments,
// whole slices and whole lines.
void full_block_crc_tables(int lgR, uint32_t* out) {
  const crc32c::XPow xp = crc32c::make_xpow();
  crc32c::fill_tables(out);
  const uint64_t R = 1ull << lgR;
  const uint64_t seg = R * 64u / 512u;  // bytes per build-slice thread
  auto powers = [&](uint32_t* P, int count, uint64_t bytes) {  // P[m] = x^(8 m bytes)
    const uint32_t step = crc32c::xpow(xp, bytes << 3);
    P[0] = 0x80000000u;
    for (int m = 1; m < count; m++) P[m] = crc32c::mulmod(P[m - 1], step);
  };
  powers(out + 1024, 512, seg);
  powers(out + 1024 + 512, 256, R * 64u);
  powers(out + 1024 + 512 + 256, 2049, 64);
}

void crc_stream_fill(void* dst, const uint8_t* data, const uint64_t* len_dev, uint64_t len_host,
                     uint32_t extra) {
  CrcStream* c = static_cast<CrcStream*>(dst);
  c->data = data;
  c->len_dev = len_dev;
  c->len_host = len_host;
  c->extra = extra;
  c->pad = 0;
}

}  // namespace dlsm
