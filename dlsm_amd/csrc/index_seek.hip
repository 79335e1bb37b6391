// dlsm_amd/csrc/index_seek.hip -- Table::InternalGet's index step for a planned
// Get batch (dlsm_index_seek_dev) and the validation half of opening the index
// blocks it searches (dlsm_tableindex_create_blocks).  The format's rules are
// the DLSM_HD functions of index_seek.h; this file is the work split.
//
// Open (after block_ingest.hip has copied and crc-checked the blocks): a header
// launch, one thread per file (Block's ctor checks, the entry count), and an
// entry launch, one thread per entry SLOT.  A block of len content bytes holds
// at most (len - 4) / kIndexEntryMinBytes entries, so the host lays the slots of
// all files out from the lengths alone -- no count comes back before the
// launch -- and a thread finds its file by a search of the slots' prefix sums,
// as ingest_parts_kernel finds its block.  Entry i is reached through restart
// i, never by walking, checks itself against its neighbours (index_entry_valid)
// and, when i is a multiple of kIndexFenceS, writes its fence.  A failed check
// stores 1 to the file's flag (every writer stores the same value).
//
// Seek: one thread per task, a workgroup takes a contiguous share of the tasks
// (the total is read on the device), so its tasks share one file or a few and
// that file's fences and upper search levels are shared through L2.
// file_begin sits in LDS when it fits.  Per task: the key's prefix (two 8-byte
// loads), a branchless lower bound over the file's fences (one 16-byte load
// per step), then <= log2(S) window steps of two dependent loads (restart
// offset, entry), the entry's key compared 8 bytes at a time.  The lanes of a
// wave step through their searches together, so a wave has 64 independent
// loads in flight per step; nothing is held in per-lane arrays.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"

namespace dlsm {
namespace {

constexpr int kOpenBlock = 256;

__global__ __launch_bounds__(kOpenBlock) void index_header_kernel(IndexFileDev* __restrict__ files,
                                                                  const IngestRecord* __restrict__ rec,
                                                                  uint32_t n_files) {
  const uint32_t f = blockIdx.x * kOpenBlock + threadIdx.x;
  if (f >= n_files) return;
  IndexFileDev F = files[f];
  if (!F.data) return;
  if (rec[F.rec].status != DLSM_INGEST_OK) {  // the contents are not to be trusted: no entry thread reads them
    files[f].bad = 1;
    return;
  }
  IndexView v;
  const bool ok = index_header_valid(F.data, F.len, &v);
  files[f].restarts = v.restarts;
  files[f].n = ok ? v.n : 0;
  files[f].bad = ok ? 0 : 1;
}

__global__ __launch_bounds__(kOpenBlock) void index_entries_kernel(IndexFileDev* __restrict__ files,
                                                                   const uint64_t* __restrict__ slot0,
                                                                   uint32_t n_files, uint64_t slots,
                                                                   RoutePrefix* __restrict__ fence) {
  const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * kOpenBlock + threadIdx.x;
  if (gid >= slots) return;
  // the file f with slot0[f] <= gid < slot0[f + 1] (slot0 has n_files + 1 entries)
  uint32_t lo = 0, hi = n_files;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (slot0[mid] <= gid) lo = mid;
    else hi = mid;
  }
  const IndexFileDev F = files[lo];
  const uint64_t i64 = gid - slot0[lo];
  if (!F.data || i64 >= F.n) return;  // (a rejected header left n = 0)
  const uint32_t i = static_cast<uint32_t>(i64);
  const IndexView v{F.data, F.restarts, F.n};
  if (!index_entry_valid(v, i)) files[lo].bad = 1;
  if (i % kIndexFenceS == 0) fence[F.fence0 + i / kIndexFenceS] = index_entry_prefix(v, i);
}

template <bool LDS>
__global__ __launch_bounds__(kIndexSeekBlock) void index_seek_kernel(IndexSeekDev a) {
  __shared__ uint64_t sfb[LDS ? kIndexSeekLdsFiles + 1 : 1];
  const uint64_t* fb = a.file_begin;
  if (LDS) {
    for (uint32_t j = threadIdx.x; j <= a.n_files; j += kIndexSeekBlock) sfb[j] = a.file_begin[j];
    __syncthreads();
    fb = sfb;
  }
  const uint64_t total = fb[a.n_files];
  const uint64_t limit = total < a.cap ? total : a.cap;
  // the workgroup's contiguous share, a multiple of the block
  uint64_t per = (limit + gridDim.x - 1) / gridDim.x;
  per = (per + kIndexSeekBlock - 1) / kIndexSeekBlock * kIndexSeekBlock;
  const uint64_t t0 = per * blockIdx.x;
  const uint64_t t1 = t0 + per < limit ? t0 + per : limit;
  const KeyDesc& kd = a.keys;
  for (uint64_t t = t0 + threadIdx.x; t < t1; t += kIndexSeekBlock) {
    // the file f with file_begin[f] <= t < file_begin[f + 1]: the last f whose begin is <= t
    uint32_t f = 0;
    for (uint32_t len = a.n_files; len > 1;) {  // f in [f, f + len)
      const uint32_t half = len >> 1;
      const bool right = fb[f + half] <= t;
      f = right ? f + half : f;
      len = right ? len - half : half;
    }
    const uint32_t g = a.gets[t];
    uint8_t state = kGetNotFound;
    KvHandle h{0, 0, 0};
    const IndexFileDev F = a.files[f];
    if (g < kd.n && F.data && F.n) {
      uint64_t s, l;
      if (kd.offsets) {
        s = kd.offsets[g];
        l = kd.offsets[g + 1] - s;
      } else {
        s = static_cast<uint64_t>(g) * kd.key_len;
        l = kd.key_len;
      }
      l = l > kd.suffix ? l - kd.suffix : 0;  // ExtractUserKey
      const uint8_t* kp = kd.bytes + s;
      const uint32_t un = static_cast<uint32_t>(l);
      const RoutePrefix q = un >= 16 ? RoutePrefix{index_be64(kp), index_be64(kp + 8)} : route_prefix(kp, un);
      const IndexView v{F.data, F.restarts, F.n};
      uint32_t lo, hi;
      index_fence_window(a.fence + F.fence0, index_fence_count(F.n, kIndexFenceS), F.n, kIndexFenceS, q, &lo, &hi);
      const uint32_t pos = index_window_search(v, lo, hi, kp, un, a.trailer);
      state = index_decide(v, pos, kp, un, f, &h);
    }
    if (a.task_state) a.task_state[t] = state;
    if (a.task_handle) a.task_handle[t] = h;
    if (state != kGetNotFound && g < kd.n) {
      if (a.get_state) a.get_state[g] = state;
      if (a.get_handle) a.get_handle[g] = h;
    }
  }
}

}  // namespace

hipError_t launch_index_open(IndexFileDev* files, const IngestRecord* rec, const uint64_t* slot0, uint32_t n_files,
                             uint64_t slots, RoutePrefix* fence, hipStream_t s) {
  if (n_files == 0) return hipSuccess;
  const uint64_t wgs = (slots + kOpenBlock - 1) / kOpenBlock;
  if (wgs > 0x7fffffffull) return hipErrorInvalidValue;
  index_header_kernel<<<(n_files + kOpenBlock - 1) / kOpenBlock, kOpenBlock, 0, s>>>(files, rec, n_files);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || wgs == 0) return e;
  index_entries_kernel<<<static_cast<uint32_t>(wgs), kOpenBlock, 0, s>>>(files, slot0, n_files, slots, fence);
  return hipGetLastError();
}

hipError_t launch_index_seek(const IndexSeekDev& a, uint32_t nwg, hipStream_t s) {
  if (a.n_files == 0 || nwg == 0 || a.cap == 0) return hipSuccess;
  if (a.n_files <= kIndexSeekLdsFiles) index_seek_kernel<true><<<nwg, kIndexSeekBlock, 0, s>>>(a);
  else index_seek_kernel<false><<<nwg, kIndexSeekBlock, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace dlsm
