// dlsm_amd/csrc/compaction_filters.h -- the filter blocks of a compaction's
// output files.  Every output file's TableBuilder feeds ExtractUserKey(key) of
// each Add to a FullFilterBlockBuilder (table/table_builder_computeside.cc:222-224)
// and writes [filter][type 0][masked crc32c] at Finish (:389-432), so file f of a
// cut run has a block of its own: the AddKey dedup (full_filter_block.cc:45-48)
// restarts at the file's first pair and the line count comes from the file's own
// consecutive-distinct count.  This header holds the geometry the kernels
// (compaction_filters.hip), the host planning (host_plan.h) and the host form
// (bloom_capi.hip) share.  Plain integer code: no device call, nothing compiled
// from the reference.
#pragma once
#include <stdint.h>

#include "bloom_math.h"
#include "compaction_output.h"

namespace dlsm {

constexpr uint32_t kCfChunk = 4096;     // pairs of one hash / partition workgroup
constexpr uint32_t kCfMaxSlices = 512;  // slices of one file: a file of more lines is flagged, not built
constexpr int kCfMinLgR = 7;            // a slice is 2^lgR lines: 8 KiB ...
constexpr int kCfMaxLgR = 9;            // ... to 32 KiB of LDS
constexpr int kCfMaxBpk = 512;          // bits per key a call takes (the bins bound below)
// Bins of one chunk.  A chunk's pairs lie in files that are contiguous, and
// flat slice ids run in file order, so the chunk's bins are one id range: the
// files that lie wholly inside the chunk and at most two edge files.  A whole
// file of n pairs has L <= n * bpk / 512 + 2 lines, so at most
// 1 + (n * bpk / 512 + 1) / R slices; W <= 4096 such files hold 4096 pairs or
// fewer together, which bounds their slices by W + (8 * bpk + W) / R.  An edge
// file adds at most kCfMaxSlices.
constexpr uint32_t cf_bins_bound(int bpk, int lgR) {
  return kCfChunk + ((8u * static_cast<uint32_t>(bpk) + kCfChunk) >> lgR) + 1 + 2 * kCfMaxSlices;
}
constexpr uint32_t kCfMaxBins = cf_bins_bound(kCfMaxBpk, kCfMinLgR);  // the LDS histogram of the partition
// Entries of one chunk's region: every bin is padded to whole 16-byte units of
// four entries, and only a bin that holds a pair has a pad.
constexpr uint32_t kCfRegion = 4 * kCfChunk;
constexpr uint32_t kCfPad = 0xffffffffu;  // a pad entry

enum : uint64_t {  // DLSM_FILTERS_* of the public header
  kCfCap = 1,
  kCfTooManyLines = 2,
  kCfInputFlagged = 256,
};
constexpr uint64_t kCfBuiltOk = kTbDataCap | kTbIndexCap | kTbChunkCap;  // bits of dlsm_output_built a call accepts

struct CfRec {  // dlsm_output_filter
  uint64_t base, bytes, n_distinct, num_lines;
};

DLSM_HD uint64_t cf_block_bytes(uint32_t L) { return 64ull * L + 10; }
DLSM_HD uint32_t cf_slices(uint32_t L, int lgR) { return (L + (1u << lgR) - 1) >> lgR; }

// What AddHash reads of a hash (bloom_impl.h:427-443): the first bit position
// h & 511 and the step's low nine bits, delta & 511 -- bit i is
// (h + i * delta) & 511 -- beside the line inside the slice.
DLSM_HD uint32_t cf_entry(uint32_t h, uint32_t line_in_slice) {
  return (h & 511u) | ((bloom_delta(h) & 511u) << 9) | (line_in_slice << 18);
}

}  // namespace dlsm
