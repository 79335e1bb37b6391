// dlsm_amd/csrc/compaction_output.h -- the output side of a compaction: a merged
// run cut into size-capped tables.  DBImpl::DoCompactionWork closes its output
// file once builder->FileSize() >= MaxOutputFileSize() (db/db_impl.cc:3562-3573;
// FileSize() is the builder's offset after Add, table_builder_bacs.cpp:226,666)
// and opens the next one, so every file is a table of its own: offsets, chunk
// chain and index block restart at the file's first pair.  This header holds the
// cut rule, the placement of the files in the shared output buffers and the
// views through which table_build.h's units write one file out of a run.  Shared
// by the kernels (compaction_output.hip), the host form (bloom_capi.hip) and the
// CPU test (tests/cpp/compaction_output_test.cc).  Plain integer code: no device
// call, nothing compiled from the reference.
#pragma once
#include <stdint.h>

#include "table_build.h"

namespace dlsm {

constexpr uint32_t kCoMaxFiles = 4096;  // files of one call: the cut table (u32[kCoMaxFiles + 1]) sits in LDS
constexpr uint32_t kCoSealPieces = 2048;  // 16-byte pieces per workgroup part of the seal (32 KiB)

enum : uint64_t {  // DLSM_OUTPUT_* of the public header, beside the kTb* bits
  kCoFileCap = 128,
  kCoInputFlagged = 256,
};

struct CoFile {  // dlsm_output_file
  uint64_t first, n, data_base, data_bytes, index_base, index_bytes, chunk_base, n_chunks, flags;
};
static_assert(sizeof(CoFile) == 72, "file record layout");

DLSM_HD uint64_t co_pad16(uint64_t x) { return (x + 15) & ~uint64_t(15); }
// What is left of a capacity behind a base.
DLSM_HD uint64_t co_left(uint64_t cap, uint64_t base) { return cap > base ? cap - base : 0; }

// ---- the cut -------------------------------------------------------------------
// The byte count a file that starts at offset off_a has to reach: no pair
// reaches ~0, so an overflowing sum means "the rest".
DLSM_HD uint64_t co_cut_limit(uint64_t off_a, uint64_t max_file_bytes) {
  return off_a + max_file_bytes < off_a ? ~uint64_t(0) : off_a + max_file_bytes;
}
// The first pair of the file behind the one that starts with pair a (a < n):
// the smallest e > a with off[e] - off[a] >= max_file_bytes (the pair that
// reaches the threshold stays), n where there is none.  max_file_bytes = 0: n.
DLSM_HD uint64_t co_cut_next(const uint64_t* off, uint64_t n, uint64_t a, uint64_t max_file_bytes) {
  if (max_file_bytes == 0) return n;
  const uint64_t lim = co_cut_limit(off[a], max_file_bytes);
  const uint64_t e = a + 1 + kv_last_le(off + a, n - a + 1, lim - 1);  // off[a] < lim: the last offset below it
  return e < n ? e : n;
}

// The file of pair i: the last f in [0, nf) with cut[f] <= i (cut[0] = 0).
DLSM_HD uint32_t co_file_of(const uint32_t* cut, uint32_t nf, uint64_t i) {
  uint32_t f = 0;
  for (uint32_t len = nf; len > 1;) {
    const uint32_t half = len >> 1;
    const bool right = cut[f + half] <= i;
    f = right ? f + half : f;
    len = right ? len - half : half;
  }
  return f;
}

// File f's restart values in the shared array: its pairs' entry starts, its
// pair count and a pad (tb_index_unit reads n + 2 values), so two more slots
// per file than pairs.
DLSM_HD uint64_t co_es_base(uint64_t first, uint64_t f) { return first + 2 * f; }

// ---- a file's pairs as the table build's units address them ---------------------
// Pairs [first, first + n) of the run, offsets counted from the file's start.
struct CoFileView {
  TbSource src;
  uint64_t first, obase;  // obase = src.off[first]
  DLSM_HD uint64_t at(uint64_t i) const { return src.off[first + i] - obase; }
  DLSM_HD uint64_t key_size(uint64_t i) const { return src.key_size(first + i); }
  DLSM_HD uint64_t key_src(uint64_t i) const { return src.key_src(first + i); }
  DLSM_HD uint64_t value_src(uint64_t i) const { return src.value_src(first + i); }
};
// The same for keys and values of one length each: pair j of the file lies at
// j * (8 + klen + vlen), so the pair of a byte comes from a division and no
// offset is loaded or searched.  Addressed from pair j0 of the file.
struct CoFixedView {
  uint64_t ksrc, vsrc;  // the addresses of the file's first key and value
  uint32_t klen, vlen;
  uint64_t j0;
  DLSM_HD uint64_t pair() const { return 8 + static_cast<uint64_t>(klen) + vlen; }
  DLSM_HD uint64_t at(uint64_t i) const { return (j0 + i) * pair(); }
  DLSM_HD uint64_t key_size(uint64_t) const { return klen; }
  DLSM_HD uint64_t key_src(uint64_t i) const { return ksrc + (j0 + i) * klen; }
  DLSM_HD uint64_t value_src(uint64_t i) const { return vsrc + (j0 + i) * vlen; }
};
// The region's unit at u of a fixed-length file (tb_region_unit's contract; u
// and p1 count from the file's start).
DLSM_HD void co_region_unit_fixed(const TbSource& src, uint64_t first, uint64_t u, uint64_t p1, uint8_t* dst) {
  CoFixedView v{reinterpret_cast<uint64_t>(src.kbytes) + first * src.klen,
                reinterpret_cast<uint64_t>(src.vbytes) + first * src.vlen, src.klen, src.vlen, 0};
  v.j0 = u / v.pair();
  tb_region_unit(v, 1, u, p1, dst);  // one candidate: the unit's walk takes the pairs behind it from at()
}

// ---- the seal ------------------------------------------------------------------
// The crc'd stream of a block is its ctot content bytes and the type byte.  The
// whole 16-byte pieces of the contents are folded in parts of kCoSealPieces by a
// workgroup each; the bytes behind the last piece and the type byte are
// appended by the finish.  A block that is not sealed (it does not fit) has no part.
DLSM_HD uint32_t co_seal_parts(uint64_t ctot) {
  const uint64_t p = (ctot / 16 + kCoSealPieces - 1) / kCoSealPieces;
  return static_cast<uint32_t>(p ? p : 1);
}

}  // namespace dlsm
