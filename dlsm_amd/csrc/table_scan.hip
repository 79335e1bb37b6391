// dlsm_amd/csrc/table_scan.hip -- the record pass of a compaction merge whose
// runs are files of opened tables (dlsm_compaction_merge_tables_dev): one
// launch in the place of compaction_merge.hip's record pass, so the call stays
// at 2 * ceil(log2 R) + 4 launches ordered by the stream alone.  The rules are
// the DLSM_HD functions of table_scan.h; this file is the work split.
//
// One thread per input, an input being one index entry of one listed file;
// kCmChunk inputs per chunk, a workgroup takes cpw consecutive chunks -- the
// grid of the decide and offset passes behind it.
//
// Staged in LDS, once per workgroup (13 KiB): the listed files' entry bases (at
// most 1,024 u64), their file numbers and runs, and the runs' bases.  A thread
// finds its listed file by a uniform-length search of the bases (tb_last_le,
// ten steps in LDS), which gives the entry's number in the file and, through
// the file's run, the input's index in the run.  The file's index record
// (IndexFileDev) and chunk range come from global memory: a chunk of inputs
// spans one file or two, so those loads are the same address across a wave.
//
// Coalesced: the restart offsets (thread i reads Fixed32 i of the file's restart
// array), the 16-byte descriptors and the two 16-byte halves of the records.
// The entries themselves lie back to back in the block in entry order and the
// pairs back to back in the region, so neighbouring threads read neighbouring
// lines of both; an entry and a pair's header and key are read by their own
// thread and by the next one (the predecessor's handle for the back-to-back
// rule, its key for the run's strict ascent), the second time out of the
// cache.  The predecessor of a file's first entry is the last entry of the
// listed file before it that has one.
//
// A thread owns input g's descriptor and record; a workgroup owns its word of
// mismatch and unsorted bits, which the next launch ORs with the others'.  No
// counter is shared, nothing looks back, and no byte outside the index contents
// and the chunks is read: every check comes before the dereference it guards
// (table_scan.h).  There is no use for matrix instructions here.
#include <hip/hip_runtime.h>

#include "bloom_internal.h"

namespace dlsm {
namespace {

constexpr int kTsBlock = 1024;
static_assert(kCmChunk == kTsBlock, "a thread per input of a chunk");
static_assert(kTsMaxFiles + 1 <= kTsBlock && kCmMaxRuns + 1 <= kTsBlock, "a thread stages one listed file and one run");

typedef uint32_t ts_u32x4 __attribute__((ext_vector_type(4)));

struct TsAt {
  const uint64_t* p;
  __device__ uint64_t at(uint64_t i) const { return p[i]; }
};

__device__ __forceinline__ TsFile ts_file(const TsDev& t, uint32_t file) {
  const IndexFileDev* f = t.files + file;
  const uint32_t c0 = t.tables.chunk_begin[file], c1 = t.tables.chunk_begin[file + 1];
  return TsFile{IndexView{f->data, f->restarts, f->n}, KvChunks{t.tables.end + c0, t.tables.base + c0, c1 - c0}};
}

__global__ __launch_bounds__(kTsBlock) void ts_record_kernel(CmDev a, TsDev t) {
  __shared__ uint64_t sbase[kTsMaxFiles + 1];
  __shared__ uint64_t srun0[kCmMaxRuns + 1];
  __shared__ uint32_t sfile[kTsMaxFiles + 1];
  __shared__ uint8_t srun[kTsMaxFiles + 1];
  if (threadIdx.x <= t.n_listed) {
    sbase[threadIdx.x] = t.ts->ebase[threadIdx.x];
    sfile[threadIdx.x] = t.ts->file[threadIdx.x];
    srun[threadIdx.x] = t.ts->run[threadIdx.x];
  }
  if (threadIdx.x <= a.n_runs) srun0[threadIdx.x] = a.tab->base[threadIdx.x];
  __syncthreads();
  const TsAt base{sbase};
  int mismatch = 0, unsorted = 0;
  const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.cpw;
  for (uint64_t c = c0; c < c0 + a.cpw; c++) {
    const uint64_t g = c * kCmChunk + threadIdx.x;
    if (g >= a.n) break;
    // ebase[0] = 0 <= g < ebase[n_listed]: the last file that starts at or before g holds it
    const uint32_t k = static_cast<uint32_t>(tb_last_le(base, t.n_listed, g));
    const uint32_t r = srun[k], i = static_cast<uint32_t>(g - sbase[k]);
    const uint64_t idx = g - srun0[r];
    const TsFile f = ts_file(t, sfile[k]);
    const bool has_prev = idx > 0;
    uint32_t pk = k, pi = i - 1;
    if (has_prev && i == 0) {  // input g - 1 is of the same run: its files are listed in a row
      pk = static_cast<uint32_t>(tb_last_le(base, t.n_listed, g - 1));
      pi = static_cast<uint32_t>(g - 1 - sbase[pk]);
    }
    const TsFile pf = pk == k ? f : ts_file(t, sfile[pk]);
    CmDesc d;
    CmRec rec;
    const uint64_t bits = ts_entry(f, i, has_prev, pf, pi, r, idx, &d, &rec);
    mismatch |= (bits & kCmTableMismatch) != 0;
    unsorted |= (bits & kCmUnsorted) != 0;
    if (bits & kCmTableMismatch) continue;
    *reinterpret_cast<ts_u32x4*>(t.desc + g) = ts_u32x4{static_cast<uint32_t>(d.addr), static_cast<uint32_t>(d.addr >> 32),
                                                        d.key_size, d.value_size};
    ts_u32x4* o = reinterpret_cast<ts_u32x4*>(a.rec[0] + g);
    o[0] = ts_u32x4{static_cast<uint32_t>(rec.hi), static_cast<uint32_t>(rec.hi >> 32), static_cast<uint32_t>(rec.lo),
                    static_cast<uint32_t>(rec.lo >> 32)};
    o[1] = ts_u32x4{static_cast<uint32_t>(rec.inv), static_cast<uint32_t>(rec.inv >> 32), static_cast<uint32_t>(rec.ref),
                    static_cast<uint32_t>(rec.ref >> 32)};
  }
  mismatch = __syncthreads_or(mismatch);
  unsorted = __syncthreads_or(unsorted);
  if (threadIdx.x == 0) a.wg_flags[blockIdx.x] = (mismatch ? kCmTableMismatch : 0) | (unsorted ? kCmUnsorted : 0);
}

}  // namespace

hipError_t launch_table_record(const CmDev& a, const TsDev& t, hipStream_t s) {
  if (t.n_listed > kTsMaxFiles || (a.n > 0 && t.n_listed == 0)) return hipErrorInvalidValue;
  ts_record_kernel<<<a.nwg, kTsBlock, 0, s>>>(a, t);
  return hipGetLastError();
}

}  // namespace dlsm
