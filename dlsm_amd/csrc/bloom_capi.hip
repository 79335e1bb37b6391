// dlsm_amd/csrc/bloom_capi.hip -- the C ABI (include/dlsm_bloom.h): contexts,
// device workspace, job set-up, and the host-buffer (staged) call variants.
// Kernels live in bloom_kernels.hip.
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <unordered_map>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/dlsm_bloom.h"
#include "bloom_internal.h"
#include "host_plan.h"

using namespace dlsm;
using namespace dlsm::plan;

namespace {

int from_hip(hipError_t e) {
  if (e == hipSuccess) return DLSM_OK;
  if (e == hipErrorOutOfMemory) return DLSM_E_NOMEM;
  return DLSM_E_DEVICE;
}

#define DLSM_TRY(expr)                       \
  do {                                       \
    hipError_t _e = (expr);                  \
    if (_e != hipSuccess) return from_hip(_e); \
  } while (0)

#define DLSM_CHECK(expr)         \
  do {                           \
    int _s = (expr);             \
    if (_s != DLSM_OK) return _s; \
  } while (0)

// Growable device buffer (never shrinks; freed with the context).
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;     // elements
  uint64_t gen = 0;   // bumped by every (re)allocation: contents are gone
  int ensure(size_t n) {
    if (n <= cap && p) return DLSM_OK;
    gen++;
    if (p) {
      (void)hipFree(p);
      p = nullptr;
      cap = 0;
    }
    size_t want = std::max<size_t>(n, 1);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return from_hip(e);
    }
    cap = want;
    return DLSM_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

}  // namespace

// Pipelined passes (opt-in knobs).  Probe: round r+1's partition runs on a
// helper stream while the context stream runs round r's slice + unpermute,
// over kProbeBufs rotating intermediate buffers.  Build: job group g+1's
// partition overlaps group g's slices the same way.  The context stream's last
// command depends on every helper command, so a call needs no separate join.
// Off by default: measured on MI355X (profiles/r01_v12_*), the overlapped
// kernels each ran ~2x slower (the slice passes fill every wave slot of a CU)
// and every round added ~10 us of launch gaps, a net loss.
constexpr int kStageEvents = 4;

// The scheduling options a pooled context starts with; a recycled context gets
// them back (a thread may have changed them, e.g. a builder's BUILD_EXACT).
// Kept inside the context itself: a detached thread that exits after main
// returns still recycles its context safely (no static map to outlive).
struct CtxOpts {
  int path, build_groups;
  uint64_t probe_round;
  int probe_lgc, probe_lgr, build_exact;
  bool probe_serial;
  int probe_multi;
};

struct dlsm_ctx {
  int device = 0;
  CtxOpts opts0{};          // creation options (pooled thread contexts)
  bool opts0_set = false;
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  hipStream_t aux = nullptr;              // helper stream of the pipelined passes
  hipEvent_t ev_fork = nullptr;           // context stream -> helper
  hipEvent_t ev_part[kStageEvents] = {};  // partition of buffer / group b done (helper)
  hipEvent_t ev_free[kStageEvents] = {};  // buffer b consumed (context stream)
  // dlsm_ctx_set_partition_stream: the partition passes run on pstream
  // (typically restricted to a CU subset), the rest on the context stream
  hipStream_t pstream = nullptr;
  uint32_t pcus = 0;                      // CUs the persistent partition grid is sized for (0: all)
  hipEvent_t ev_pfork = nullptr;          // context stream -> pstream
  hipEvent_t ev_pdone = nullptr;          // partition done (pstream -> context stream)
  int path = 0;
  int build_groups = 1;     // job groups of a build (1 = one partition + one slice launch)
  uint64_t probe_round = 0;  // keys per probe round (0 = whole batch)
  int probe_lgc = 13;        // log2 keys per probe partition chunk (12..14; 13 = two 4,096-key units, 512 threads)
  int probe_lgr = 8;         // log2 stacked lines per probe slice (7: 64 KiB, 8: 128 KiB of LDS)
  int build_exact = 0;       // DLSM_OPT_BUILD_EXACT: 0 auto, 1 always count first, 2 never
  bool probe_serial = false;  // DLSM_OPT_PROBE_ROUND_SERIAL: rounds one after another on one stream
  int fault = 0;              // DLSM_OPT_FAULT_INJECT: > 0 -> builds / probes return -fault
  int probe_multi = 1;        // DLSM_OPT_PROBE_MULTI: 1 one pass over a multi-group set, 0 a pass per group
  uint64_t vslice_bytes = 0;  // DLSM_OPT_VERSION_SLICE_BYTES (0: default)
  uint32_t vpass_slices = kVMaxSlices;  // DLSM_OPT_VERSION_PASS_SLICES
  std::atomic<uint64_t> fallbacks{0};  // dlsm_fallback_note: host re-runs of this context's failed calls
  // build workspace
  DevBuf<uint32_t> entries;
  DevBuf<uint16_t> tab;  // chunk-major bucket offsets
  DevBuf<FullJobDev> jobs;
  DevBuf<uint32_t> starts;  // chunk0s | slice0s
  DevBuf<uint32_t> dchunk;  // per-chunk consecutive-distinct counts
  DevBuf<uint32_t> jobL;    // per-job line count (direct path)
  // last uploaded job table (skip the H2D when a caller repeats a batch); the
  // device buffers' allocation generations are part of the key, so a buffer
  // that ensure() reallocated (reserve, a bigger batch) -- even at the same
  // address -- is never taken as filled
  std::vector<FullJobDev> last_jobs;
  std::vector<uint32_t> last_starts;
  uint64_t last_jobs_gen = 0, last_starts_gen = 0;
  DevBuf<LegacyJobDev> ljobs;
  DevBuf<uint64_t> lstarts;
  // LDS-tiled legacy build (util/bloom.cc format)
  DevBuf<LegacyTileJobDev> ltjobs;
  DevBuf<uint32_t> ltstarts;  // chunk0s | slice0s
  DevBuf<uint16_t> lentries;  // u16 bit positions per tile bucket
  DevBuf<uint16_t> ltab;      // chunk-major tile-bucket offsets
  // probe workspace
  DevBuf<uint32_t> hashes;  // grouped probe / sliced version probe: one BloomHash per lookup
  DevBuf<uint32_t> vgl;     // sliced version probe: per sliced level, each lookup's global line
  DevBuf<uint8_t> vabyte;   // sliced version probe: per lookup, the sliced levels' answer bits
  DevBuf<uint32_t> vplan;   // sliced version probe: per-slice unit counters | slice-pass plan
  uint64_t vplan_zeroed = 0;  // vplan's allocation generation whose counters were zeroed
  DevBuf<uint16_t> pos;
  DevBuf<uint8_t> smask;
  DevBuf<uint8_t> plan_ws;  // read plan: tables and intermediate pairs (plan::ReadPlan's layout)
  DevBuf<uint8_t> route_ws;  // shard route: the Gets' bins and the tables (plan::ShardRoute's layout)
  DevBuf<uint8_t> kv_ws;     // value read: lengths, source addresses, partial sums (plan::KvReadPlan's layout)
  hipEvent_t ev_kv[4] = {};  // value read: around its three launches (dlsm_kv_read_stats)
  bool kv_timed = false;     // the last dlsm_kv_read_dev recorded all four
  int cus = 0;               // the device's compute units (0: not asked yet)
  // host-API staging
  DevBuf<uint8_t> st_keys;
  DevBuf<uint64_t> st_offs;
  DevBuf<uint8_t> st_out;
  DevBuf<uint64_t> st_len;
  DevBuf<uint8_t> st_filter;
  // crc32c / block sealing
  DevBuf<uint8_t> crc_streams;
  DevBuf<uint32_t> crc_partial;
  DevBuf<uint32_t> crc_tabs;  // fused seal: full_block_crc_tables(crc_tabs_lgr)
  int crc_tabs_lgr = -1;
  uint64_t crc_tabs_gen = 0;
  DevBuf<uint8_t*> crc_outp;
  DevBuf<uint64_t> crc_cap;
  DevBuf<uint32_t> crc_val;
  // sealed-block ingest (block_ingest.hip): descriptors, part prefix sums,
  // per-part crcs, per-block records; the events time its two launches
  DevBuf<IngestBlock> ing_blocks;
  DevBuf<uint32_t> ing_part0;
  DevBuf<uint32_t> ing_partial;
  DevBuf<IngestRecord> ing_rec;
  hipEvent_t ev_ing0 = nullptr, ev_ing1 = nullptr;
  uint64_t ing_read = 0, ing_written = 0;  // bytes of the last ingest
  // internal-key selection / gather: [blk_cnt | blk_bytes | tot(2) | first_bad]
  DevBuf<uint64_t> sel;
  // host-API results: page-locked, device-mapped, so the build kernels store
  // filters and lengths straight to host memory (one synchronisation, no D2H)
  uint8_t* h_out = nullptr;
  uint64_t h_out_cap = 0;
  uint64_t* h_len = nullptr;
  uint64_t h_len_cap = 0;
  // page-locked host staging lent to the context's (single) builder
  void* host_buf = nullptr;
  uint64_t host_cap = 0;
  std::atomic<const void*> host_owner{nullptr};
  // Page-locked sources of the small tables a call builds on the host and
  // uploads asynchronously (job tables, rebased offsets, lengths, crc stream
  // descriptors): a ring of slots, each reused only after the event recorded
  // behind its copy has completed -- a pageable (e.g. stack) source could be
  // gone before a queued copy reads it.
  // The slots are carved from one page-locked block allocated with the
  // context (hipHostMalloc takes a process-wide lock and milliseconds: lazily
  // allocated slots stalled concurrent builder threads' first calls by up to
  // 15 ms); a table larger than a slot gets a buffer of its own.
  static constexpr int kUpSlots = 16;
  static constexpr uint64_t kUpSlotBytes = 16384;
  uint8_t* up_block = nullptr;
  uint8_t* up_buf[kUpSlots] = {};
  uint64_t up_cap[kUpSlots] = {};
  bool up_own[kUpSlots] = {};  // up_buf[i] is a buffer of its own (not in up_block)
  hipEvent_t up_ev[kUpSlots] = {};
  bool up_live[kUpSlots] = {};
  int up_next = 0;
  // How a host-API call waits for its stream (ctx_sync): 0 hipStreamSynchronize,
  // 1 poll an event, yielding the core between polls, 2 a blocking-sync event
  // (DLSM_HOST_SYNC; default 1).  Many builder threads (dLSM runs 28) share
  // the host's cores with the HIP runtime's own threads: a waiter that spins
  // holds a core the other builders' AddKey hashing needs.
  int host_sync = 1;
  hipEvent_t ev_wait = nullptr;      // ctx_sync modes 1 and 2
};

struct dlsm_filterset {
  int device = 0;
  int F = 0;
  uint8_t* blob = nullptr;
  uint64_t blob_bytes = 0;
  FilterDev* d_filters = nullptr;
  FilterDev* d_slots = nullptr;  // 8 stacking slots per group
  std::vector<FilterDev> h;
  // sliced probe: one group (<= 8 filters, one L and k: the bench's set) or
  // several (filters of different sizes, > 8 filters); empty = direct only
  // (a filter in the reference's log2_cache_line_size_ == 0 branch)
  std::vector<ProbeGroup> groups;
  uint64_t stacked_bytes = 0;
  // One-pass probe (2..kMGMaxGroups groups, every group sliceable at 128 KiB
  // slices): the groups in slice order (by image width), their slices
  // numbered globally, and one slice launch per width class.
  MGroupDev* d_mg = nullptr;
  uint32_t* d_mgplan = nullptr;
  int mg_n = 0;
  uint32_t mg_slices = 0;
  uint32_t mg_region = 0;  // entries per chunk region (every group's sub-region)
  uint32_t mg_abytes = 0;  // answer bytes per chunk
  uint32_t mg_stage_bytes = 0;  // the partition's largest staging area (LDS)
  std::vector<MGClass> mg_classes;
};

namespace {

// Wait until everything queued on s so far has completed (see host_sync).
hipError_t ctx_sync(dlsm_ctx* ctx, hipStream_t s) {
  if (ctx->host_sync == 0 || !ctx->ev_wait) return hipStreamSynchronize(s);
  hipError_t e = hipEventRecord(ctx->ev_wait, s);
  if (e != hipSuccess) return e;
  if (ctx->host_sync == 2) return hipEventSynchronize(ctx->ev_wait);
  while ((e = hipEventQuery(ctx->ev_wait)) == hipErrorNotReady) sched_yield();
  return e;
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

int validate_keyset(const dlsm_keyset& k) {
  if (k.n == 0) return DLSM_OK;
  if (!k.bytes) return DLSM_E_ARG;
  if (k.suffix_len > 255) return DLSM_E_ARG;
  // fixed keys must hold the stripped suffix; zero-length user keys are legal
  if (!k.offsets && k.key_len < k.suffix_len) return DLSM_E_ARG;
  return DLSM_OK;
}

// The K20 kernels stage keys through LDS with 16-byte loads.
bool is_k20(const dlsm_keyset& k) {
  return k.offsets == nullptr && k.key_len == 20 && k.suffix_len == 0 &&
         (k.n == 0 || aligned(k.bytes, 16));
}

// 28-byte internal keys (20-byte user key + 8-byte trailer) straight from the
// memtable / compaction iterators take the LDS-tiled K28 partition loaders.
bool is_k28(const dlsm_keyset& k) {
  return k.offsets == nullptr && k.key_len == 28 && k.suffix_len == 8 &&
         (k.n == 0 || aligned(k.bytes, 16));
}

// The helper stream starts behind everything already queued on the context
// stream (the call's inputs).
int fork_aux(dlsm_ctx* ctx) {
  DLSM_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
  DLSM_TRY(hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
  return DLSM_OK;
}

// `to` waits for everything queued on `from` so far.
// dlsm_ctx_set_partition_stream: the partition stream starts behind
// everything queued on the context stream (the call's inputs, and the
// previous call's consumers of the workspace it overwrites) ...
int fork_part(dlsm_ctx* ctx) {
  DLSM_TRY(hipEventRecord(ctx->ev_pfork, ctx->stream));
  DLSM_TRY(hipStreamWaitEvent(ctx->pstream, ctx->ev_pfork, 0));
  return DLSM_OK;
}
// ... and the context stream's next pass starts behind the partition.
int join_part(dlsm_ctx* ctx) {
  DLSM_TRY(hipEventRecord(ctx->ev_pdone, ctx->pstream));
  DLSM_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_pdone, 0));
  return DLSM_OK;
}

int hand_over(hipStream_t from, hipStream_t to, hipEvent_t ev) {
  DLSM_TRY(hipEventRecord(ev, from));
  DLSM_TRY(hipStreamWaitEvent(to, ev, 0));
  return DLSM_OK;
}

// Asynchronous H2D copy of n bytes of a host-built table (any memory, e.g.
// a std::vector about to go out of scope) on stream s: the bytes are copied
// into one of the context's page-locked upload slots first, so the caller's
// buffer may be released as soon as this returns.  A slot is reused only
// after the event behind its previous copy has completed.
int ctx_upload(dlsm_ctx* ctx, void* dst, const void* src, size_t n, hipStream_t s) {
  if (n == 0) return DLSM_OK;
  const int i = ctx->up_next;
  ctx->up_next = (i + 1) % dlsm_ctx::kUpSlots;
  if (ctx->up_live[i]) {
    DLSM_TRY(hipEventSynchronize(ctx->up_ev[i]));
    ctx->up_live[i] = false;
  }
  if (ctx->up_cap[i] < n) {
    if (ctx->up_own[i]) (void)hipHostFree(ctx->up_buf[i]);
    ctx->up_buf[i] = nullptr;
    ctx->up_cap[i] = 0;
    ctx->up_own[i] = false;
    uint64_t c = 2 * dlsm_ctx::kUpSlotBytes;
    while (c < n) c <<= 1;
    DLSM_TRY(hipHostMalloc(reinterpret_cast<void**>(&ctx->up_buf[i]), c, hipHostMallocDefault));
    ctx->up_cap[i] = c;
    ctx->up_own[i] = true;
  }
  memcpy(ctx->up_buf[i], src, n);
  DLSM_TRY(hipMemcpyAsync(dst, ctx->up_buf[i], n, hipMemcpyHostToDevice, s));
  DLSM_TRY(hipEventRecord(ctx->up_ev[i], s));
  ctx->up_live[i] = true;
  return DLSM_OK;
}

}  // namespace

extern "C" {

const char* dlsm_strerror(int status) {
  switch (status) {
    case DLSM_OK: return "ok";
    case DLSM_E_ARG: return "invalid argument";
    case DLSM_E_CAPACITY: return "output slot too small";
    case DLSM_E_CORRUPT: return "corrupt bloom filter";
    case DLSM_E_DEVICE: return "HIP device error";
    case DLSM_E_NOMEM: return "device out of memory";
    case DLSM_E_BUSY: return "host staging buffer held by another user";
    default: return "unknown status";
  }
}

int dlsm_abi_version(void) { return DLSM_BLOOM_ABI_VERSION; }

uint32_t dlsm_bloom_hash(const void* key, size_t n) {
  return bloom_hash_host(static_cast<const uint8_t*>(key), n);
}

int dlsm_bloom_full_num_probes(int bits_per_key) { return full_num_probes(bits_per_key); }

int dlsm_bloom_full_size(uint64_t n_dedup, int bits_per_key, uint32_t* num_lines,
                         uint64_t* nbytes) {
  uint32_t tb;
  const uint32_t L = full_num_lines(n_dedup, bits_per_key, &tb);
  if (num_lines) *num_lines = L;
  if (nbytes) *nbytes = static_cast<uint64_t>(tb / 8u) + 5u;
  return DLSM_OK;
}

int dlsm_bloom_legacy_size(uint64_t n, int bits_per_key, uint64_t* nbytes) {
  if (nbytes) *nbytes = legacy_bits(n, bits_per_key) / 8 + 1;
  return DLSM_OK;
}

int dlsm_bloom_full_parse(const uint8_t* f, uint64_t len64, int* num_probes, uint32_t* num_lines,
                          int* log2_line) {
  if (!f || len64 < 5) return DLSM_E_CORRUPT;
  int k, lg;
  uint32_t L;
  DLSM_CHECK(parse_tail(f + len64 - 5, len64, &k, &L, &lg));
  if (num_probes) *num_probes = k;
  if (num_lines) *num_lines = L;
  if (log2_line) *log2_line = lg;
  return DLSM_OK;
}

int dlsm_device_count(int* n) {
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) c = 0;
  if (n) *n = c;
  return e == hipSuccess ? DLSM_OK : from_hip(e);
}

}  // extern "C"
namespace {
// Per-thread contexts (dlsm_thread_ctx): owned = handed out here, returned to
// a per-device free list at the thread's exit; bound = the caller's
// (dlsm_thread_ctx_bind), never touched here.  dLSM starts a std::thread per
// subcompaction (db/db_impl.cc:3373-3386): with the free list a new thread
// takes a context a finished one left -- its stream, page-locked blocks,
// events and grown device workspaces -- instead of paying their creation
// (hipHostMalloc takes a process-wide lock) and teardown per compaction.
// The list is never freed: contexts outlive every thread, so a builder that
// outlives its thread still holds a live context, and nothing is destroyed
// during static destruction, after the HIP runtime may be gone.
struct CtxPool {
  std::mutex m;
  std::map<int, std::vector<dlsm_ctx*>> free;  // device -> idle contexts
  uint64_t created = 0, reused = 0;
};
CtxPool& ctx_pool() {
  static CtxPool* p = new CtxPool();  // intentionally leaked (see above)
  return *p;
}
void ctx_pool_put(dlsm_ctx* c);
struct ThreadCtx {
  dlsm_ctx* owned = nullptr;
  dlsm_ctx* bound = nullptr;
  ~ThreadCtx() {
    if (owned) ctx_pool_put(owned);
  }
};
ThreadCtx& thread_ctx_slot() {
  thread_local ThreadCtx t;
  return t;
}
std::atomic<unsigned> g_thread_ctx_next{0};
std::atomic<uint64_t> g_fallbacks{0};  // dlsm_fallback_note, process-wide
}  // namespace
extern "C" {

int dlsm_thread_ctx(dlsm_ctx** out) {
  if (!out) return DLSM_E_ARG;
  ThreadCtx& t = thread_ctx_slot();
  if (t.bound) {
    *out = t.bound;
    return DLSM_OK;
  }
  if (!t.owned) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
      *out = nullptr;
      return DLSM_E_DEVICE;
    }
    const int dev = static_cast<int>(g_thread_ctx_next.fetch_add(1) % static_cast<unsigned>(n));
    CtxPool& p = ctx_pool();
    {
      std::lock_guard<std::mutex> lk(p.m);
      auto& v = p.free[dev];
      if (!v.empty()) {
        t.owned = v.back();
        v.pop_back();
        p.reused++;
      }
    }
    if (!t.owned) {
      DLSM_CHECK(dlsm_ctx_create(dev, &t.owned));
      t.owned->opts0 = CtxOpts{t.owned->path,      t.owned->build_groups, t.owned->probe_round,
                               t.owned->probe_lgc, t.owned->probe_lgr,    t.owned->build_exact,
                               t.owned->probe_serial, t.owned->probe_multi};
      t.owned->opts0_set = true;
      std::lock_guard<std::mutex> lk(p.m);
      p.created++;
    }
  }
  *out = t.owned;
  return DLSM_OK;
}

int dlsm_thread_ctx_bind(dlsm_ctx* ctx) {
  thread_ctx_slot().bound = ctx;
  return DLSM_OK;
}

int dlsm_thread_ctx_stats(uint64_t* created, uint64_t* reused, uint64_t* idle) {
  CtxPool& p = ctx_pool();
  std::lock_guard<std::mutex> lk(p.m);
  uint64_t n = 0;
  for (auto& kv : p.free) n += kv.second.size();
  if (created) *created = p.created;
  if (reused) *reused = p.reused;
  if (idle) *idle = n;
  return DLSM_OK;
}

void dlsm_fallback_note(dlsm_ctx* ctx) {
  g_fallbacks.fetch_add(1, std::memory_order_relaxed);
  if (ctx) ctx->fallbacks.fetch_add(1, std::memory_order_relaxed);
}

int dlsm_fallback_stats(const dlsm_ctx* ctx, uint64_t* ctx_count, uint64_t* process_count) {
  if (ctx_count) *ctx_count = ctx ? ctx->fallbacks.load(std::memory_order_relaxed) : 0;
  if (process_count) *process_count = g_fallbacks.load(std::memory_order_relaxed);
  return DLSM_OK;
}

int dlsm_ctx_create(int device, dlsm_ctx** out) {
  if (!out) return DLSM_E_ARG;
  *out = nullptr;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess || device < 0 || device >= c) return DLSM_E_DEVICE;
  DeviceGuard g(device);
  dlsm_ctx* ctx = new (std::nothrow) dlsm_ctx();
  if (!ctx) return DLSM_E_NOMEM;
  ctx->device = device;
  hipError_t e = hipStreamCreateWithFlags(&ctx->own, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_pfork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_pdone, hipEventDisableTiming);
  for (int b = 0; b < kStageEvents && e == hipSuccess; b++) {
    e = hipEventCreateWithFlags(&ctx->ev_part[b], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_free[b], hipEventDisableTiming);
  }
  if (e == hipSuccess)
    e = hipHostMalloc(reinterpret_cast<void**>(&ctx->up_block), dlsm_ctx::kUpSlots * dlsm_ctx::kUpSlotBytes,
                      hipHostMallocDefault);
  for (int i = 0; i < dlsm_ctx::kUpSlots && e == hipSuccess; i++) {
    ctx->up_buf[i] = ctx->up_block + i * dlsm_ctx::kUpSlotBytes;
    ctx->up_cap[i] = dlsm_ctx::kUpSlotBytes;
    e = hipEventCreateWithFlags(&ctx->up_ev[i], hipEventDisableTiming);
  }
  if (const char* v = getenv("DLSM_HOST_SYNC")) ctx->host_sync = atoi(v);
  if (e == hipSuccess)
    e = hipEventCreateWithFlags(&ctx->ev_wait, hipEventDisableTiming |
                                                   (ctx->host_sync == 2 ? hipEventBlockingSync : 0u));
  ctx->stream = ctx->own;
  if (e != hipSuccess) {
    dlsm_ctx_destroy(ctx);
    return from_hip(e);
  }
  if (const char* v = getenv("DLSM_PROBE_ROUND_KEYS")) ctx->probe_round = strtoull(v, nullptr, 10);
  if (const char* v = getenv("DLSM_PROBE_CHUNK_LG")) dlsm_ctx_set_option(ctx, DLSM_OPT_PROBE_CHUNK_LG, strtoull(v, nullptr, 10));
  if (const char* v = getenv("DLSM_PROBE_SLICE_LG")) dlsm_ctx_set_option(ctx, DLSM_OPT_PROBE_SLICE_LG, strtoull(v, nullptr, 10));
  if (const char* v = getenv("DLSM_PROBE_SERIAL")) ctx->probe_serial = atoi(v) != 0;
  if (const char* v = getenv("DLSM_PROBE_MULTI")) ctx->probe_multi = atoi(v) != 0;
  *out = ctx;
  return DLSM_OK;
}

int dlsm_ctx_destroy(dlsm_ctx* ctx) {
  if (!ctx) return DLSM_OK;
  DeviceGuard g(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->aux) (void)hipStreamSynchronize(ctx->aux);
  if (ctx->pstream) (void)hipStreamSynchronize(ctx->pstream);
  ctx->entries.release();
  ctx->tab.release();
  ctx->jobs.release();
  ctx->starts.release();
  ctx->dchunk.release();
  ctx->jobL.release();
  ctx->ljobs.release();
  ctx->lstarts.release();
  ctx->ltjobs.release();
  ctx->ltstarts.release();
  ctx->lentries.release();
  ctx->ltab.release();
  ctx->pos.release();
  ctx->hashes.release();
  ctx->vgl.release();
  ctx->vabyte.release();
  ctx->vplan.release();
  ctx->smask.release();
  ctx->plan_ws.release();
  ctx->route_ws.release();
  ctx->kv_ws.release();
  ctx->sel.release();
  ctx->st_keys.release();
  ctx->st_offs.release();
  ctx->st_out.release();
  ctx->st_len.release();
  ctx->st_filter.release();
  ctx->crc_streams.release();
  ctx->crc_partial.release();
  ctx->crc_tabs.release();
  ctx->crc_outp.release();
  ctx->crc_cap.release();
  ctx->crc_val.release();
  ctx->ing_blocks.release();
  ctx->ing_part0.release();
  ctx->ing_partial.release();
  ctx->ing_rec.release();
  for (hipEvent_t e : ctx->ev_kv)
    if (e) (void)hipEventDestroy(e);
  if (ctx->ev_ing0) (void)hipEventDestroy(ctx->ev_ing0);
  if (ctx->ev_ing1) (void)hipEventDestroy(ctx->ev_ing1);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_wait) (void)hipEventDestroy(ctx->ev_wait);
  if (ctx->ev_pfork) (void)hipEventDestroy(ctx->ev_pfork);
  if (ctx->ev_pdone) (void)hipEventDestroy(ctx->ev_pdone);
  for (int b = 0; b < kStageEvents; b++) {
    if (ctx->ev_part[b]) (void)hipEventDestroy(ctx->ev_part[b]);
    if (ctx->ev_free[b]) (void)hipEventDestroy(ctx->ev_free[b]);
  }
  if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
  if (ctx->own) (void)hipStreamDestroy(ctx->own);
  if (ctx->host_buf) (void)hipHostFree(ctx->host_buf);
  if (ctx->h_out) (void)hipHostFree(ctx->h_out);
  if (ctx->h_len) (void)hipHostFree(ctx->h_len);
  for (int i = 0; i < dlsm_ctx::kUpSlots; i++) {
    if (ctx->up_own[i]) (void)hipHostFree(ctx->up_buf[i]);
    if (ctx->up_ev[i]) (void)hipEventDestroy(ctx->up_ev[i]);
  }
  if (ctx->up_block) (void)hipHostFree(ctx->up_block);
  delete ctx;
  return DLSM_OK;
}

}  // extern "C"
namespace {
// A thread's context back to its device's free list: drained, its stream and
// partition stream reset to its own, its scheduling options to their
// creation values, fault injection off.
void ctx_pool_put(dlsm_ctx* c) {
  {
    DeviceGuard g(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->pstream) (void)hipStreamSynchronize(c->pstream);
  }
  c->stream = c->own;
  c->pstream = nullptr;
  c->pcus = 0;
  c->fault = 0;
  c->vslice_bytes = 0;
  c->vpass_slices = kVMaxSlices;
  c->fallbacks.store(0, std::memory_order_relaxed);  // the next thread's count starts at zero
  if (c->opts0_set) {
    const CtxOpts& o = c->opts0;
    c->path = o.path;
    c->build_groups = o.build_groups;
    c->probe_round = o.probe_round;
    c->probe_lgc = o.probe_lgc;
    c->probe_lgr = o.probe_lgr;
    c->build_exact = o.build_exact;
    c->probe_serial = o.probe_serial;
    c->probe_multi = o.probe_multi;
  }
  CtxPool& p = ctx_pool();
  std::lock_guard<std::mutex> lk(p.m);
  p.free[c->device].push_back(c);
}
}  // namespace
extern "C" {

int dlsm_ctx_set_stream(dlsm_ctx* ctx, void* s) {
  if (!ctx) return DLSM_E_ARG;
  ctx->stream = s ? static_cast<hipStream_t>(s) : ctx->own;
  return DLSM_OK;
}

void* dlsm_ctx_stream(dlsm_ctx* ctx) { return ctx ? static_cast<void*>(ctx->stream) : nullptr; }

int dlsm_ctx_device(const dlsm_ctx* ctx) { return ctx ? ctx->device : -1; }

int dlsm_ctx_set_partition_stream(dlsm_ctx* ctx, void* s, uint32_t cus) {
  if (!ctx) return DLSM_E_ARG;
  ctx->pstream = static_cast<hipStream_t>(s);
  ctx->pcus = s ? cus : 0u;
  return DLSM_OK;
}

int dlsm_stream_create_cu_mask(int device, const uint32_t* mask, uint32_t words, void** out) {
  if (!out || !mask || words == 0) return DLSM_E_ARG;
  *out = nullptr;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess || device < 0 || device >= c) return DLSM_E_DEVICE;
  DeviceGuard g(device);
  hipStream_t st = nullptr;
  DLSM_TRY(hipExtStreamCreateWithCUMask(&st, words, mask));  // size in uint32 elements
  *out = st;
  return DLSM_OK;
}

int dlsm_stream_destroy(void* s) {
  if (!s) return DLSM_E_ARG;
  DLSM_TRY(hipStreamDestroy(static_cast<hipStream_t>(s)));
  return DLSM_OK;
}

int dlsm_ctx_sync(dlsm_ctx* ctx) {
  if (!ctx) return DLSM_E_ARG;
  DeviceGuard g(ctx->device);
  DLSM_TRY(ctx_sync(ctx, ctx->stream));
  return DLSM_OK;
}

int dlsm_ctx_set_path(dlsm_ctx* ctx, int path) {
  if (!ctx || path < 0 || path > 2) return DLSM_E_ARG;
  ctx->path = path;
  return DLSM_OK;
}

int dlsm_ctx_set_option(dlsm_ctx* ctx, int option, uint64_t value) {
  if (!ctx) return DLSM_E_ARG;
  switch (option) {
    case DLSM_OPT_PATH:
      return value > 2 ? DLSM_E_ARG : dlsm_ctx_set_path(ctx, static_cast<int>(value));
    case DLSM_OPT_PROBE_ROUND_KEYS:
      ctx->probe_round = value;
      return DLSM_OK;
    case DLSM_OPT_BUILD_GROUPS:
      if (value > static_cast<uint64_t>(kStageEvents)) return DLSM_E_ARG;
      ctx->build_groups = value ? static_cast<int>(value) : 1;
      return DLSM_OK;
    case DLSM_OPT_PROBE_CHUNK_LG:
      if (value < 12 || value > 14) return DLSM_E_ARG;
      ctx->probe_lgc = static_cast<int>(value);
      return DLSM_OK;
    case DLSM_OPT_PROBE_SLICE_LG:
      if (value < 7 || value > 8) return DLSM_E_ARG;
      ctx->probe_lgr = static_cast<int>(value);
      return DLSM_OK;
    case DLSM_OPT_BUILD_EXACT:
      if (value > 2) return DLSM_E_ARG;
      ctx->build_exact = static_cast<int>(value);
      return DLSM_OK;
    case DLSM_OPT_PROBE_ROUND_SERIAL:
      if (value > 1) return DLSM_E_ARG;
      ctx->probe_serial = value != 0;
      return DLSM_OK;
    case DLSM_OPT_FAULT_INJECT:
      if (value > static_cast<uint64_t>(-DLSM_E_BUSY)) return DLSM_E_ARG;
      ctx->fault = static_cast<int>(value);
      return DLSM_OK;
    case DLSM_OPT_VERSION_SLICE_BYTES:
      ctx->vslice_bytes = value;
      return DLSM_OK;
    case DLSM_OPT_VERSION_PASS_SLICES:
      if (value < 1 || value > kVMaxSlices) return DLSM_E_ARG;
      ctx->vpass_slices = static_cast<uint32_t>(value);
      return DLSM_OK;
    case DLSM_OPT_PROBE_MULTI:
      if (value > 1) return DLSM_E_ARG;
      ctx->probe_multi = static_cast<int>(value);
      return DLSM_OK;
    default:
      return DLSM_E_ARG;
  }
}

int dlsm_ctx_get_option(dlsm_ctx* ctx, int option, uint64_t* value) {
  if (!ctx || !value) return DLSM_E_ARG;
  switch (option) {
    case DLSM_OPT_PATH: *value = static_cast<uint64_t>(ctx->path); return DLSM_OK;
    case DLSM_OPT_PROBE_ROUND_KEYS: *value = ctx->probe_round; return DLSM_OK;
    case DLSM_OPT_BUILD_GROUPS: *value = static_cast<uint64_t>(ctx->build_groups); return DLSM_OK;
    case DLSM_OPT_PROBE_CHUNK_LG: *value = static_cast<uint64_t>(ctx->probe_lgc); return DLSM_OK;
    case DLSM_OPT_PROBE_SLICE_LG: *value = static_cast<uint64_t>(ctx->probe_lgr); return DLSM_OK;
    case DLSM_OPT_BUILD_EXACT: *value = static_cast<uint64_t>(ctx->build_exact); return DLSM_OK;
    case DLSM_OPT_PROBE_ROUND_SERIAL: *value = ctx->probe_serial ? 1u : 0u; return DLSM_OK;
    case DLSM_OPT_FAULT_INJECT: *value = static_cast<uint64_t>(ctx->fault); return DLSM_OK;
    case DLSM_OPT_VERSION_SLICE_BYTES: *value = ctx->vslice_bytes; return DLSM_OK;
    case DLSM_OPT_VERSION_PASS_SLICES: *value = ctx->vpass_slices; return DLSM_OK;
    case DLSM_OPT_PROBE_MULTI: *value = static_cast<uint64_t>(ctx->probe_multi); return DLSM_OK;
    default: return DLSM_E_ARG;
  }
}

int dlsm_ctx_reserve(dlsm_ctx* ctx, uint64_t max_keys, uint32_t max_jobs) {
  if (!ctx) return DLSM_E_ARG;
  DeviceGuard g(ctx->device);
  // probe intermediates are sized in whole chunks of up to 2^14 keys
  const uint64_t pkeys = (max_keys + 16383u) & ~uint64_t(16383u);
  // probe entries / answers: chunk regions of probe_region(C) per C keys
  uint64_t pregion = 0;
  for (uint32_t C : {4096u, 8192u, 16384u})
    pregion = std::max<uint64_t>(pregion, ((max_keys + C - 1) / C) * probe_region(C));
  const uint64_t bregion = ((max_keys + kBuildChunk - 1) / kBuildChunk + max_jobs) * kBuildRegion;
  DLSM_CHECK(ctx->entries.ensure(std::max({pkeys, pregion, bregion})));
  DLSM_CHECK(ctx->pos.ensure(pkeys));
  DLSM_CHECK(ctx->smask.ensure(pregion));
  const uint64_t chunks = (max_keys + kBuildChunk - 1) / kBuildChunk + max_jobs;
  DLSM_CHECK(ctx->tab.ensure(chunks * (kMaxSlices + 1)));
  DLSM_CHECK(ctx->jobs.ensure(max_jobs));
  DLSM_CHECK(ctx->starts.ensure(2 * (max_jobs + 1)));
  DLSM_CHECK(ctx->dchunk.ensure(chunks));
  DLSM_CHECK(ctx->jobL.ensure(max_jobs));
  return DLSM_OK;
}

int dlsm_ctx_stats(dlsm_ctx* ctx, uint64_t* device_allocs, uint64_t* device_bytes) {
  if (!ctx) return DLSM_E_ARG;
  uint64_t n = 0, b = 0;
  auto add = [&](const auto& buf) {
    n += buf.gen;
    b += buf.cap * sizeof(*buf.p);
  };
  add(ctx->entries); add(ctx->tab); add(ctx->jobs); add(ctx->starts); add(ctx->dchunk);
  add(ctx->jobL); add(ctx->ljobs); add(ctx->lstarts); add(ctx->ltjobs); add(ctx->ltstarts);
  add(ctx->lentries); add(ctx->ltab); add(ctx->pos); add(ctx->smask); add(ctx->hashes);
  add(ctx->vgl); add(ctx->vabyte); add(ctx->vplan); add(ctx->plan_ws); add(ctx->route_ws);
  add(ctx->st_keys); add(ctx->st_offs); add(ctx->st_out); add(ctx->st_len); add(ctx->st_filter);
  add(ctx->crc_streams); add(ctx->crc_partial); add(ctx->crc_tabs); add(ctx->crc_outp); add(ctx->crc_cap);
  add(ctx->crc_val); add(ctx->sel); add(ctx->kv_ws);
  if (device_allocs) *device_allocs = n;
  if (device_bytes) *device_bytes = b;
  return DLSM_OK;
}

int dlsm_host_register(void* p, size_t len) {
  if (!p || !len) return DLSM_E_ARG;
  DLSM_TRY(hipHostRegister(p, len, hipHostRegisterDefault));
  return DLSM_OK;
}

int dlsm_host_unregister(void* p) {
  if (!p) return DLSM_E_ARG;
  DLSM_TRY(hipHostUnregister(p));
  return DLSM_OK;
}

int dlsm_ctx_host_buffer_claim(dlsm_ctx* ctx, const void* owner) {
  if (!ctx || !owner) return DLSM_E_ARG;
  const void* cur = nullptr;
  if (ctx->host_owner.compare_exchange_strong(cur, owner) || cur == owner) return DLSM_OK;
  return DLSM_E_BUSY;
}

int dlsm_ctx_host_buffer_release(dlsm_ctx* ctx, const void* owner) {
  if (!ctx || !owner) return DLSM_E_ARG;
  const void* cur = owner;
  return ctx->host_owner.compare_exchange_strong(cur, nullptr) ? DLSM_OK : DLSM_E_ARG;
}

int dlsm_ctx_host_buffer(dlsm_ctx* ctx, uint64_t min_bytes, uint64_t keep_bytes, void** out,
                         uint64_t* cap) {
  if (!ctx || !out || keep_bytes > ctx->host_cap) return DLSM_E_ARG;
  if (min_bytes > ctx->host_cap || !ctx->host_buf) {
    uint64_t c = std::max<uint64_t>(ctx->host_cap ? 2 * ctx->host_cap : (uint64_t(1) << 20), min_bytes);
    void* p = nullptr;
    DLSM_TRY(hipHostMalloc(&p, c, hipHostMallocDefault));
    if (keep_bytes) memcpy(p, ctx->host_buf, keep_bytes);
    if (ctx->host_buf) {
      // the previous buffer may still be the source of a queued copy
      (void)hipStreamSynchronize(ctx->stream);
      (void)hipHostFree(ctx->host_buf);
    }
    ctx->host_buf = p;
    ctx->host_cap = c;
  }
  *out = ctx->host_buf;
  if (cap) *cap = ctx->host_cap;
  return DLSM_OK;
}

// Process-wide pool of page-locked host buffers (key staging of builders
// that cannot borrow their context's buffer): a released buffer is kept and
// handed to the next acquire that fits, so steady-state staging page-locks
// nothing.  Sizes are powers of two >= 1 MiB.  At most kPoolKeepBytes of
// released buffers are kept (a burst of builders does not pin host memory
// for good); a release past that frees the buffer.
}  // extern "C"
namespace {
constexpr uint64_t kPoolKeepBytes = uint64_t(1) << 30;
struct HostPool {
  std::mutex m;
  std::multimap<uint64_t, void*> free_by_size;
  struct Entry {
    uint64_t size;
    bool in_use;
  };
  std::unordered_map<void*, Entry> entry;
  uint64_t free_bytes = 0;
};
HostPool& host_pool() {
  static HostPool p;
  return p;
}
}  // namespace
extern "C" {

int dlsm_host_pool_acquire(uint64_t min_bytes, void** out, uint64_t* cap) {
  if (!out) return DLSM_E_ARG;
  *out = nullptr;
  HostPool& hp = host_pool();
  {
    std::lock_guard<std::mutex> lk(hp.m);
    auto it = hp.free_by_size.lower_bound(min_bytes);
    if (it != hp.free_by_size.end()) {
      *out = it->second;
      if (cap) *cap = it->first;
      hp.free_bytes -= it->first;
      hp.entry[it->second].in_use = true;
      hp.free_by_size.erase(it);
      return DLSM_OK;
    }
  }
  uint64_t c = uint64_t(1) << 20;
  while (c < min_bytes) c <<= 1;
  void* p = nullptr;
  DLSM_TRY(hipHostMalloc(&p, c, hipHostMallocDefault));
  {
    std::lock_guard<std::mutex> lk(hp.m);
    hp.entry[p] = HostPool::Entry{c, true};
  }
  *out = p;
  if (cap) *cap = c;
  return DLSM_OK;
}

// DLSM_E_ARG for a pointer the pool did not hand out, or one already released
// (a double release would give one buffer to two later acquirers).
int dlsm_host_pool_release(void* p) {
  if (!p) return DLSM_OK;
  HostPool& hp = host_pool();
  void* drop = nullptr;
  {
    std::lock_guard<std::mutex> lk(hp.m);
    auto it = hp.entry.find(p);
    if (it == hp.entry.end() || !it->second.in_use) return DLSM_E_ARG;
    if (hp.free_bytes + it->second.size > kPoolKeepBytes) {
      drop = p;
      hp.entry.erase(it);
    } else {
      it->second.in_use = false;
      hp.free_by_size.emplace(it->second.size, p);
      hp.free_bytes += it->second.size;
    }
  }
  if (drop) DLSM_TRY(hipHostFree(drop));
  return DLSM_OK;
}

int dlsm_host_pool_trim(void) {
  HostPool& hp = host_pool();
  std::lock_guard<std::mutex> lk(hp.m);
  for (auto& kv : hp.free_by_size) {
    (void)hipHostFree(kv.second);
    hp.entry.erase(kv.second);
  }
  hp.free_by_size.clear();
  hp.free_bytes = 0;
  return DLSM_OK;
}

int dlsm_host_alloc(size_t len, void** out) {
  if (!out || !len) return DLSM_E_ARG;
  *out = nullptr;
  DLSM_TRY(hipHostMalloc(out, len, hipHostMallocDefault));
  return DLSM_OK;
}

int dlsm_host_free(void* p) {
  if (!p) return DLSM_OK;
  DLSM_TRY(hipHostFree(p));
  return DLSM_OK;
}

// ---------------------------------------------------------------------------
// Full filter build
// ---------------------------------------------------------------------------
namespace {

// Hashed jobs: keys.bytes holds n BloomHash values (u32, 4-byte aligned,
// key_len 4, no offsets) -- what AddKey computed on the host.
bool is_hash_set(const dlsm_keyset& k) {
  return k.offsets == nullptr && k.key_len == 4 && k.suffix_len == 0 && (k.n == 0 || aligned(k.bytes, 4));
}

// seal (dlsm_bloom_full_build_block_dev): on the sliced path the slices also
// compute their crc32c partials and a seal kernel appends the block trailer
// (*sealed = true); the direct path leaves sealing to the caller.
int full_build_dev_impl(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs, int bits_per_key,
                        uint64_t* out_len_dev, bool hashed, bool seal = false, bool* sealed = nullptr) {
  if (sealed) *sealed = false;
  if (!ctx || n_jobs < 0 || (n_jobs > 0 && (!jobs || !out_len_dev))) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  if (n_jobs == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  std::vector<uint32_t> Ls(n_jobs);
  bool all_k20 = true, all_k28 = true, sliced_ok = ctx->path != 1;
  for (int j = 0; j < n_jobs; j++) {
    const dlsm_build_job& b = jobs[j];
    DLSM_CHECK(validate_keyset(b.keys));
    if (hashed && !is_hash_set(b.keys)) return DLSM_E_ARG;
    if (!b.out || !aligned(b.out, 16)) return DLSM_E_ARG;
    if (b.keys.n > 0xffffffffull * kBuildChunk) return DLSM_E_ARG;
    Ls[j] = full_num_lines(b.keys.n, bits_per_key, nullptr);
    all_k20 = all_k20 && is_k20(b.keys);
    all_k28 = all_k28 && is_k28(b.keys);
  }
  int lgR = choose_build_lgR(Ls);
  if (lgR < 0) sliced_ok = false;
  if (ctx->path == 2 && !sliced_ok) return DLSM_E_ARG;
  const int mode = hashed ? KM_HASH : (all_k20 ? KM_K20 : (all_k28 ? KM_K28 : KM_GENERIC));
  // Exact line counts (a count pass before the partition) where duplicate
  // user keys are expected to lower L below the speculative n-key count:
  // internal keys (several versions of a user key, suffix_len 8) and the
  // per-key-length batches a TableBuilder adapter hands over.  The
  // device-resident fixed-length user-key batches (one entry per user key)
  // stay speculative: one pass over the keys, with a per-slice re-hash
  // fallback for the rare batch whose duplicates do change L.
  bool any_suffix = false;
  for (int j = 0; j < n_jobs; j++) any_suffix = any_suffix || jobs[j].keys.suffix_len > 0;
  // Hashed jobs always count first: the entries keep no key to re-hash, so
  // the slice pass's fallback for a lowered line count is not available.
  const bool exact = sliced_ok && (hashed || ctx->build_exact == 1 ||
                                   (ctx->build_exact == 0 && (any_suffix || mode == KM_GENERIC)));

  const JobTable<FullJobDev> T = plan_full_jobs(jobs, n_jobs, bits_per_key, out_len_dev, Ls, lgR, sliced_ok, exact);
  const std::vector<FullJobDev>& hj = T.hj;
  const std::vector<uint32_t>& starts = T.starts;
  const uint64_t entry = T.entry, tabw = T.tabw;
  const uint32_t chunk = T.chunk, slice = T.slice;
  hipStream_t s = ctx->stream;
  const bool same = ctx->last_jobs.size() == hj.size() && ctx->last_starts == starts &&
                    memcmp(ctx->last_jobs.data(), hj.data(), sizeof(FullJobDev) * n_jobs) == 0 &&
                    ctx->jobs.gen == ctx->last_jobs_gen && ctx->starts.gen == ctx->last_starts_gen &&
                    ctx->jobs.cap >= static_cast<size_t>(n_jobs);
  if (!same) {
    ctx->last_jobs.clear();  // until the upload below is queued
    DLSM_CHECK(ctx->jobs.ensure(n_jobs));
    DLSM_CHECK(ctx->starts.ensure(2 * n_jobs));
    DLSM_CHECK(ctx_upload(ctx, ctx->jobs.p, hj.data(), sizeof(FullJobDev) * n_jobs, s));
    DLSM_CHECK(ctx_upload(ctx, ctx->starts.p, starts.data(), sizeof(uint32_t) * 2 * n_jobs, s));
    ctx->last_jobs = hj;
    ctx->last_starts = starts;
    ctx->last_jobs_gen = ctx->jobs.gen;
    ctx->last_starts_gen = ctx->starts.gen;
  }
  DLSM_CHECK(ctx->dchunk.ensure(chunk));
  DLSM_CHECK(ctx->jobL.ensure(n_jobs));
  const uint32_t* chunk0s = ctx->starts.p;
  const uint32_t* slice0s = ctx->starts.p + n_jobs;
  if (sliced_ok) {
    DLSM_CHECK(ctx->entries.ensure(entry));
    DLSM_CHECK(ctx->tab.ensure(tabw));
    uint32_t* crc_part = nullptr;
    if (seal) {
      DLSM_CHECK(ctx->crc_partial.ensure(slice));
      if (ctx->crc_tabs_lgr != lgR || ctx->crc_tabs.gen != ctx->crc_tabs_gen) {
        DLSM_CHECK(ctx->crc_tabs.ensure(kCrcTabWords));
        std::vector<uint32_t> t(kCrcTabWords);
        full_block_crc_tables(lgR, t.data());
        DLSM_CHECK(ctx_upload(ctx, ctx->crc_tabs.p, t.data(), sizeof(uint32_t) * kCrcTabWords, s));
        ctx->crc_tabs_lgr = lgR;
        ctx->crc_tabs_gen = ctx->crc_tabs.gen;
      }
      crc_part = ctx->crc_partial.p;
    }
    // Job groups of about equal chunk counts: group g's partition (HBM-bound)
    // runs on the helper stream while the context stream runs group g-1's
    // slices (LDS-bound).
    const int G = std::max(1, std::min(ctx->build_groups, n_jobs));
    const std::vector<int> cut = job_group_cuts(starts, chunk, n_jobs, G);
    const int ng = static_cast<int>(cut.size()) - 1;
    auto chunk_at = [&](int j) { return j < n_jobs ? starts[j] : chunk; };
    auto slice_at = [&](int j) { return j < n_jobs ? starts[n_jobs + j] : slice; };
    // partition stream (dlsm_ctx_set_partition_stream, one job group): the
    // count and partition passes there, the slices on the context stream
    const bool split = ctx->pstream && ng == 1;
    hipStream_t ps = split ? ctx->pstream : s;
    if (split) DLSM_CHECK(fork_part(ctx));
    if (exact) DLSM_TRY(launch_full_count(ctx->jobs.p, chunk0s, n_jobs, chunk, ctx->dchunk.p, mode, ps));
    if (ng > 1) DLSM_CHECK(fork_aux(ctx));
    for (int g = 0; g < ng; g++) {
      const uint32_t c0 = chunk_at(cut[g]), s0 = slice_at(cut[g]);
      DLSM_TRY(launch_full_partition(ctx->jobs.p, chunk0s, n_jobs, c0, chunk_at(cut[g + 1]) - c0,
                                     ctx->dchunk.p, ctx->entries.p, ctx->tab.p, lgR, mode, exact,
                                     ng > 1 ? ctx->aux : ps));
      if (split) DLSM_CHECK(join_part(ctx));
      if (ng > 1) DLSM_CHECK(hand_over(ctx->aux, s, ctx->ev_part[g % kStageEvents]));
      DLSM_TRY(launch_full_slices(ctx->jobs.p, slice0s, n_jobs, s0, slice_at(cut[g + 1]) - s0,
                                  ctx->dchunk.p, ctx->entries.p, ctx->tab.p, lgR, s, crc_part,
                                  ctx->crc_tabs.p));
    }
    if (seal) {
      DLSM_TRY(launch_full_block_seal(ctx->jobs.p, n_jobs, crc_part, ctx->crc_tabs.p, lgR, s));
      if (sealed) *sealed = true;
    }
  } else {
    DLSM_TRY(launch_full_count(ctx->jobs.p, chunk0s, n_jobs, chunk, ctx->dchunk.p, mode, s));
    DLSM_TRY(launch_full_zero(ctx->jobs.p, n_jobs, ctx->dchunk.p, ctx->jobL.p, s));
    DLSM_TRY(launch_full_scatter(ctx->jobs.p, chunk0s, n_jobs, chunk, ctx->jobL.p, mode, s));
  }
  return DLSM_OK;
}

}  // namespace

int dlsm_bloom_full_build_dev(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs,
                              int bits_per_key, uint64_t* out_len_dev) {
  return full_build_dev_impl(ctx, jobs, n_jobs, bits_per_key, out_len_dev, false);
}

int dlsm_bloom_full_build_hashed_dev(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs,
                                     int bits_per_key, uint64_t* out_len_dev) {
  return full_build_dev_impl(ctx, jobs, n_jobs, bits_per_key, out_len_dev, true);
}

namespace {

// Stage host keysets into one device buffer; returns per-job device keysets.
// Variable-length sets are copied from offsets[0] and their offsets rebased.
int stage_keys(dlsm_ctx* ctx, const dlsm_keyset* const* sets, int n, std::vector<dlsm_keyset>& dev) {
  hipStream_t s = ctx->stream;
  uint64_t bytes = 0, offs = 0;
  std::vector<uint64_t> bpos(n), opos(n), src0(n), nb(n);
  for (int j = 0; j < n; j++) {
    const dlsm_keyset& k = *sets[j];
    src0[j] = (k.offsets && k.n) ? k.offsets[0] : 0;
    nb[j] = k.n == 0 ? 0 : (k.offsets ? k.offsets[k.n] - k.offsets[0] : k.n * uint64_t(k.key_len));
    bpos[j] = bytes;
    bytes += (nb[j] + 15) & ~uint64_t(15);
    opos[j] = offs;
    if (k.offsets) offs += k.n + 1;
  }
  DLSM_CHECK(ctx->st_keys.ensure(bytes + 16));
  DLSM_CHECK(ctx->st_offs.ensure(offs + 1));
  dev.resize(n);
  for (int j = 0; j < n; j++) {
    const dlsm_keyset& k = *sets[j];
    dlsm_keyset d = k;
    d.bytes = ctx->st_keys.p + bpos[j];
    if (nb[j])
      DLSM_TRY(hipMemcpyAsync(const_cast<uint8_t*>(d.bytes), k.bytes + src0[j], nb[j],
                              hipMemcpyHostToDevice, s));
    if (k.offsets) {
      std::vector<uint64_t> ro(k.n + 1);
      for (uint64_t i = 0; i <= k.n; i++) ro[i] = k.offsets[i] - src0[j];
      d.offsets = ctx->st_offs.p + opos[j];
      DLSM_CHECK(ctx_upload(ctx, const_cast<uint64_t*>(d.offsets), ro.data(), sizeof(uint64_t) * (k.n + 1), s));
    }
    dev[j] = d;
  }
  return DLSM_OK;
}

}  // namespace

namespace {
// Grow a page-locked host array (contents dropped; the context stream is idle
// between host-API calls, so no queued command still uses the old one).
extern "C++" template <typename T>
int host_ensure(T*& p, uint64_t& cap, uint64_t n) {
  if (n <= cap && p) return DLSM_OK;
  if (p) (void)hipHostFree(p);
  p = nullptr;
  cap = 0;
  const uint64_t want = std::max<uint64_t>(n, 64);
  DLSM_TRY(hipHostMalloc(reinterpret_cast<void**>(&p), want * sizeof(T), hipHostMallocDefault));
  cap = want;
  return DLSM_OK;
}

// The device address of a page-locked host pointer (hipHostMalloc'd, or
// registered: dlsm_host_register), or nullptr for pageable memory.
uint8_t* host_device_view(void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // not HIP memory: clear the error the query left
    return nullptr;
  }
  if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
  const uintptr_t off = a.hostPointer ? reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(a.hostPointer) : 0;
  return static_cast<uint8_t*>(a.devicePointer) + off;
}

// Whether full_build_dev_impl takes the sliced path for this batch (the
// same choice it makes: not forced direct, and a slice width that fits).
bool full_build_sliced(const dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs, int bits_per_key) {
  if (ctx->path == 1) return false;
  std::vector<uint32_t> Ls(n_jobs);
  for (int j = 0; j < n_jobs; j++) Ls[j] = full_num_lines(jobs[j].keys.n, bits_per_key, nullptr);
  return choose_build_lgR(Ls) >= 0;
}

// Host keys -> host filters.  The keys go H2D into the context's staging.
// Sliced path: the slice kernels store each filter straight into the
// caller's slot when it is page-locked (16-byte aligned), else into
// page-locked staging copied out after the call, and the lengths into
// page-locked memory -- one stream synchronisation per call and no
// device-to-host copy commands; their stores are plain 16-byte writes.  The
// direct path (forced, or a batch too large to slice) sets bits with global
// atomics, which must not target host memory (that would need PCIe
// AtomicOps): it builds into device staging and copies the filters out.
int full_build_host_impl(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs, int bits_per_key,
                         uint64_t* out_len, bool hashed) {
  if (!ctx || n_jobs < 0 || (n_jobs > 0 && (!jobs || !out_len))) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  if (n_jobs == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  std::vector<const dlsm_keyset*> sets(n_jobs);
  for (int j = 0; j < n_jobs; j++) {
    DLSM_CHECK(validate_keyset(jobs[j].keys));
    if (!jobs[j].out) return DLSM_E_ARG;
    sets[j] = &jobs[j].keys;
  }
  const bool to_host = full_build_sliced(ctx, jobs, n_jobs, bits_per_key);
  std::vector<dlsm_keyset> dk;
  DLSM_CHECK(stage_keys(ctx, sets.data(), n_jobs, dk));
  std::vector<dlsm_build_job> dj(n_jobs);
  std::vector<uint8_t*> direct(n_jobs);
  uint64_t obytes = 0;
  std::vector<uint64_t> opos(n_jobs);
  for (int j = 0; j < n_jobs; j++) {
    const uint64_t spec = full_filter_len(jobs[j].keys.n, bits_per_key);
    const uint64_t cap = std::min(spec, jobs[j].out_cap);
    direct[j] = to_host ? host_device_view(jobs[j].out) : nullptr;
    if (direct[j] && !aligned(direct[j], 16)) direct[j] = nullptr;
    opos[j] = obytes;
    if (!direct[j]) obytes += (cap + 255) & ~uint64_t(255);
    dj[j].keys = dk[j];
    dj[j].out_cap = cap;
  }
  hipStream_t s = ctx->stream;
  if (!to_host) {
    DLSM_CHECK(ctx->st_out.ensure(obytes + 256));
    DLSM_CHECK(ctx->st_len.ensure(n_jobs));
    for (int j = 0; j < n_jobs; j++) dj[j].out = ctx->st_out.p + opos[j];
    DLSM_CHECK(full_build_dev_impl(ctx, dj.data(), n_jobs, bits_per_key, ctx->st_len.p, hashed));
    DLSM_TRY(hipMemcpyAsync(out_len, ctx->st_len.p, sizeof(uint64_t) * n_jobs, hipMemcpyDeviceToHost, s));
    DLSM_TRY(ctx_sync(ctx, s));
    int st = DLSM_OK;
    for (int j = 0; j < n_jobs; j++) {
      if (out_len[j] == 0) {
        st = DLSM_E_CAPACITY;
        continue;
      }
      DLSM_TRY(hipMemcpyAsync(jobs[j].out, dj[j].out, out_len[j], hipMemcpyDeviceToHost, s));
    }
    DLSM_TRY(ctx_sync(ctx, s));
    return st;
  }
  DLSM_CHECK(host_ensure(ctx->h_out, ctx->h_out_cap, obytes + 256));
  DLSM_CHECK(host_ensure(ctx->h_len, ctx->h_len_cap, static_cast<uint64_t>(n_jobs)));
  uint8_t* h_out_dev = host_device_view(ctx->h_out);
  uint64_t* h_len_dev = reinterpret_cast<uint64_t*>(host_device_view(ctx->h_len));
  if (!h_out_dev || !h_len_dev) return DLSM_E_DEVICE;
  for (int j = 0; j < n_jobs; j++) dj[j].out = direct[j] ? direct[j] : h_out_dev + opos[j];
  DLSM_CHECK(full_build_dev_impl(ctx, dj.data(), n_jobs, bits_per_key, h_len_dev, hashed));
  DLSM_TRY(ctx_sync(ctx, s));
  int st = DLSM_OK;
  for (int j = 0; j < n_jobs; j++) {
    out_len[j] = ctx->h_len[j];
    if (out_len[j] == 0) {
      st = DLSM_E_CAPACITY;
      continue;
    }
    if (!direct[j]) memcpy(jobs[j].out, ctx->h_out + opos[j], out_len[j]);
  }
  return st;
}
}  // namespace

int dlsm_bloom_full_build(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs, int bits_per_key,
                          uint64_t* out_len) {
  return full_build_host_impl(ctx, jobs, n_jobs, bits_per_key, out_len, false);
}

int dlsm_bloom_full_build_hashed(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs, int bits_per_key,
                                 uint64_t* out_len) {
  return full_build_host_impl(ctx, jobs, n_jobs, bits_per_key, out_len, true);
}

// ---------------------------------------------------------------------------
// Filter blocks (build + crc32c trailer) and crc32c of device buffers
// ---------------------------------------------------------------------------
namespace {
struct Crc32cTable {
  uint32_t t[256];
  Crc32cTable() {
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0x82f63b78u : (c >> 1);
      t[i] = c;
    }
  }
};
}  // namespace

uint32_t dlsm_crc32c_extend(uint32_t init_crc, const void* data, size_t n) {
  // function-local static: C++11 thread-safe initialisation (TableBuilders
  // seal blocks from several threads)
  static const Crc32cTable table;
  const uint8_t* p = static_cast<const uint8_t*>(data);
  uint32_t c = ~init_crc;
  for (size_t i = 0; i < n; i++) c = table.t[(c ^ p[i]) & 0xffu] ^ (c >> 8);
  return ~c;
}

uint32_t dlsm_crc32c_mask(uint32_t crc) { return ((crc >> 15) | (crc << 17)) + 0xa282ead8u; }

namespace {
int run_crc(dlsm_ctx* ctx, const std::vector<std::vector<uint8_t>>& streams, int n, uint64_t max_total,
            uint8_t* const* seal_out_host, const uint64_t* seal_cap_host, uint64_t* seal_len_dev,
            uint32_t* crc_val_dev) {
  hipStream_t s = ctx->stream;
  const size_t ss = crc_stream_size();
  const int max_parts = static_cast<int>(std::max<uint64_t>(1, crc_max_parts(max_total)));
  DLSM_CHECK(ctx->crc_streams.ensure(ss * n));
  DLSM_CHECK(ctx->crc_partial.ensure(static_cast<size_t>(max_parts) * n));
  std::vector<uint8_t> flat(ss * n);
  for (int j = 0; j < n; j++) memcpy(flat.data() + ss * j, streams[j].data(), ss);
  DLSM_CHECK(ctx_upload(ctx, ctx->crc_streams.p, flat.data(), ss * n, s));
  uint8_t* const* seal_out = nullptr;
  const uint64_t* seal_cap = nullptr;
  if (seal_out_host) {
    DLSM_CHECK(ctx->crc_outp.ensure(n));
    DLSM_CHECK(ctx->crc_cap.ensure(n));
    DLSM_CHECK(ctx_upload(ctx, ctx->crc_outp.p, seal_out_host, sizeof(uint8_t*) * n, s));
    DLSM_CHECK(ctx_upload(ctx, ctx->crc_cap.p, seal_cap_host, sizeof(uint64_t) * n, s));
    seal_out = ctx->crc_outp.p;
    seal_cap = ctx->crc_cap.p;
  }
  DLSM_TRY(launch_crc_streams(ctx->crc_streams.p, n, max_parts, ctx->crc_partial.p, seal_out, seal_cap,
                              seal_len_dev, crc_val_dev, s));
  return DLSM_OK;
}
}  // namespace

static int build_block_dev_impl(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs, int bits_per_key,
                                uint64_t* out_len_dev, bool hashed) {
  if (!ctx || n_jobs < 0 || (n_jobs > 0 && (!jobs || !out_len_dev))) return DLSM_E_ARG;
  if (n_jobs == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  // The filter must leave room for the 5-byte trailer.
  std::vector<dlsm_build_job> fj(jobs, jobs + n_jobs);
  std::vector<uint8_t*> outs(n_jobs);
  std::vector<uint64_t> caps(n_jobs);
  uint64_t max_total = 0;
  for (int j = 0; j < n_jobs; j++) {
    fj[j].out_cap = jobs[j].out_cap >= 5 ? jobs[j].out_cap - 5 : 0;
    outs[j] = jobs[j].out;
    caps[j] = jobs[j].out_cap;
    max_total = std::max(max_total, full_filter_len(jobs[j].keys.n, bits_per_key) + 1);
  }
  // the sliced build seals its own filters (the crc fused into its slice
  // pass); the direct path takes the separate crc passes below
  bool sealed = false;
  DLSM_CHECK(full_build_dev_impl(ctx, fj.data(), n_jobs, bits_per_key, out_len_dev, hashed, true, &sealed));
  if (sealed) return DLSM_OK;
  std::vector<std::vector<uint8_t>> st(n_jobs, std::vector<uint8_t>(crc_stream_size()));
  for (int j = 0; j < n_jobs; j++) crc_stream_fill(st[j].data(), jobs[j].out, out_len_dev + j, 0, 1);
  return run_crc(ctx, st, n_jobs, max_total, outs.data(), caps.data(), out_len_dev, nullptr);
}

int dlsm_bloom_full_build_block_dev(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs,
                                    int bits_per_key, uint64_t* out_len_dev) {
  return build_block_dev_impl(ctx, jobs, n_jobs, bits_per_key, out_len_dev, false);
}

int dlsm_bloom_full_build_block_hashed_dev(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs,
                                           int bits_per_key, uint64_t* out_len_dev) {
  return build_block_dev_impl(ctx, jobs, n_jobs, bits_per_key, out_len_dev, true);
}

static int build_block_host_impl(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs, int bits_per_key,
                                 uint64_t* out_len, bool hashed) {
  if (!ctx || n_jobs < 0 || (n_jobs > 0 && (!jobs || !out_len))) return DLSM_E_ARG;
  if (n_jobs == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  std::vector<const dlsm_keyset*> sets(n_jobs);
  for (int j = 0; j < n_jobs; j++) {
    DLSM_CHECK(validate_keyset(jobs[j].keys));
    if (!jobs[j].out) return DLSM_E_ARG;
    sets[j] = &jobs[j].keys;
  }
  std::vector<dlsm_keyset> dk;
  DLSM_CHECK(stage_keys(ctx, sets.data(), n_jobs, dk));
  std::vector<dlsm_build_job> dj(n_jobs);
  std::vector<uint64_t> opos(n_jobs);
  uint64_t obytes = 0;
  for (int j = 0; j < n_jobs; j++) {
    const uint64_t spec = full_filter_len(jobs[j].keys.n, bits_per_key) + 5;
    const uint64_t cap = std::min(spec, jobs[j].out_cap);
    opos[j] = obytes;
    obytes += (cap + 255) & ~uint64_t(255);
    dj[j].keys = dk[j];
    dj[j].out_cap = cap;
  }
  DLSM_CHECK(ctx->st_out.ensure(obytes + 256));
  DLSM_CHECK(ctx->st_len.ensure(n_jobs));
  for (int j = 0; j < n_jobs; j++) dj[j].out = ctx->st_out.p + opos[j];
  DLSM_CHECK(build_block_dev_impl(ctx, dj.data(), n_jobs, bits_per_key, ctx->st_len.p, hashed));
  hipStream_t s = ctx->stream;
  DLSM_TRY(hipMemcpyAsync(out_len, ctx->st_len.p, sizeof(uint64_t) * n_jobs, hipMemcpyDeviceToHost, s));
  DLSM_TRY(ctx_sync(ctx, s));
  int st = DLSM_OK;
  for (int j = 0; j < n_jobs; j++) {
    if (out_len[j] == 0) {
      st = DLSM_E_CAPACITY;
      continue;
    }
    DLSM_TRY(hipMemcpyAsync(jobs[j].out, dj[j].out, out_len[j], hipMemcpyDeviceToHost, s));
  }
  DLSM_TRY(ctx_sync(ctx, s));
  return st;
}

int dlsm_bloom_full_build_block(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs,
                                int bits_per_key, uint64_t* out_len) {
  return build_block_host_impl(ctx, jobs, n_jobs, bits_per_key, out_len, false);
}

int dlsm_bloom_full_build_block_hashed(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs,
                                       int bits_per_key, uint64_t* out_len) {
  return build_block_host_impl(ctx, jobs, n_jobs, bits_per_key, out_len, true);
}

int dlsm_crc32c_dev(dlsm_ctx* ctx, const uint8_t* const* bufs, const uint64_t* lens, int n,
                    uint32_t* crc_out) {
  if (!ctx || n < 0 || (n > 0 && (!bufs || !lens || !crc_out))) return DLSM_E_ARG;
  if (n == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  std::vector<std::vector<uint8_t>> st(n, std::vector<uint8_t>(crc_stream_size()));
  uint64_t max_total = 0;
  for (int j = 0; j < n; j++) {
    if (lens[j] && !bufs[j]) return DLSM_E_ARG;
    crc_stream_fill(st[j].data(), bufs[j], nullptr, lens[j], 0);
    max_total = std::max(max_total, lens[j]);
  }
  DLSM_CHECK(ctx->crc_val.ensure(n));
  DLSM_CHECK(run_crc(ctx, st, n, max_total, nullptr, nullptr, nullptr, ctx->crc_val.p));
  DLSM_TRY(hipMemcpyAsync(crc_out, ctx->crc_val.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
  DLSM_TRY(ctx_sync(ctx, ctx->stream));
  return DLSM_OK;
}

// ---------------------------------------------------------------------------
// Sealed blocks, read side: ReadFilterBlock (table/format.cc:380-444) for n
// blocks in two launches (block_ingest.hip)
// ---------------------------------------------------------------------------
static_assert(DLSM_BLOCK_OK == DLSM_INGEST_OK && DLSM_BLOCK_SHORT == DLSM_INGEST_SHORT &&
                  DLSM_BLOCK_CHECKSUM == DLSM_INGEST_CHECKSUM && DLSM_BLOCK_TYPE == DLSM_INGEST_TYPE &&
                  DLSM_BLOCK_FILTER == DLSM_INGEST_FILTER,
              "block outcomes");
namespace {
// Verify (and copy, where dst differs from src) the device-resident blocks
// `blk`; recs gets one record per block.  One upload of the work list, two
// launches, one D2H, one synchronisation.
int queue_ingest(dlsm_ctx* ctx, const std::vector<IngestBlock>& blk, bool verify, bool parse,
                 std::vector<IngestRecord>& recs);
int run_ingest(dlsm_ctx* ctx, const std::vector<IngestBlock>& blk, bool verify, bool parse,
               std::vector<IngestRecord>& recs) {
  DLSM_CHECK(queue_ingest(ctx, blk, verify, parse, recs));
  if (!blk.empty()) DLSM_TRY(ctx_sync(ctx, ctx->stream));
  return DLSM_OK;
}

// run_ingest without its synchronisation: the caller queues more work behind
// the pass (ctx->ing_rec.p holds the records on the device) and syncs once;
// recs is filled by then.
int queue_ingest(dlsm_ctx* ctx, const std::vector<IngestBlock>& blk, bool verify, bool parse,
                 std::vector<IngestRecord>& recs) {
  const size_t n = blk.size();
  recs.assign(n, IngestRecord{});
  if (n == 0) return DLSM_OK;
  if (n > 0x7fffffffull) return DLSM_E_ARG;
  hipStream_t s = ctx->stream;
  std::vector<uint32_t> part0(n + 1);
  uint64_t parts = 0, rd = 0, wr = 0;
  for (size_t j = 0; j < n; j++) {
    part0[j] = static_cast<uint32_t>(parts);
    parts += ingest_block_parts(blk[j].len);
    if (parts > 0x7fffffffull) return DLSM_E_ARG;
    if (blk[j].len >= 5) {
      const bool store = blk[j].dst && blk[j].dst != blk[j].src;
      if (store || verify) rd += blk[j].len;
      if (store) wr += blk[j].len - 5;
    }
  }
  part0[n] = static_cast<uint32_t>(parts);
  DLSM_CHECK(ctx->ing_blocks.ensure(n));
  DLSM_CHECK(ctx->ing_part0.ensure(n + 1));
  DLSM_CHECK(ctx->ing_partial.ensure(parts));
  DLSM_CHECK(ctx->ing_rec.ensure(n));
  if (!ctx->ev_ing0) DLSM_TRY(hipEventCreate(&ctx->ev_ing0));
  if (!ctx->ev_ing1) DLSM_TRY(hipEventCreate(&ctx->ev_ing1));
  DLSM_CHECK(ctx_upload(ctx, ctx->ing_blocks.p, blk.data(), sizeof(IngestBlock) * n, s));
  DLSM_CHECK(ctx_upload(ctx, ctx->ing_part0.p, part0.data(), sizeof(uint32_t) * (n + 1), s));
  DLSM_TRY(hipEventRecord(ctx->ev_ing0, s));
  DLSM_TRY(launch_block_ingest(ctx->ing_blocks.p, ctx->ing_part0.p, static_cast<uint32_t>(n),
                               static_cast<uint32_t>(parts), verify, parse, ctx->ing_partial.p, ctx->ing_rec.p, s));
  DLSM_TRY(hipEventRecord(ctx->ev_ing1, s));
  DLSM_TRY(hipMemcpyAsync(recs.data(), ctx->ing_rec.p, sizeof(IngestRecord) * n, hipMemcpyDeviceToHost, s));
  ctx->ing_read = rd;
  ctx->ing_written = wr;
  return DLSM_OK;
}

// status[j] (when given) for every record; DLSM_E_CORRUPT if any is not OK.
int ingest_status(const std::vector<IngestRecord>& recs, const std::vector<int>& where, uint8_t* status) {
  int st = DLSM_OK;
  for (size_t j = 0; j < recs.size(); j++) {
    if (status) status[where.empty() ? j : static_cast<size_t>(where[j])] = static_cast<uint8_t>(recs[j].status);
    if (recs[j].status != DLSM_BLOCK_OK) st = DLSM_E_CORRUPT;
  }
  return st;
}
}  // namespace

int dlsm_blocks_check(dlsm_ctx* ctx, const uint8_t* const* blocks, const uint64_t* lens, int n,
                      int blocks_are_device, int verify_checksums, uint8_t* status) {
  if (!ctx || n < 0 || (n > 0 && (!blocks || !lens || !status))) return DLSM_E_ARG;
  if (n == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  std::vector<IngestBlock> blk(n);
  uint64_t bytes = 0;
  for (int j = 0; j < n; j++) {
    if (lens[j] && !blocks[j]) return DLSM_E_ARG;
    blk[j] = IngestBlock{blocks[j], nullptr, lens[j]};
    bytes += (lens[j] + 255) & ~uint64_t(255);
  }
  if (!blocks_are_device) {
    DLSM_CHECK(ctx->st_filter.ensure(bytes + 256));
    uint64_t off = 0;
    for (int j = 0; j < n; j++) {
      blk[j].src = ctx->st_filter.p + off;
      if (lens[j]) DLSM_TRY(hipMemcpyAsync(ctx->st_filter.p + off, blocks[j], lens[j], hipMemcpyHostToDevice, s));
      off += (lens[j] + 255) & ~uint64_t(255);
    }
  }
  std::vector<IngestRecord> recs;
  DLSM_CHECK(run_ingest(ctx, blk, verify_checksums != 0, false, recs));
  return ingest_status(recs, {}, status);
}

int dlsm_block_open_stats(const dlsm_ctx* ctx, uint64_t* bytes_read, uint64_t* bytes_written, double* kernel_ms) {
  if (!ctx) return DLSM_E_ARG;
  if (bytes_read) *bytes_read = ctx->ing_read;
  if (bytes_written) *bytes_written = ctx->ing_written;
  if (kernel_ms) {
    *kernel_ms = 0;
    if (ctx->ev_ing0 && ctx->ev_ing1) {
      float ms = 0;
      DLSM_TRY(hipEventElapsedTime(&ms, ctx->ev_ing0, ctx->ev_ing1));
      *kernel_ms = ms;
    }
  }
  return DLSM_OK;
}

// ---------------------------------------------------------------------------
// Internal keys: flush / compaction selection and user-key gather
// ---------------------------------------------------------------------------
int dlsm_internal_keys_select_dev(dlsm_ctx* ctx, const dlsm_keyset* ikeys, int policy,
                                  uint64_t smallest_snapshot, uint8_t* keep_dev, uint64_t* n_kept,
                                  uint64_t* kept_bytes, uint64_t* first_corrupt) {
  if (!ctx || !ikeys || (policy != DLSM_SELECT_FLUSH && policy != DLSM_SELECT_COMPACTION))
    return DLSM_E_ARG;
  dlsm_keyset k = *ikeys;
  k.suffix_len = 0;
  DLSM_CHECK(validate_keyset(k));
  if (ikeys->n > 0 && !keep_dev) return DLSM_E_ARG;
  uint64_t res[4] = {0, 0, ~uint64_t(0), 0};  // n_kept, kept_bytes, first_bad
  if (k.n > 0) {
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    const uint64_t nb = select_blocks(k.n);
    DLSM_CHECK(ctx->sel.ensure(2 * nb + 3));
    uint64_t* bc = ctx->sel.p;
    uint64_t* bb = bc + nb;
    uint64_t* tot = bb + nb;
    uint64_t* bad = tot + 2;
    DLSM_TRY(hipMemsetAsync(bad, 0xff, sizeof(uint64_t), s));
    DLSM_TRY(launch_key_select(to_desc(k), policy, smallest_snapshot, keep_dev, bc, bb,
                               reinterpret_cast<unsigned long long*>(bad), tot, s));
    DLSM_TRY(hipMemcpyAsync(res, tot, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DLSM_TRY(ctx_sync(ctx, s));
  }
  if (n_kept) *n_kept = res[0];
  if (kept_bytes) *kept_bytes = res[1];
  if (first_corrupt) *first_corrupt = res[2];
  if (policy == DLSM_SELECT_FLUSH && res[2] != ~uint64_t(0)) return DLSM_E_CORRUPT;
  return DLSM_OK;
}

int dlsm_user_keys_gather_dev(dlsm_ctx* ctx, const dlsm_keyset* ikeys, const uint8_t* keep_dev,
                              uint8_t* user_keys_dev, uint64_t* offsets_dev) {
  if (!ctx || !ikeys) return DLSM_E_ARG;
  dlsm_keyset k = *ikeys;
  k.suffix_len = 0;
  DLSM_CHECK(validate_keyset(k));
  if (k.offsets && !offsets_dev) return DLSM_E_ARG;
  if (!k.offsets && k.key_len < DLSM_INTERNAL_KEY_TRAILER) return DLSM_E_ARG;
  if (k.n == 0) {
    if (offsets_dev) DLSM_TRY(hipMemsetAsync(offsets_dev, 0, sizeof(uint64_t), ctx->stream));
    return DLSM_OK;
  }
  if (!keep_dev || !user_keys_dev) return DLSM_E_ARG;
  DeviceGuard g(ctx->device);
  const uint64_t nb = select_blocks(k.n);
  DLSM_CHECK(ctx->sel.ensure(2 * nb + 3));
  uint64_t* bc = ctx->sel.p;
  uint64_t* bb = bc + nb;
  DLSM_TRY(launch_key_gather(to_desc(k), keep_dev, bc, bb, user_keys_dev,
                             k.offsets ? offsets_dev : nullptr, bb + nb, ctx->stream));
  return DLSM_OK;
}

// ---------------------------------------------------------------------------
// Full filter probe
// ---------------------------------------------------------------------------
}  // extern "C"
namespace {
uint32_t device_cus_of(int dev) {
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  return static_cast<uint32_t>(n);
}

// The one-pass layout of a multi-group set (plan_mg_layout) on the device; a
// set that does not fit keeps the per-group passes (mg_n stays 0).
int mg_layout(dlsm_filterset* fs) {
  const MGLayout M = plan_mg_layout(fs->groups, device_cus_of(fs->device));
  if (!M.ok) return DLSM_OK;
  DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&fs->d_mg), sizeof(MGroupDev) * M.md.size()));
  DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&fs->d_mgplan), sizeof(uint32_t) * M.plan.size()));
  DLSM_TRY(hipMemcpy(fs->d_mg, M.md.data(), sizeof(MGroupDev) * M.md.size(), hipMemcpyHostToDevice));
  DLSM_TRY(hipMemcpy(fs->d_mgplan, M.plan.data(), sizeof(uint32_t) * M.plan.size(), hipMemcpyHostToDevice));
  fs->mg_n = static_cast<int>(M.md.size());
  fs->mg_slices = M.slices;
  fs->mg_region = M.region;
  fs->mg_abytes = M.abytes;
  fs->mg_stage_bytes = M.stage_bytes;
  fs->mg_classes = M.classes;
  return DLSM_OK;
}

// The five tail bytes of a filter of len >= 5 bytes in host or device memory.
int fetch_tail(dlsm_ctx* ctx, const uint8_t* filter, uint64_t len, bool on_device, uint8_t* tail) {
  const uint8_t* tp = filter + len - 5;
  if (on_device) {
    DLSM_TRY(hipMemcpyAsync(tail, tp, 5, hipMemcpyDeviceToHost, ctx->stream));
    DLSM_TRY(ctx_sync(ctx, ctx->stream));
  } else {
    memcpy(tail, tp, 5);
  }
  return DLSM_OK;
}
}  // namespace
extern "C" {

// How the *_create_blocks calls hand their inputs to the create code: the
// pointers are sealed blocks, verified and parsed on the device.
struct BlocksArg {
  bool verify;
  uint8_t* status;  // host u8 per block in the caller's order, or nullptr
};

// The device half of a filter-set create: fs->h holds the parsed tails (host
// filters; sealed blocks get theirs from the ingest pass here), off each
// filter's place in the blob.  The caller owns fs and `slots` (a pageable
// source of a queued copy) and destroys fs on a non-zero status while both
// are alive.
static int filterset_upload(dlsm_ctx* ctx, const uint8_t* const* filters, const uint64_t* lens,
                            int filters_are_device, const BlocksArg* ba, const std::vector<uint64_t>& off,
                            bool packed, std::vector<FilterDev>& slots, dlsm_filterset* fs) {
  hipStream_t s = ctx->stream;
  const int n_filters = fs->F;
  std::vector<FilterDev>& h = fs->h;
  DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&fs->blob), fs->blob_bytes));
  DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&fs->d_filters), sizeof(FilterDev) * n_filters));
  if (ba) {
    // host blocks: one copy to the slot, then the pass runs in place
    std::vector<IngestBlock> blk(n_filters);
    for (int f = 0; f < n_filters; f++) {
      blk[f] = IngestBlock{filters[f], fs->blob + off[f], lens[f]};
      if (filters_are_device) continue;
      blk[f].src = blk[f].dst;
      if (lens[f]) DLSM_TRY(hipMemcpyAsync(blk[f].dst, filters[f], lens[f], hipMemcpyHostToDevice, s));
    }
    std::vector<IngestRecord> recs;
    DLSM_CHECK(run_ingest(ctx, blk, ba->verify, true, recs));
    DLSM_CHECK(ingest_status(recs, {}, ba->status));
    for (int f = 0; f < n_filters; f++)
      h[f] = FilterDev{fs->blob + off[f], recs[f].L, recs[f].magic, recs[f].k, recs[f].lg};
  }
  for (int f = 0; f < n_filters && !ba; f++) {
    DLSM_TRY(hipMemcpyAsync(fs->blob + off[f], filters[f], lens[f],
                            filters_are_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    h[f].data = fs->blob + off[f];
  }
  DLSM_TRY(hipMemcpyAsync(fs->d_filters, h.data(), sizeof(FilterDev) * n_filters, hipMemcpyHostToDevice, s));
  const FilterGroupPlan gp = plan_filter_groups(h, packed);
  fs->groups = gp.groups;
  const size_t G = fs->groups.size();
  if (G) {
    slots.assign(8 * G, FilterDev{nullptr, 0, 0, 0, 0});
    for (size_t g = 0; g < G; g++)
      for (int f : gp.members[g]) slots[8 * g + (f % 8)] = h[f];
    DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&fs->d_slots), sizeof(FilterDev) * slots.size()));
    DLSM_TRY(hipMemcpyAsync(fs->d_slots, slots.data(), sizeof(FilterDev) * slots.size(), hipMemcpyHostToDevice, s));
    for (size_t g = 0; g < G; g++) {
      ProbeGroup& grp = fs->groups[g];
      const uint64_t bytes = static_cast<uint64_t>(grp.L) * (64u << grp.lgw);
      DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&grp.stacked), bytes));
      DLSM_TRY(grp.lgw == 3 ? launch_stack_filters(fs->d_slots + 8 * g, grp.L, grp.stacked, s)
                            : launch_pack_filters(fs->d_slots + 8 * g, grp.slotmap, grp.lgw, grp.L, grp.stacked, s));
      fs->stacked_bytes += bytes;
    }
  }
  if (G >= 2 && G <= static_cast<size_t>(kMGMaxGroups)) DLSM_CHECK(mg_layout(fs));
  DLSM_TRY(hipStreamSynchronize(s));  // `slots` and fs->h are pageable host memory
  return DLSM_OK;
}

static int filterset_create_impl(dlsm_ctx* ctx, const uint8_t* const* filters, const uint64_t* lens,
                                 int n_filters, int filters_are_device, const BlocksArg* ba,
                                 dlsm_filterset** out) {
  if (!ctx || !out || !filters || !lens || n_filters < 1 || n_filters > 64) return DLSM_E_ARG;
  *out = nullptr;
  DeviceGuard g(ctx->device);
  // Metadata (k, num_lines) from each filter's 5-byte tail.
  std::vector<FilterDev> h(n_filters);
  std::vector<uint64_t> off(n_filters);
  uint64_t blob = 0;
  for (int f = 0; f < n_filters; f++) {
    if (ba) {
      // sealed blocks: the device pass reads the tails; a slot holds the
      // whole block (host blocks are verified in place)
      if (lens[f] && !filters[f]) return DLSM_E_ARG;
    } else {
      if (!filters[f] || lens[f] < 5) return DLSM_E_CORRUPT;
      uint8_t tail[5];
      DLSM_CHECK(fetch_tail(ctx, filters[f], lens[f], filters_are_device, tail));
      int k, lg;
      uint32_t L;
      DLSM_CHECK(parse_tail(tail, lens[f], &k, &L, &lg));
      h[f] = FilterDev{nullptr, L, fastmod_magic(L), k, lg};
    }
    off[f] = blob;
    blob += (lens[f] + 255) & ~uint64_t(255);
  }
  const char* pk = getenv("DLSM_PROBE_PACKED");  // A/B knob: 0 = byte-wide images only
  dlsm_filterset* fs = new (std::nothrow) dlsm_filterset();
  if (!fs) return DLSM_E_NOMEM;
  fs->device = ctx->device;
  fs->F = n_filters;
  fs->blob_bytes = blob;
  fs->h = h;
  std::vector<FilterDev> slots;
  const int st = filterset_upload(ctx, filters, lens, filters_are_device, ba, off, !(pk && atoi(pk) == 0), slots, fs);
  if (st != DLSM_OK) {
    dlsm_filterset_destroy(fs);
    return st;
  }
  *out = fs;
  return DLSM_OK;
}

int dlsm_filterset_create(dlsm_ctx* ctx, const uint8_t* const* filters, const uint64_t* lens,
                          int n_filters, int filters_are_device, dlsm_filterset** out) {
  return filterset_create_impl(ctx, filters, lens, n_filters, filters_are_device, nullptr, out);
}

int dlsm_filterset_create_blocks(dlsm_ctx* ctx, const uint8_t* const* blocks, const uint64_t* lens,
                                 int n_filters, int blocks_are_device, int verify_checksums, uint8_t* status,
                                 dlsm_filterset** out) {
  const BlocksArg ba{verify_checksums != 0, status};
  return filterset_create_impl(ctx, blocks, lens, n_filters, blocks_are_device, &ba, out);
}

int dlsm_filterset_destroy(dlsm_filterset* fs) {
  if (!fs) return DLSM_OK;
  DeviceGuard g(fs->device);
  for (auto& grp : fs->groups)
    if (grp.stacked) (void)hipFree(grp.stacked);
  if (fs->d_mg) (void)hipFree(fs->d_mg);
  if (fs->d_mgplan) (void)hipFree(fs->d_mgplan);
  if (fs->d_slots) (void)hipFree(fs->d_slots);
  if (fs->d_filters) (void)hipFree(fs->d_filters);
  if (fs->blob) (void)hipFree(fs->blob);
  delete fs;
  return DLSM_OK;
}

int dlsm_filterset_size(const dlsm_filterset* fs, int* n_filters, uint64_t* device_bytes) {
  if (!fs) return DLSM_E_ARG;
  if (n_filters) *n_filters = fs->F;
  if (device_bytes) *device_bytes = fs->blob_bytes + fs->stacked_bytes;
  return DLSM_OK;
}

namespace {

// A filter set of several groups (filters of different sizes, more than 8
// filters): every lookup is hashed ONCE (hash pass, 4 B per key), then each
// group partitions the hashes by its own line count and probes its stacked
// image, OR-ing its answer bits into the group's mask byte.  A group too large
// to slice is probed directly from the same hashes.
int probe_grouped(dlsm_ctx* ctx, const dlsm_filterset* fs, const KeyDesc& kd, int mode, uint8_t* mask_dev) {
  hipStream_t s = ctx->stream;
  const uint64_t n = kd.n;
  const int lgC = ctx->probe_lgc;
  const uint64_t C = 1ull << lgC;
  const int mb = (fs->F + 7) / 8;
  const uint32_t nC = ceil_div_u32(n, C);
  KeyDesc hk = kd;  // hashed lookups (KM_HASH) are probed as given
  if (mode != KM_HASH) {
    DLSM_CHECK(ctx->hashes.ensure(n));
    DLSM_TRY(launch_probe_hash(kd, ctx->hashes.p, mode, s));
    hk.bytes = reinterpret_cast<const uint8_t*>(ctx->hashes.p);
    hk.offsets = nullptr;
    hk.n = n;
    hk.key_len = 4;
    hk.suffix = 0;
  }
  uint32_t Smax = 0;
  for (const auto& g : fs->groups) {
    int lg;
    uint32_t R;
    Smax = std::max(Smax, group_slices(ctx->probe_lgr, g.L, g.lgw, &lg, &R));
  }
  const uint64_t rstride = static_cast<uint64_t>(nC) * probe_region(static_cast<uint32_t>(C));
  DLSM_CHECK(ctx->entries.ensure(rstride));
  DLSM_CHECK(ctx->pos.ensure(static_cast<uint64_t>(nC) * C));
  DLSM_CHECK(ctx->smask.ensure(rstride));
  DLSM_CHECK(ctx->tab.ensure(static_cast<uint64_t>(Smax + 1) * nC));
  for (size_t gi = 0; gi < fs->groups.size(); gi++) {
    const ProbeGroup& g = fs->groups[gi];
    int lgR;
    uint32_t R;
    const uint32_t S = group_slices(ctx->probe_lgr, g.L, g.lgw, &lgR, &R);
    if (S == 0 || ctx->path == 1) {
      DLSM_TRY(launch_probe_direct_group(fs->d_slots + 8 * gi, hk, mask_dev, mb, g.mask_byte,
                                         g.first_of_byte, s));
      continue;
    }
    DLSM_TRY(launch_probe_partition(hk, g.L, g.magic, R, S, ctx->entries.p, ctx->pos.p, ctx->tab.p,
                                    KM_HASH, lgC, s));
    DLSM_TRY(launch_probe_slices(g.stacked, g.L, g.magic, g.k, lgR, R, g.lgw, g.slotmap, S, nC, ctx->entries.p,
                                 ctx->tab.p, ctx->smask.p, slice_parts(S, nC, lgR), lgC, s));
    DLSM_TRY(launch_probe_unpermute_group(n, ctx->pos.p, ctx->smask.p, mask_dev, mb, g.mask_byte,
                                          g.first_of_byte, lgC, s));
  }
  return DLSM_OK;
}

// A multi-group set in ONE pass (dlsm_filterset::d_mg): one partition that
// reads and hashes each lookup once and buckets it by every group's slice, one
// slice launch per image-width class over all of the class's slices, one
// unpermute that assembles every mask byte.  Per lookup: 20 B key in, G x
// (4 B entry + 2 B position) out; G x 4 B in, G x W/8 B out (W: the group's
// image field, 1..8 bits); G x (2 B + W/8 B) in, the mask bytes out --
// against the per-group passes' hash pass plus G x (4 B hash in + 6 B out,
// 5 B, 3 B + a mask read-modify-write).
int probe_multi(dlsm_ctx* ctx, const dlsm_filterset* fs, const KeyDesc& kd, int mode, uint8_t* mask_dev) {
  hipStream_t s = ctx->stream;
  const uint64_t n = kd.n;
  const int G = fs->mg_n;
  constexpr int lgC = kMGChunkLg;
  constexpr uint64_t C = kMGChunk;
  const uint32_t rowlen = fs->mg_slices + static_cast<uint32_t>(G);
  const uint64_t mbytes = (fs->F + 7) / 8;
  // Rounds of probe_round keys (DLSM_OPT_PROBE_ROUND_KEYS), pipelined over
  // two streams as in the one-group path: round r's partition (HBM-bound, on
  // the helper stream) beside round r-1's slice pass (LDS-bound) and
  // unpermute, over kProbeBufs rotating buffer sets.
  const ProbeRounds pr = probe_rounds(n, ctx->probe_round, ctx->probe_serial, C);
  const uint64_t round = pr.round, n_rounds = pr.n_rounds, nCmax = pr.nCmax;
  const bool pipe = pr.pipe;
  const int nbuf = pr.nbuf;
  const uint64_t estride = nCmax * fs->mg_region, astride = nCmax * fs->mg_abytes;
  const uint64_t pstride = nCmax * G * C, tstride = nCmax * rowlen;
  DLSM_CHECK(ctx->entries.ensure(estride * nbuf));
  DLSM_CHECK(ctx->smask.ensure(astride * nbuf));
  DLSM_CHECK(ctx->pos.ensure(pstride * nbuf));
  DLSM_CHECK(ctx->tab.ensure(tstride * nbuf));
  if (pipe) DLSM_CHECK(fork_aux(ctx));
  hipStream_t ps = pipe ? ctx->aux : s;
  for (uint64_t r = 0; r < n_rounds; r++) {
    const uint64_t r0 = r * round;
    const uint64_t nr = std::min(round, n - r0);
    const uint64_t nC = (nr + C - 1) >> lgC;
    const int b = static_cast<int>(r % nbuf);
    uint32_t* ent = ctx->entries.p + b * estride;
    uint8_t* ans = ctx->smask.p + b * astride;
    uint16_t* pos = ctx->pos.p + b * pstride;
    uint16_t* tab = ctx->tab.p + b * tstride;
    const KeyDesc kr = round_keys(kd, r0, nr);
    if (pipe && r >= static_cast<uint64_t>(nbuf)) DLSM_TRY(hipStreamWaitEvent(ps, ctx->ev_free[b], 0));
    DLSM_TRY(launch_probe_mpartition(kr, fs->d_mg, G, rowlen, fs->mg_region, fs->mg_stage_bytes, ent, pos, tab,
                                     mode, ps));
    if (pipe) DLSM_CHECK(hand_over(ps, s, ctx->ev_part[b]));
    for (const MGClass& cl : fs->mg_classes)
      DLSM_TRY(launch_probe_mslices(cl.lgw, cl.K, fs->d_mg, G, cl.s0, cl.S, rowlen, fs->mg_region, fs->mg_abytes,
                                    static_cast<uint32_t>(nC), ent, tab, ans, fs->d_mgplan + cl.plan_off, cl.wgs, s));
    DLSM_TRY(launch_probe_munpermute(nr, fs->d_mg, G, fs->mg_abytes, pos, ans, mask_dev + r0 * mbytes, mbytes, s));
    if (pipe) DLSM_TRY(hipEventRecord(ctx->ev_free[b], s));
  }
  return DLSM_OK;
}

}  // namespace

namespace {
// hashed: the keys are BloomHash values (u32 each, key_len 4), as the host
// computes them in KeyMayMatch (full_filter_block.cc:271).
int full_probe_dev_impl(dlsm_ctx* ctx, const dlsm_filterset* fs, const dlsm_keyset* keys, uint8_t* mask_dev,
                        bool hashed) {
  if (!ctx || !fs || !keys) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  if (fs->device != ctx->device) return DLSM_E_ARG;
  DLSM_CHECK(validate_keyset(*keys));
  if (hashed && !is_hash_set(*keys)) return DLSM_E_ARG;
  if (keys->n == 0) return DLSM_OK;
  if (!mask_dev) return DLSM_E_ARG;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const int mode = hashed ? KM_HASH : is_k20(*keys) ? KM_K20 : (is_k28(*keys) ? KM_K28 : KM_GENERIC);
  const KeyDesc kd = to_desc(*keys);
  const int lgC = ctx->probe_lgc;
  const uint64_t C = 1ull << lgC;
  const bool fits = keys->n <= 0xffffffffull * C;
  // The set's sliceable groups (all of them must be, for the forced sliced path).
  bool all_sliceable = !fs->groups.empty();
  for (const auto& grp : fs->groups) {
    int lg;
    uint32_t R;
    all_sliceable = all_sliceable && group_slices(ctx->probe_lgr, grp.L, grp.lgw, &lg, &R) != 0;
  }
  if (ctx->path == 2 && !(all_sliceable && fits)) return DLSM_E_ARG;
  if (fs->groups.empty() || ctx->path == 1 || !fits) {
    DLSM_TRY(launch_probe_direct(fs->d_filters, fs->F, kd, mask_dev, mode, s));
    return DLSM_OK;
  }
  if (fs->mg_n > 0 && ctx->probe_multi && fs->groups.size() > 1 && keys->n <= (0xffffffffull << kMGChunkLg))
    return probe_multi(ctx, fs, kd, mode, mask_dev);
  if (fs->groups.size() > 1 || !all_sliceable) return probe_grouped(ctx, fs, kd, mode, mask_dev);

  // One group (the bench's set: <= 8 filters of one line count): the keys are
  // hashed inside the partition pass.
  const ProbeGroup& grp = fs->groups[0];
  int lgR;
  uint32_t R;
  const uint32_t S = group_slices(ctx->probe_lgr, grp.L, grp.lgw, &lgR, &R);
  // Rounds of probe_round keys, pipelined: round r's partition (helper
  // stream) overlaps round r-1's slice + unpermute (context stream), or
  // serial (DLSM_OPT_PROBE_ROUND_SERIAL).  A round's intermediates (4 B hash +
  // 2 B position + 1 B answer per key) live in one of kProbeBufs rotating
  // buffers, small enough to stay resident in the 256 MiB Infinity Cache
  // while the keys stream past.
  const uint64_t n = keys->n;
  const ProbeRounds pr = probe_rounds(n, ctx->probe_round, ctx->probe_serial, C);
  const uint64_t round = pr.round, n_rounds = pr.n_rounds, nCmax = pr.nCmax;
  const bool pipe = pr.pipe;
  const int nbuf = pr.nbuf;
  const uint64_t kstride = static_cast<uint64_t>(nCmax) * C;  // keys per buffer (16-B aligned)
  const uint64_t rstride = static_cast<uint64_t>(nCmax) * probe_region(static_cast<uint32_t>(C));  // entries / answers
  const uint64_t tstride = static_cast<uint64_t>(S + 1) * nCmax;        // table u16 per buffer
  DLSM_CHECK(ctx->entries.ensure(rstride * nbuf));
  DLSM_CHECK(ctx->pos.ensure(kstride * nbuf));
  DLSM_CHECK(ctx->smask.ensure(rstride * nbuf));
  DLSM_CHECK(ctx->tab.ensure(tstride * nbuf));
  if (pipe) DLSM_CHECK(fork_aux(ctx));
  // dlsm_ctx_set_partition_stream (one round): the partition there, the
  // slice + unpermute passes on the context stream
  const bool split = ctx->pstream && n_rounds == 1;
  if (split) DLSM_CHECK(fork_part(ctx));
  hipStream_t ps = pipe ? ctx->aux : (split ? ctx->pstream : s);
  for (uint64_t r = 0; r < n_rounds; r++) {
    const uint64_t r0 = r * round;
    const uint64_t nr = std::min(round, n - r0);
    const uint32_t nC = ceil_div_u32(nr, C);
    const int b = static_cast<int>(r % nbuf);
    uint32_t* ent = ctx->entries.p + b * rstride;
    uint16_t* pos = ctx->pos.p + b * kstride;
    uint8_t* sm = ctx->smask.p + b * rstride;
    uint16_t* tab = ctx->tab.p + b * tstride;
    const KeyDesc kr = round_keys(kd, r0, nr);
    if (pipe && r >= static_cast<uint64_t>(nbuf)) DLSM_TRY(hipStreamWaitEvent(ps, ctx->ev_free[b], 0));
    DLSM_TRY(launch_probe_partition(kr, grp.L, grp.magic, R, S, ent, pos, tab, mode, lgC, ps,
                                    split ? ctx->pcus : 0u));
    if (pipe) DLSM_CHECK(hand_over(ps, s, ctx->ev_part[b]));
    if (split) DLSM_CHECK(join_part(ctx));
    DLSM_TRY(launch_probe_slices(grp.stacked, grp.L, grp.magic, grp.k, lgR, R, grp.lgw, grp.slotmap, S, nC, ent,
                                 tab, sm, slice_parts(S, nC, lgR), lgC, s));
    DLSM_TRY(launch_probe_unpermute(nr, pos, sm, mask_dev + r0, lgC, s));
    if (pipe) DLSM_TRY(hipEventRecord(ctx->ev_free[b], s));
  }
  return DLSM_OK;
}
}  // namespace

int dlsm_bloom_full_probe_dev(dlsm_ctx* ctx, const dlsm_filterset* fs, const dlsm_keyset* keys,
                              uint8_t* mask_dev) {
  return full_probe_dev_impl(ctx, fs, keys, mask_dev, false);
}

int dlsm_bloom_full_probe_hashed_dev(dlsm_ctx* ctx, const dlsm_filterset* fs, const dlsm_keyset* hashes,
                                     uint8_t* mask_dev) {
  return full_probe_dev_impl(ctx, fs, hashes, mask_dev, true);
}

int dlsm_bloom_full_probe(dlsm_ctx* ctx, const dlsm_filterset* fs, const dlsm_keyset* keys,
                          uint8_t* mask) {
  if (!ctx || !fs || !keys) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  DLSM_CHECK(validate_keyset(*keys));
  if (keys->n == 0) return DLSM_OK;
  if (!mask) return DLSM_E_ARG;
  DeviceGuard g(ctx->device);
  const dlsm_keyset* sets[1] = {keys};
  std::vector<dlsm_keyset> dk;
  DLSM_CHECK(stage_keys(ctx, sets, 1, dk));
  const uint64_t mb = static_cast<uint64_t>((fs->F + 7) / 8) * keys->n;
  DLSM_CHECK(ctx->st_out.ensure(mb));
  DLSM_CHECK(dlsm_bloom_full_probe_dev(ctx, fs, &dk[0], ctx->st_out.p));
  DLSM_TRY(hipMemcpyAsync(mask, ctx->st_out.p, mb, hipMemcpyDeviceToHost, ctx->stream));
  DLSM_TRY(ctx_sync(ctx, ctx->stream));
  return DLSM_OK;
}

// ---------------------------------------------------------------------------
// Legacy block-based filter block (table/filter_block.cc), §8f row 4
// ---------------------------------------------------------------------------
int dlsm_filter_block_size(const uint64_t* block_key_end, const uint64_t* block_end_offset,
                           int n_blocks, uint64_t n_keys, int bits_per_key, uint64_t* nbytes) {
  if (!nbytes) return DLSM_E_ARG;
  FilterGroups G;
  DLSM_CHECK(filter_groups(block_key_end, block_end_offset, n_blocks, n_keys, bits_per_key, G));
  *nbytes = G.total;
  return DLSM_OK;
}

int dlsm_filter_block_build_dev(dlsm_ctx* ctx, const dlsm_keyset* keys, const uint64_t* block_key_end,
                                const uint64_t* block_end_offset, int n_blocks, int bits_per_key,
                                uint8_t* out_dev, uint64_t out_cap, uint64_t* out_len) {
  if (!ctx || !keys || !out_dev) return DLSM_E_ARG;
  DLSM_CHECK(validate_keyset(*keys));
  FilterGroups G;
  DLSM_CHECK(filter_groups(block_key_end, block_end_offset, n_blocks, keys->n, bits_per_key, G));
  if (out_len) *out_len = 0;
  if (G.total > out_cap) return DLSM_E_CAPACITY;
  DeviceGuard g(ctx->device);
  // one legacy CreateFilter job per non-empty group, written in place
  std::vector<dlsm_build_job> jobs;
  for (size_t f = 0; f < G.off.size(); f++) {
    if (G.end[f] == G.begin[f]) continue;
    dlsm_build_job j{};
    j.keys = *keys;
    j.keys.n = G.end[f] - G.begin[f];
    if (keys->offsets) j.keys.offsets = keys->offsets + G.begin[f];
    else j.keys.bytes = keys->bytes + G.begin[f] * keys->key_len;
    j.out = out_dev + G.off[f];
    j.out_cap = legacy_bits(j.keys.n, bits_per_key) / 8 + 1;
    jobs.push_back(j);
  }
  if (!jobs.empty()) {
    DLSM_CHECK(ctx->st_len.ensure(jobs.size()));
    DLSM_CHECK(dlsm_bloom_legacy_build_dev(ctx, jobs.data(), static_cast<int>(jobs.size()), bits_per_key,
                                           ctx->st_len.p));
  }
  // Finish: Fixed32 filter offsets, Fixed32 array offset, kFilterBaseLg
  std::vector<uint8_t> tail(G.total - G.array_offset);
  for (size_t f = 0; f < G.off.size(); f++) memcpy(&tail[4 * f], &G.off[f], 4);  // little-endian
  const uint32_t ao = static_cast<uint32_t>(G.array_offset);
  memcpy(&tail[4 * G.off.size()], &ao, 4);
  tail.back() = static_cast<uint8_t>(kFilterBaseLg);
  DLSM_TRY(hipMemcpyAsync(out_dev + G.array_offset, tail.data(), tail.size(), hipMemcpyHostToDevice,
                          ctx->stream));
  DLSM_TRY(ctx_sync(ctx, ctx->stream));  // `tail` is pageable host memory
  if (out_len) *out_len = G.total;
  return DLSM_OK;
}

int dlsm_filter_block_probe_dev(dlsm_ctx* ctx, const uint8_t* block_dev, uint64_t len,
                                const dlsm_keyset* keys, const uint64_t* block_offsets_dev,
                                uint8_t* out_dev) {
  if (!ctx || !keys) return DLSM_E_ARG;
  DLSM_CHECK(validate_keyset(*keys));
  if (keys->n == 0) return DLSM_OK;
  if (!out_dev || !block_offsets_dev || (len && !block_dev)) return DLSM_E_ARG;
  DeviceGuard g(ctx->device);
  DLSM_TRY(launch_filter_block_probe(block_dev, len, to_desc(*keys), block_offsets_dev, out_dev, ctx->stream));
  return DLSM_OK;
}

int dlsm_filter_block_build(dlsm_ctx* ctx, const dlsm_keyset* keys, const uint64_t* block_key_end,
                            const uint64_t* block_end_offset, int n_blocks, int bits_per_key,
                            uint8_t* out, uint64_t out_cap, uint64_t* out_len) {
  if (!ctx || !keys || !out) return DLSM_E_ARG;
  DLSM_CHECK(validate_keyset(*keys));
  uint64_t need = 0;
  DLSM_CHECK(dlsm_filter_block_size(block_key_end, block_end_offset, n_blocks, keys->n, bits_per_key, &need));
  if (out_len) *out_len = 0;
  if (need > out_cap) return DLSM_E_CAPACITY;
  DeviceGuard g(ctx->device);
  const dlsm_keyset* sets[1] = {keys};
  std::vector<dlsm_keyset> dk;
  DLSM_CHECK(stage_keys(ctx, sets, 1, dk));
  DLSM_CHECK(ctx->st_out.ensure(need));
  uint64_t len = 0;
  DLSM_CHECK(dlsm_filter_block_build_dev(ctx, &dk[0], block_key_end, block_end_offset, n_blocks,
                                         bits_per_key, ctx->st_out.p, need, &len));
  DLSM_TRY(hipMemcpyAsync(out, ctx->st_out.p, len, hipMemcpyDeviceToHost, ctx->stream));
  DLSM_TRY(ctx_sync(ctx, ctx->stream));
  if (out_len) *out_len = len;
  return DLSM_OK;
}

int dlsm_filter_block_probe(dlsm_ctx* ctx, const uint8_t* block, uint64_t len, const dlsm_keyset* keys,
                            const uint64_t* block_offsets, uint8_t* out) {
  if (!ctx || !keys) return DLSM_E_ARG;
  DLSM_CHECK(validate_keyset(*keys));
  if (keys->n == 0) return DLSM_OK;
  if (!out || !block_offsets || (len && !block)) return DLSM_E_ARG;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const dlsm_keyset* sets[1] = {keys};
  std::vector<dlsm_keyset> dk;
  DLSM_CHECK(stage_keys(ctx, sets, 1, dk));
  // staging: [block | offsets | answers]
  const uint64_t bo = (len + 15) & ~uint64_t(15);
  const uint64_t oo = bo + 8 * keys->n;
  DLSM_CHECK(ctx->st_out.ensure(oo + keys->n));
  if (len) DLSM_TRY(hipMemcpyAsync(ctx->st_out.p, block, len, hipMemcpyHostToDevice, s));
  DLSM_TRY(hipMemcpyAsync(ctx->st_out.p + bo, block_offsets, 8 * keys->n, hipMemcpyHostToDevice, s));
  DLSM_CHECK(dlsm_filter_block_probe_dev(ctx, len ? ctx->st_out.p : nullptr, len, &dk[0],
                                         reinterpret_cast<const uint64_t*>(ctx->st_out.p + bo),
                                         ctx->st_out.p + oo));
  DLSM_TRY(hipMemcpyAsync(out, ctx->st_out.p + oo, keys->n, hipMemcpyDeviceToHost, s));
  DLSM_TRY(ctx_sync(ctx, s));
  return DLSM_OK;
}

// ---------------------------------------------------------------------------
// Version: files + filters for the MultiGet-style probe (§8f row 3)
// ---------------------------------------------------------------------------
static_assert(DLSM_NUM_LEVELS == kNumLevels, "config::kNumLevels");

struct dlsm_version {
  int device = 0;
  VersionDev v{};
  int n_files = 0;
  uint8_t* mem = nullptr;  // one allocation: files | key blob | filters (sliced levels: their images) | order
  std::vector<VersionLevel> sliced;
  const uint32_t* order = nullptr;  // device: search order -> the caller's file index (the read plan's output names)
};

namespace {
// A level >= 1 goes to the sliced probe when its filters hold more than this
// many bytes and every filter of the level has 64-byte lines and one probe
// count.  Default 256 MiB, the Infinity Cache: below it the direct probe's
// line reads (four lanes per line, tasks queued per wave) are served on-die
// and beat a partition / slice / unpermute round per level -- the db_bench
// version (139.5 MB of filters) takes 4.0 ms direct against 5.4 ms with its
// two big levels sliced (profiles/r05_version_probe.txt).
// ($DLSM_VERSION_SLICE_MIN_BYTES overrides; 0 disables the sliced probe.)
// The sliced version probe measured slower than the direct one at both level
// sizes tried (db_bench's 125 MB level 3: 3.76 vs 3.48 ms per 100 M Gets; a
// 1.25 GB level 3: 11.1 vs 5.0 ms; profiles/r05_p_version_large.txt), so no
// level is sliced unless a caller asks ($DLSM_VERSION_SLICE_MIN_BYTES or
// DLSM_OPT_VERSION_SLICE_BYTES: levels whose filters exceed that many bytes).
uint64_t version_slice_min_bytes() {
  static const uint64_t v = [] {
    const char* e = getenv("DLSM_VERSION_SLICE_MIN_BYTES");
    return e ? strtoull(e, nullptr, 10) : uint64_t(0);
  }();
  return v;
}
}  // namespace

// The device half of a version create: allocate, (sealed blocks: ingest,)
// copy the filters and the plan's tables.  The caller owns the plan and h
// (the plan's file table, here given its device pointers) -- pageable sources
// of queued copies -- and ver, and destroys ver on a non-zero status while
// they are alive.
static int version_upload(dlsm_ctx* ctx, const VersionPlan& P, const dlsm_version_file* files,
                          int filters_are_device, const BlocksArg* ba, std::vector<VFileDev>& h, dlsm_version* ver) {
  hipStream_t s = ctx->stream;
  const int n_files = ver->n_files;
  h = P.h;
  DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&ver->mem), std::max<uint64_t>(P.total, 256)));
  if (ba) {
    // one verify-and-ingest pass over every file's block (search order);
    // host blocks are copied to their slots first and verified in place
    std::vector<IngestBlock> blk;
    std::vector<int> where, slot;
    for (int j = 0; j < n_files; j++) {
      const dlsm_version_file& F = files[P.order[j]];
      if (ba->status) ba->status[P.order[j]] = DLSM_BLOCK_OK;
      if (!F.filter) continue;
      IngestBlock b{F.filter, ver->mem + P.foff[j], F.filter_len};
      if (!filters_are_device) {
        b.src = b.dst;
        if (F.filter_len) DLSM_TRY(hipMemcpyAsync(b.dst, F.filter, F.filter_len, hipMemcpyHostToDevice, s));
      }
      blk.push_back(b);
      where.push_back(P.order[j]);
      slot.push_back(j);
    }
    std::vector<IngestRecord> recs;
    DLSM_CHECK(run_ingest(ctx, blk, ba->verify, true, recs));
    DLSM_CHECK(ingest_status(recs, where, ba->status));
    for (size_t q = 0; q < blk.size(); q++)
      h[slot[q]].f = FilterDev{blk[q].dst, recs[q].L, recs[q].magic, recs[q].k, recs[q].lg};
  }
  for (int j = 0; j < n_files && !ba; j++) {
    const dlsm_version_file& F = files[P.order[j]];
    if (!F.filter) continue;
    h[j].f.data = ver->mem + P.foff[j];
    DLSM_TRY(hipMemcpyAsync(ver->mem + P.foff[j], F.filter, P.copy_len[j],
                            filters_are_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  }
  ver->sliced = P.sliced;
  for (size_t q = 0; q < ver->sliced.size(); q++) ver->sliced[q].image = ver->mem + P.image_off[q];
  const uint64_t pre_off = P.files_bytes, keys_off = pre_off + P.pre_bytes;
  const uint64_t bnd_off = keys_off + P.keys_bytes, ivl_off = bnd_off + P.bnd_bytes;
  if (n_files) {
    DLSM_TRY(hipMemcpyAsync(ver->mem, h.data(), sizeof(VFileDev) * n_files, hipMemcpyHostToDevice, s));
    DLSM_TRY(hipMemcpyAsync(ver->mem + pre_off, P.pre.data(), sizeof(ulonglong2) * P.pre.size(),
                            hipMemcpyHostToDevice, s));
  }
  if (!P.keys.empty())
    DLSM_TRY(hipMemcpyAsync(ver->mem + keys_off, P.keys.data(), P.keys.size(), hipMemcpyHostToDevice, s));
  if (!P.bnd.empty())
    DLSM_TRY(hipMemcpyAsync(ver->mem + bnd_off, P.bnd.data(), sizeof(ulonglong2) * P.bnd.size(),
                            hipMemcpyHostToDevice, s));
  DLSM_TRY(hipMemcpyAsync(ver->mem + ivl_off, P.ivl.data(), sizeof(VIntervalDev) * P.ivl.size(),
                          hipMemcpyHostToDevice, s));
  static_assert(sizeof(int) == sizeof(uint32_t), "VersionPlan::order uploads as u32");
  if (n_files)
    DLSM_TRY(hipMemcpyAsync(ver->mem + P.order_off, P.order.data(), sizeof(uint32_t) * n_files, hipMemcpyHostToDevice,
                            s));
  ver->order = reinterpret_cast<const uint32_t*>(ver->mem + P.order_off);
  DLSM_TRY(hipStreamSynchronize(s));  // pageable sources: finish before returning
  ver->v.files = reinterpret_cast<const VFileDev*>(ver->mem);
  ver->v.pre_small = reinterpret_cast<const ulonglong2*>(ver->mem + pre_off);
  ver->v.pre_large = ver->v.pre_small + n_files;
  ver->v.keyblob = ver->mem + keys_off;
  ver->v.bnd = reinterpret_cast<const ulonglong2*>(ver->mem + bnd_off);
  ver->v.ivl = reinterpret_cast<const VIntervalDev*>(ver->mem + ivl_off);
  ver->v.n_bnd = static_cast<uint32_t>(P.bnd.size());
  ver->v.k_all = ba ? version_k_all(files, P.order, h) : P.k_all;
  ver->v.n_l0 = static_cast<uint32_t>(P.n_l0);
  for (int lv = 0; lv < kNumLevels; lv++) {
    ver->v.lvl_begin[lv] = P.begin[lv];
    ver->v.lvl_count[lv] = P.count[lv];
    ver->v.lvl_sliced[lv] = P.lvl_sliced[lv];
  }
  return DLSM_OK;
}

static int version_create_impl(dlsm_ctx* ctx, const dlsm_version_file* files, int n_files,
                               int filters_are_device, const BlocksArg* ba, dlsm_version** out) {
  if (!ctx || !out || n_files < 0 || (n_files > 0 && !files)) return DLSM_E_ARG;
  *out = nullptr;
  DLSM_CHECK(check_version_files(files, n_files));
  DeviceGuard g(ctx->device);
  // (sealed blocks: the device pass reads the tails)
  std::vector<uint8_t> tails(5 * static_cast<size_t>(n_files));
  for (int f = 0; f < n_files && !ba; f++)
    if (files[f].filter && files[f].filter_len >= 5)
      DLSM_CHECK(fetch_tail(ctx, files[f].filter, files[f].filter_len, filters_are_device, &tails[5 * f]));
  const uint64_t min_bytes = ctx->vslice_bytes == 0 ? version_slice_min_bytes()
                             : (ctx->vslice_bytes == UINT64_MAX ? 0 : ctx->vslice_bytes);
  VersionPlan P;
  DLSM_CHECK(plan_version(files, n_files, tails.data(), !ba, min_bytes, P));
  dlsm_version* ver = new (std::nothrow) dlsm_version();
  if (!ver) return DLSM_E_NOMEM;
  ver->device = ctx->device;
  ver->n_files = n_files;
  std::vector<VFileDev> h;
  const int st = version_upload(ctx, P, files, filters_are_device, ba, h, ver);
  if (st != DLSM_OK) {
    dlsm_version_destroy(ver);
    return st;
  }
  *out = ver;
  return DLSM_OK;
}

int dlsm_version_create(dlsm_ctx* ctx, const dlsm_version_file* files, int n_files,
                        int filters_are_device, dlsm_version** out) {
  return version_create_impl(ctx, files, n_files, filters_are_device, nullptr, out);
}

int dlsm_version_create_blocks(dlsm_ctx* ctx, const dlsm_version_file* files, int n_files,
                               int blocks_are_device, int verify_checksums, uint8_t* status,
                               dlsm_version** out) {
  const BlocksArg ba{verify_checksums != 0, status};
  return version_create_impl(ctx, files, n_files, blocks_are_device, &ba, out);
}

int dlsm_version_destroy(dlsm_version* v) {
  if (!v) return DLSM_OK;
  DeviceGuard g(v->device);
  if (v->mem) (void)hipFree(v->mem);
  delete v;
  return DLSM_OK;
}

int dlsm_version_slots(const dlsm_version* v, int* n_l0, int* n_slots) {
  if (!v) return DLSM_E_ARG;
  if (n_l0) *n_l0 = static_cast<int>(v->v.n_l0);
  if (n_slots) *n_slots = static_cast<int>(v->v.n_l0) + kNumLevels - 1;
  return DLSM_OK;
}

int dlsm_version_probe_dev(dlsm_ctx* ctx, const dlsm_version* v, const dlsm_keyset* keys,
                           uint64_t snapshot, uint64_t* slot_mask_dev, uint32_t* level_file_dev) {
  if (!ctx || !v || !keys) return DLSM_E_ARG;
  if (v->device != ctx->device) return DLSM_E_ARG;
  if (snapshot > ((uint64_t(1) << 56) - 1)) return DLSM_E_ARG;  // kMaxSequenceNumber
  DLSM_CHECK(validate_keyset(*keys));
  if (keys->n == 0) return DLSM_OK;
  if (!slot_mask_dev) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const KeyDesc kd = to_desc(*keys);
  if (v->sliced.empty() || ctx->path == 1) {
    // every level probed directly: one thread per lookup, filter lines read
    // where they lie (the L2-resident shape)
    VersionDev vd = v->v;
    for (int lv = 0; lv < kNumLevels; lv++) vd.lvl_sliced[lv] = -1;
    DLSM_TRY(launch_version_probe(vd, kd, snapshot, slot_mask_dev, level_file_dev, s));
    return DLSM_OK;
  }
  // Sliced: a route pass (the direct levels answered, each sliced level's
  // global line per lookup), then per sliced level and group of up to
  // kVMaxSlices slices a partition / LDS slice / unpermute round.
  const uint64_t n = keys->n;
  const int J = static_cast<int>(v->sliced.size());
  const uint32_t nC = ceil_div_u32(n, kVChunk);
  const uint64_t span = static_cast<uint64_t>(ctx->vpass_slices) << kVSliceLg;
  struct Pass {
    int j;
    uint32_t g0, S, L;
  };
  std::vector<Pass> passes;
  uint32_t Smax = 1;
  for (int j = 0; j < J; j++)
    for (uint64_t g0 = 0; g0 < v->sliced[j].lines; g0 += span) {
      const uint32_t L = static_cast<uint32_t>(std::min<uint64_t>(v->sliced[j].lines - g0, span));
      const uint32_t S = ceil_div_u32(L, 1u << kVSliceLg);
      passes.push_back(Pass{j, static_cast<uint32_t>(g0), S, L});
      Smax = std::max(Smax, S);
    }
  uint64_t slots = 0;
  for (int j = 0; j < J; j++) slots |= static_cast<uint64_t>(v->v.n_l0 + v->sliced[j].level - 1) << (8 * j);
  DLSM_CHECK(ctx->hashes.ensure(n));
  DLSM_CHECK(ctx->vgl.ensure(static_cast<uint64_t>(J) * n));
  DLSM_CHECK(ctx->entries.ensure(static_cast<uint64_t>(nC) * kVRegion));
  DLSM_CHECK(ctx->smask.ensure(static_cast<uint64_t>(nC) * kVRegion));
  DLSM_CHECK(ctx->pos.ensure(static_cast<uint64_t>(nC) * kVChunk));
  DLSM_CHECK(ctx->tab.ensure(static_cast<uint64_t>(nC) * (Smax + 1)));
  if (passes.size() > 1) DLSM_CHECK(ctx->vabyte.ensure(n));
  DLSM_CHECK(ctx->vplan.ensure(2 * (kVMaxSlices + 1)));
  uint32_t* gcnt = ctx->vplan.p;
  uint32_t* plan = ctx->vplan.p + kVMaxSlices + 1;
  if (ctx->vplan_zeroed != ctx->vplan.gen) {  // the plan kernel re-zeroes the counters after every pass
    DLSM_TRY(hipMemsetAsync(gcnt, 0, sizeof(uint32_t) * (kVMaxSlices + 1), s));
    ctx->vplan_zeroed = ctx->vplan.gen;
  }
  DLSM_TRY(launch_version_route(v->v, kd, snapshot, slot_mask_dev, level_file_dev, ctx->hashes.p, ctx->vgl.p, s));
  for (size_t p = 0; p < passes.size(); p++) {
    const Pass& P = passes[p];
    const VersionLevel& VL = v->sliced[P.j];
    DLSM_TRY(launch_version_partition(ctx->hashes.p, ctx->vgl.p + static_cast<uint64_t>(P.j) * n, n, P.g0, P.S,
                                      ctx->entries.p, ctx->pos.p, ctx->tab.p, gcnt, plan, s));
    DLSM_TRY(launch_version_slices(VL.image + static_cast<uint64_t>(P.g0) * 64, P.L, VL.k, P.S, nC,
                                   ctx->entries.p, ctx->tab.p, ctx->smask.p, plan, s));
    DLSM_TRY(launch_version_unpermute(n, ctx->pos.p, ctx->smask.p, ctx->vabyte.p, slot_mask_dev, P.j, J, slots,
                                      p == 0, p + 1 == passes.size(), s));
  }
  return DLSM_OK;
}

uint32_t dlsm_version_read_plan_chunk(void) { return kPlanChunk; }

int dlsm_version_read_plan_dev(dlsm_ctx* ctx, const dlsm_version* v, const uint64_t* slot_mask_dev,
                               const uint32_t* level_file_dev, uint64_t n, int mode, uint64_t* file_begin_dev,
                               uint32_t* gets_dev, uint64_t cap, uint64_t* dropped_dev) {
  if (!ctx || !v || v->device != ctx->device) return DLSM_E_ARG;
  if (n > 0xffffffffull || (mode != DLSM_PLAN_FIRST && mode != DLSM_PLAN_ALL)) return DLSM_E_ARG;
  if (!file_begin_dev || (!gets_dev && cap > 0)) return DLSM_E_ARG;
  if (n > 0 && !slot_mask_dev) return DLSM_E_ARG;
  const PlanShape shape = plan_shape(v->v.n_l0, v->v.lvl_begin, v->v.lvl_count);
  bool level_files = false;
  for (int lv = 0; lv < kPlanLevels; lv++) level_files = level_files || shape.lvl_count[lv] != 0;
  if (n > 0 && !level_file_dev && level_files) return DLSM_E_ARG;
  ReadPlan R;
  DLSM_CHECK(plan_read(n, static_cast<uint64_t>(v->n_files), plan_tasks_per_get(shape), mode, R));
  if (ctx->fault) return -ctx->fault;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  if (n == 0) {
    DLSM_TRY(hipMemsetAsync(file_begin_dev, 0, sizeof(uint64_t) * (static_cast<uint64_t>(v->n_files) + 1), s));
    if (dropped_dev) DLSM_TRY(hipMemsetAsync(dropped_dev, 0, sizeof(uint64_t), s));
    return DLSM_OK;
  }
  DLSM_CHECK(ctx->plan_ws.ensure(R.bytes));
  uint8_t* ws = ctx->plan_ws.p;
  ReadPlanDev a{};
  a.shape = shape;
  a.order = v->order;
  a.mask = slot_mask_dev;
  a.pick = level_file_dev;
  a.n = n;
  a.n_files = static_cast<uint32_t>(v->n_files);
  a.all = mode == DLSM_PLAN_ALL ? 1 : 0;
  a.cnt = reinterpret_cast<uint32_t*>(ws + R.cnt_off);
  a.off = reinterpret_cast<uint64_t*>(ws + R.off_off);
  a.drop = reinterpret_cast<uint64_t*>(ws + R.drop_off);
  a.total = reinterpret_cast<uint64_t*>(ws + R.total_off);
  a.pair_items = R.pair_items;
  a.file_begin = file_begin_dev;
  a.gets = gets_dev;
  a.cap = cap;
  a.dropped = dropped_dev;
  uint32_t* keys[2];
  uint32_t* vals[2];
  for (int b = 0; b < 2; b++) {
    keys[b] = R.keys_bytes[b] ? reinterpret_cast<uint32_t*>(ws + R.keys_off[b]) : nullptr;
    vals[b] = R.vals_bytes[b] ? reinterpret_cast<uint32_t*>(ws + R.vals_off[b]) : nullptr;
  }
  for (int p = 0; p < R.passes; p++) {
    const ReadPlanPass& P = R.pass[p];
    const bool last = p + 1 == R.passes;
    // pass p writes buffer p % 2 and reads the other (pass 0: FIRST's file ids)
    uint32_t* kin = keys[(p + 1) % 2];
    const uint32_t* vin = p > 0 ? vals[(p + 1) % 2] : nullptr;
    uint32_t* kout = R.passes > 1 ? keys[p % 2] : nullptr;  // (the last of several: the bounds kernel's input)
    uint32_t* vout = last ? nullptr : vals[p % 2];
    DLSM_TRY(launch_read_plan_pass(a, p, R.passes, P.shift, P.cpw, P.nwg, kin, vin, kout, vout, s));
  }
  if (R.passes > 1) DLSM_TRY(launch_read_plan_bounds(a, keys[(R.passes - 1) % 2], s));
  return DLSM_OK;
}

int dlsm_version_masks_advance_dev(dlsm_ctx* ctx, uint64_t* slot_mask_dev, const uint8_t* hit_dev, uint64_t n) {
  if (!ctx || n > 0xffffffffull) return DLSM_E_ARG;
  if (n == 0) return DLSM_OK;
  if (!slot_mask_dev || !hit_dev) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  DeviceGuard g(ctx->device);
  DLSM_TRY(launch_masks_advance(slot_mask_dev, hit_dev, n, ctx->stream));
  return DLSM_OK;
}

// ---------------------------------------------------------------------------
// Shard route: DBImpl_Sharding::Get_Target_Shard for a Get batch
// ---------------------------------------------------------------------------
static_assert(DLSM_MAX_SHARDS == kSortBins - 1 && DLSM_ROUTE_ALIGN == kRouteAlign, "shard route constants");

struct dlsm_shardmap {
  int device = 0;
  int n_shards = 0;
  uint8_t* mem = nullptr;  // one allocation: prefixes | byte offsets | bytes (plan::ShardMapImage)
  RouteBounds b{};         // device pointers into mem
};

int dlsm_shardmap_create(dlsm_ctx* ctx, const uint8_t* const* upper_bounds, const uint64_t* lens, int n_shards,
                         dlsm_shardmap** out) {
  if (!out) return DLSM_E_ARG;
  *out = nullptr;
  ShardMapImage M;
  DLSM_CHECK(plan_shardmap(upper_bounds, lens, n_shards, M));
  if (!ctx) return DLSM_E_ARG;
  DeviceGuard g(ctx->device);
  uint8_t* mem = nullptr;
  DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&mem), M.total));
  hipStream_t s = ctx->stream;
  hipError_t e = hipMemcpyAsync(mem + M.pre_off, M.pre.data(), sizeof(RoutePrefix) * M.pre.size(),
                                hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(mem + M.off_off, M.off.data(), sizeof(uint64_t) * M.off.size(), hipMemcpyHostToDevice, s);
  if (e == hipSuccess && !M.bytes.empty())
    e = hipMemcpyAsync(mem + M.bytes_off, M.bytes.data(), M.bytes.size(), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = ctx_sync(ctx, s);  // the image is pageable host memory
  if (e != hipSuccess) {
    (void)hipFree(mem);
    return from_hip(e);
  }
  dlsm_shardmap* m = new (std::nothrow) dlsm_shardmap;
  if (!m) {
    (void)hipFree(mem);
    return DLSM_E_NOMEM;
  }
  m->device = ctx->device;
  m->n_shards = n_shards;
  m->mem = mem;
  m->b.pre = reinterpret_cast<const RoutePrefix*>(mem + M.pre_off);
  m->b.off = reinterpret_cast<const uint64_t*>(mem + M.off_off);
  m->b.bytes = mem + M.bytes_off;
  m->b.n = static_cast<uint32_t>(n_shards);
  *out = m;
  return DLSM_OK;
}

int dlsm_shardmap_destroy(dlsm_shardmap* m) {
  if (!m) return DLSM_OK;
  DeviceGuard g(m->device);
  if (m->mem) (void)hipFree(m->mem);
  delete m;
  return DLSM_OK;
}

int dlsm_shardmap_size(const dlsm_shardmap* m, int* n_shards) {
  if (!m) return DLSM_E_ARG;
  if (n_shards) *n_shards = m->n_shards;
  return DLSM_OK;
}

uint64_t dlsm_shard_route_cap(uint64_t n, int n_shards) { return shard_route_cap(n, n_shards < 0 ? 0 : n_shards); }

uint32_t dlsm_shard_route_chunk(void) { return kRouteChunk; }

int dlsm_shard_route_dev(dlsm_ctx* ctx, const dlsm_shardmap* map, const dlsm_keyset* keys, uint64_t* shard_off_dev,
                         uint64_t* shard_cnt_dev, uint32_t* gets_dev, uint8_t* keys_out_dev, uint64_t cap) {
  if (!ctx || !map || !keys || map->device != ctx->device) return DLSM_E_ARG;
  if (!shard_off_dev || !shard_cnt_dev) return DLSM_E_ARG;
  DLSM_CHECK(validate_keyset(*keys));
  const uint64_t n = keys->n;
  if (keys_out_dev && keys->offsets) return DLSM_E_ARG;  // variable-length keys: the indices only
  ShardRoute R;
  DLSM_CHECK(plan_shard_route(n, map->n_shards, kSortMaxWgs, R));
  if (cap < shard_route_cap(n, map->n_shards) || (n > 0 && !gets_dev)) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  if (n == 0) {
    DLSM_TRY(hipMemsetAsync(shard_off_dev, 0, sizeof(uint64_t) * R.bins, s));
    DLSM_TRY(hipMemsetAsync(shard_cnt_dev, 0, sizeof(uint64_t) * R.bins, s));
    return DLSM_OK;
  }
  DLSM_CHECK(ctx->route_ws.ensure(R.bytes));
  uint8_t* ws = ctx->route_ws.p;
  ShardRouteDev a{};
  a.bounds = map->b;
  a.keys = to_desc(*keys);
  a.bins = R.bins;
  a.cpw = R.cpw;
  a.nwg = R.nwg;
  a.ids = reinterpret_cast<uint16_t*>(ws + R.ids_off);
  a.cnt = reinterpret_cast<uint32_t*>(ws + R.cnt_off);
  a.off = reinterpret_cast<uint64_t*>(ws + R.off_off);
  a.shard_off = shard_off_dev;
  a.shard_cnt = shard_cnt_dev;
  a.gets = gets_dev;
  a.keys_out = keys_out_dev;
  a.cap = cap;
  DLSM_TRY(launch_shard_route(a, s));
  return DLSM_OK;
}

int dlsm_shard_route(dlsm_ctx* ctx, const dlsm_shardmap* map, const dlsm_keyset* keys, uint64_t* shard_off,
                     uint64_t* shard_cnt, uint32_t* gets, uint8_t* keys_out, uint64_t cap) {
  if (!ctx || !map || !keys || !shard_off || !shard_cnt) return DLSM_E_ARG;
  DLSM_CHECK(validate_keyset(*keys));
  if (keys_out && keys->offsets) return DLSM_E_ARG;
  const uint64_t n = keys->n, bins = static_cast<uint64_t>(map->n_shards) + 1;
  if (n > 0xffffffffull || cap < shard_route_cap(n, map->n_shards) || (n > 0 && !gets)) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const dlsm_keyset* sets[1] = {keys};
  std::vector<dlsm_keyset> dk;
  DLSM_CHECK(stage_keys(ctx, sets, 1, dk));
  // staging: [shard_off | shard_cnt | gets | keys_out], each 256-byte aligned
  auto pad = [](uint64_t b) { return (b + 255) & ~uint64_t(255); };
  const uint64_t co = pad(8 * bins), go = co + pad(8 * bins), ko = go + pad(4 * cap);
  const uint64_t kb = keys_out ? cap * keys->key_len : 0;
  DLSM_CHECK(ctx->st_out.ensure(ko + kb));
  uint8_t* st = ctx->st_out.p;
  DLSM_CHECK(dlsm_shard_route_dev(ctx, map, &dk[0], reinterpret_cast<uint64_t*>(st),
                                  reinterpret_cast<uint64_t*>(st + co), reinterpret_cast<uint32_t*>(st + go),
                                  keys_out ? st + ko : nullptr, cap));
  DLSM_TRY(hipMemcpyAsync(shard_off, st, 8 * bins, hipMemcpyDeviceToHost, s));
  DLSM_TRY(hipMemcpyAsync(shard_cnt, st + co, 8 * bins, hipMemcpyDeviceToHost, s));
  DLSM_TRY(ctx_sync(ctx, s));
  // only the runs are defined: the gaps are copied as they are and the caller's
  // gap slots keep what the device staging held, so copy run by run
  for (uint64_t b = 0; b < bins; b++) {
    if (!shard_cnt[b]) continue;
    DLSM_TRY(hipMemcpyAsync(gets + shard_off[b], st + go + 4 * shard_off[b], 4 * shard_cnt[b], hipMemcpyDeviceToHost, s));
    if (keys_out)
      DLSM_TRY(hipMemcpyAsync(keys_out + shard_off[b] * keys->key_len, st + ko + shard_off[b] * keys->key_len,
                              shard_cnt[b] * keys->key_len, hipMemcpyDeviceToHost, s));
  }
  DLSM_TRY(ctx_sync(ctx, s));
  return DLSM_OK;
}

// ---------------------------------------------------------------------------
// Table index: Table::InternalGet's index step (table/table.cc:452-513) for a
// planned Get batch (index_seek.hip)
// ---------------------------------------------------------------------------
static_assert(sizeof(dlsm_kv_handle) == sizeof(KvHandle) && offsetof(dlsm_kv_handle, size) == offsetof(KvHandle, size) &&
                  offsetof(dlsm_kv_handle, file) == offsetof(KvHandle, file),
              "handle layout");
static_assert(DLSM_GET_NOTFOUND == kGetNotFound && DLSM_GET_FOUND == kGetFound && DLSM_GET_DELETED == kGetDeleted &&
                  DLSM_GET_CORRUPT == kGetCorrupt,
              "Get states");

struct dlsm_tableindex {
  int device = 0;
  int n_files = 0;
  uint64_t n_entries = 0;
  uint64_t bytes = 0;
  uint8_t* arena = nullptr;       // the held files' blocks, each at a multiple of 256 bytes
  IndexFileDev* files = nullptr;  // n_files records
  RoutePrefix* fence = nullptr;   // the fence table
  uint64_t* slot0 = nullptr;      // the open's slot prefix sums
};

// The device half of the open: copy + crc (the ingest pass), the validation
// launches and the records' way back, behind one synchronisation.
static int tableindex_open(dlsm_ctx* ctx, const uint8_t* const* blocks, const uint64_t* lens, int blocks_are_device,
                           bool verify, const IndexOpen& P, dlsm_tableindex* ti, std::vector<uint8_t>& st) {
  hipStream_t s = ctx->stream;
  const int n_files = ti->n_files;
  DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&ti->arena), std::max<uint64_t>(P.arena_bytes, 256)));
  DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&ti->files), sizeof(IndexFileDev) * std::max(n_files, 1)));
  DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&ti->fence), sizeof(RoutePrefix) * std::max<uint64_t>(P.fences, 1)));
  DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&ti->slot0), sizeof(uint64_t) * P.slot0.size()));
  ti->bytes = P.arena_bytes + sizeof(IndexFileDev) * n_files + sizeof(RoutePrefix) * P.fences;
  std::vector<IndexFileDev> h(n_files, IndexFileDev{});
  std::vector<IngestBlock> blk;
  blk.reserve(P.held);
  for (int f = 0; f < n_files; f++) {
    if (!blocks[f]) continue;
    uint8_t* slot = ti->arena + P.arena_off[f];
    h[f].data = slot;
    h[f].fence0 = P.fence0[f];
    h[f].len = static_cast<uint32_t>(lens[f] >= 5 ? lens[f] - 5 : 0);
    h[f].rec = P.rec[f];
    IngestBlock b{blocks[f], slot, lens[f]};
    if (!blocks_are_device) {  // one copy to the slot, then the pass runs in place
      b.src = slot;
      if (lens[f]) DLSM_TRY(hipMemcpyAsync(slot, blocks[f], lens[f], hipMemcpyHostToDevice, s));
    }
    blk.push_back(b);
  }
  DLSM_CHECK(ctx_upload(ctx, ti->files, h.data(), sizeof(IndexFileDev) * n_files, s));
  DLSM_CHECK(ctx_upload(ctx, ti->slot0, P.slot0.data(), sizeof(uint64_t) * P.slot0.size(), s));
  std::vector<IngestRecord> recs;
  DLSM_CHECK(queue_ingest(ctx, blk, verify, false, recs));
  DLSM_TRY(launch_index_open(ti->files, ctx->ing_rec.p, ti->slot0, static_cast<uint32_t>(n_files), P.slots, ti->fence, s));
  if (n_files) DLSM_TRY(hipMemcpyAsync(h.data(), ti->files, sizeof(IndexFileDev) * n_files, hipMemcpyDeviceToHost, s));
  DLSM_TRY(ctx_sync(ctx, s));
  int ret = DLSM_OK;
  for (int f = 0; f < n_files; f++) {
    st[f] = DLSM_BLOCK_OK;
    if (!blocks[f]) continue;
    const uint32_t r = recs[P.rec[f]].status;
    st[f] = static_cast<uint8_t>(r != DLSM_INGEST_OK ? r : (h[f].bad ? DLSM_BLOCK_INDEX : DLSM_BLOCK_OK));
    if (st[f] != DLSM_BLOCK_OK) ret = DLSM_E_CORRUPT;
    ti->n_entries += h[f].n;
  }
  return ret;
}

int dlsm_tableindex_create_blocks(dlsm_ctx* ctx, const uint8_t* const* blocks, const uint64_t* lens, int n_files,
                                  int blocks_are_device, int verify_checksums, uint8_t* status,
                                  dlsm_tableindex** out) {
  if (!out) return DLSM_E_ARG;
  *out = nullptr;
  if (!ctx || n_files < 0 || (n_files > 0 && (!blocks || !lens))) return DLSM_E_ARG;
  std::vector<uint8_t> present(n_files);
  for (int f = 0; f < n_files; f++) present[f] = blocks[f] != nullptr;
  IndexOpen P;
  DLSM_CHECK(plan_index_open(lens, present.data(), n_files, kIndexFenceS, P));
  if (ctx->fault) return -ctx->fault;
  DeviceGuard g(ctx->device);
  dlsm_tableindex* ti = new (std::nothrow) dlsm_tableindex();
  if (!ti) return DLSM_E_NOMEM;
  ti->device = ctx->device;
  ti->n_files = n_files;
  std::vector<uint8_t> st(n_files, DLSM_BLOCK_OK);
  const int ret = tableindex_open(ctx, blocks, lens, blocks_are_device, verify_checksums != 0, P, ti, st);
  if (status && (ret == DLSM_OK || ret == DLSM_E_CORRUPT) && n_files) memcpy(status, st.data(), n_files);
  if (ret != DLSM_OK) {
    dlsm_tableindex_destroy(ti);
    return ret;
  }
  (void)hipFree(ti->slot0);  // the open's only
  ti->slot0 = nullptr;
  *out = ti;
  return DLSM_OK;
}

int dlsm_tableindex_destroy(dlsm_tableindex* ti) {
  if (!ti) return DLSM_OK;
  DeviceGuard g(ti->device);
  if (ti->slot0) (void)hipFree(ti->slot0);
  if (ti->fence) (void)hipFree(ti->fence);
  if (ti->files) (void)hipFree(ti->files);
  if (ti->arena) (void)hipFree(ti->arena);
  delete ti;
  return DLSM_OK;
}

int dlsm_tableindex_size(const dlsm_tableindex* ti, int* n_files, uint64_t* n_entries, uint64_t* device_bytes) {
  if (!ti) return DLSM_E_ARG;
  if (n_files) *n_files = ti->n_files;
  if (n_entries) *n_entries = ti->n_entries;
  if (device_bytes) *device_bytes = ti->bytes;
  return DLSM_OK;
}

uint32_t dlsm_index_fence_interval(void) { return kIndexFenceS; }
uint32_t dlsm_index_seek_block(void) { return kIndexSeekBlock; }

int dlsm_index_block_check(const uint8_t* contents, uint64_t len, uint64_t* n_entries) {
  if (n_entries) *n_entries = 0;
  if (!contents && len) return DLSM_E_ARG;
  IndexView v;
  if (!index_header_valid(contents, len, &v)) return DLSM_E_CORRUPT;
  for (uint32_t i = 0; i < v.n; i++)
    if (!index_entry_valid(v, i)) return DLSM_E_CORRUPT;
  if (n_entries) *n_entries = v.n;
  return DLSM_OK;
}

int dlsm_index_block_seek(const uint8_t* contents, uint64_t len, const uint8_t* user_key, uint64_t key_len,
                          uint64_t snapshot, uint32_t file, uint8_t* state, dlsm_kv_handle* handle) {
  if (state) *state = DLSM_GET_NOTFOUND;
  if (handle) *handle = dlsm_kv_handle{0, 0, 0};
  if ((!contents && len) || (!user_key && key_len) || key_len > 0xffffffffull) return DLSM_E_ARG;
  if (snapshot > ((uint64_t(1) << 56) - 1)) return DLSM_E_ARG;
  IndexView v;
  if (!index_view(contents, len, &v)) return DLSM_E_CORRUPT;
  KvHandle h;
  const uint8_t st = index_block_seek(v, user_key, static_cast<uint32_t>(key_len), snapshot, file, &h);
  if (state) *state = st;
  if (handle) *handle = dlsm_kv_handle{h.offset, h.size, h.file};
  return DLSM_OK;
}

int dlsm_index_seek_dev(dlsm_ctx* ctx, const dlsm_tableindex* ti, const dlsm_keyset* keys, uint64_t snapshot,
                        const uint64_t* file_begin_dev, const uint32_t* gets_dev, uint64_t cap,
                        uint8_t* task_state_dev, dlsm_kv_handle* task_handle_dev, uint8_t* get_state_dev,
                        dlsm_kv_handle* get_handle_dev) {
  if (!ctx || !ti || !keys || ti->device != ctx->device) return DLSM_E_ARG;
  if (snapshot > ((uint64_t(1) << 56) - 1)) return DLSM_E_ARG;  // kMaxSequenceNumber
  DLSM_CHECK(validate_keyset(*keys));
  if (keys->n > 0xffffffffull || !file_begin_dev || (cap > 0 && !gets_dev)) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  if (ti->n_files == 0 || cap == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  IndexSeekDev a{};
  a.files = ti->files;
  a.fence = ti->fence;
  a.n_files = static_cast<uint32_t>(ti->n_files);
  a.keys = to_desc(*keys);
  a.trailer = index_seek_trailer(snapshot);
  a.file_begin = file_begin_dev;
  a.gets = gets_dev;
  a.cap = cap;
  a.task_state = task_state_dev;
  a.task_handle = reinterpret_cast<KvHandle*>(task_handle_dev);
  a.get_state = get_state_dev;
  a.get_handle = reinterpret_cast<KvHandle*>(get_handle_dev);
  DLSM_TRY(launch_index_seek(a, plan_index_seek_wgs(cap, kIndexSeekMaxWgs), ctx->stream));
  return DLSM_OK;
}

int dlsm_index_seek(dlsm_ctx* ctx, const dlsm_tableindex* ti, const dlsm_keyset* keys, uint64_t snapshot,
                    const uint64_t* file_begin, const uint32_t* gets, uint64_t cap, uint8_t* task_state,
                    dlsm_kv_handle* task_handle, uint8_t* get_state, dlsm_kv_handle* get_handle) {
  if (!ctx || !ti || !keys || !file_begin || ti->device != ctx->device) return DLSM_E_ARG;
  DLSM_CHECK(validate_keyset(*keys));
  if (keys->n > 0xffffffffull || snapshot > ((uint64_t(1) << 56) - 1)) return DLSM_E_ARG;
  const uint64_t nf = static_cast<uint64_t>(ti->n_files), n = keys->n;
  const uint64_t limit = std::min(file_begin[nf], cap);
  if (limit > 0 && !gets) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  if (limit == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const dlsm_keyset* sets[1] = {keys};
  std::vector<dlsm_keyset> dk;
  DLSM_CHECK(stage_keys(ctx, sets, 1, dk));
  // staging: [file_begin | gets | task states | task handles | get states | get handles]
  Layout L;
  const uint64_t fo = L.take(8 * (nf + 1)), go = L.take(4 * limit), tso = L.take(limit), tho = L.take(16 * limit),
                 gso = L.take(n), gho = L.take(16 * n);
  DLSM_CHECK(ctx->st_out.ensure(L.at));
  uint8_t* st = ctx->st_out.p;
  DLSM_TRY(hipMemcpyAsync(st + fo, file_begin, 8 * (nf + 1), hipMemcpyHostToDevice, s));
  DLSM_TRY(hipMemcpyAsync(st + go, gets, 4 * limit, hipMemcpyHostToDevice, s));
  // the Get arrays are written only where a task found something: what the caller holds goes in first
  if (get_state && n) DLSM_TRY(hipMemcpyAsync(st + gso, get_state, n, hipMemcpyHostToDevice, s));
  if (get_handle && n) DLSM_TRY(hipMemcpyAsync(st + gho, get_handle, 16 * n, hipMemcpyHostToDevice, s));
  DLSM_CHECK(dlsm_index_seek_dev(ctx, ti, &dk[0], snapshot, reinterpret_cast<uint64_t*>(st + fo),
                                 reinterpret_cast<uint32_t*>(st + go), limit, task_state ? st + tso : nullptr,
                                 task_handle ? reinterpret_cast<dlsm_kv_handle*>(st + tho) : nullptr,
                                 get_state ? st + gso : nullptr,
                                 get_handle ? reinterpret_cast<dlsm_kv_handle*>(st + gho) : nullptr));
  if (task_state) DLSM_TRY(hipMemcpyAsync(task_state, st + tso, limit, hipMemcpyDeviceToHost, s));
  if (task_handle) DLSM_TRY(hipMemcpyAsync(task_handle, st + tho, 16 * limit, hipMemcpyDeviceToHost, s));
  if (get_state && n) DLSM_TRY(hipMemcpyAsync(get_state, st + gso, n, hipMemcpyDeviceToHost, s));
  if (get_handle && n) DLSM_TRY(hipMemcpyAsync(get_handle, st + gho, 16 * n, hipMemcpyDeviceToHost, s));
  DLSM_TRY(ctx_sync(ctx, s));
  return DLSM_OK;
}

// ---------------------------------------------------------------------------
// Value read: the tail of Table::InternalGet (table/table.cc:482-508) for a
// seeked Get batch (kv_read.hip)
// ---------------------------------------------------------------------------
struct dlsm_tabledata {
  int device = 0;
  int n_files = 0;
  uint64_t n_chunks = 0;
  uint64_t bytes = 0;
  uint8_t* tables = nullptr;  // [chunk_begin | end | base], each region 256-byte aligned
  uint8_t* arena = nullptr;   // host chunks' copies
  KvTables t{};
};

int dlsm_tabledata_create(dlsm_ctx* ctx, const dlsm_data_chunk* chunks, const uint32_t* chunk_begin, int n_files,
                          int chunks_are_device, dlsm_tabledata** out) {
  if (!out) return DLSM_E_ARG;
  *out = nullptr;
  if (!ctx || n_files < 0) return DLSM_E_ARG;
  TableDataPlan P;
  DLSM_CHECK(plan_tabledata(chunks, chunk_begin, n_files, P));
  if (ctx->fault) return -ctx->fault;
  DeviceGuard g(ctx->device);
  dlsm_tabledata* td = new (std::nothrow) dlsm_tabledata();
  if (!td) return DLSM_E_NOMEM;
  td->device = ctx->device;
  td->n_files = n_files;
  td->n_chunks = P.end.size();
  const uint64_t nc = td->n_chunks;
  auto run = [&]() -> int {
    hipStream_t s = ctx->stream;
    Layout L;
    const uint64_t bo = L.take(sizeof(uint32_t) * (static_cast<uint64_t>(n_files) + 1)), eo = L.take(sizeof(uint64_t) * nc),
                   po = L.take(sizeof(uint8_t*) * nc);
    DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&td->tables), L.at));
    if (!chunks_are_device) DLSM_TRY(hipMalloc(reinterpret_cast<void**>(&td->arena), std::max<uint64_t>(P.arena_bytes, 256)));
    td->bytes = L.at + (chunks_are_device ? 0 : P.arena_bytes);
    std::vector<const uint8_t*> base(nc);
    for (uint64_t c = 0; c < nc; c++) {
      base[c] = chunks[c].base;
      if (chunks_are_device) continue;
      base[c] = td->arena + P.arena_off[c];
      if (chunks[c].len)
        DLSM_TRY(hipMemcpyAsync(td->arena + P.arena_off[c], chunks[c].base, chunks[c].len, hipMemcpyHostToDevice, s));
    }
    DLSM_CHECK(ctx_upload(ctx, td->tables + bo, chunk_begin, sizeof(uint32_t) * (static_cast<uint64_t>(n_files) + 1), s));
    DLSM_CHECK(ctx_upload(ctx, td->tables + eo, P.end.data(), sizeof(uint64_t) * nc, s));
    DLSM_CHECK(ctx_upload(ctx, td->tables + po, base.data(), sizeof(uint8_t*) * nc, s));
    DLSM_TRY(ctx_sync(ctx, s));  // the caller's host chunks are free again
    td->t.chunk_begin = reinterpret_cast<const uint32_t*>(td->tables + bo);
    td->t.end = reinterpret_cast<const uint64_t*>(td->tables + eo);
    td->t.base = reinterpret_cast<const uint8_t* const*>(td->tables + po);
    td->t.n_files = static_cast<uint32_t>(n_files);
    return DLSM_OK;
  };
  const int ret = run();
  if (ret != DLSM_OK) {
    dlsm_tabledata_destroy(td);
    return ret;
  }
  *out = td;
  return DLSM_OK;
}

int dlsm_tabledata_destroy(dlsm_tabledata* td) {
  if (!td) return DLSM_OK;
  DeviceGuard g(td->device);
  if (td->arena) (void)hipFree(td->arena);
  if (td->tables) (void)hipFree(td->tables);
  delete td;
  return DLSM_OK;
}

int dlsm_tabledata_size(const dlsm_tabledata* td, int* n_files, uint64_t* n_chunks, uint64_t* device_bytes) {
  if (!td) return DLSM_E_ARG;
  if (n_files) *n_files = td->n_files;
  if (n_chunks) *n_chunks = td->n_chunks;
  if (device_bytes) *device_bytes = td->bytes;
  return DLSM_OK;
}

uint32_t dlsm_kv_read_chunk(void) { return kKvChunk; }
uint32_t dlsm_kv_read_span(void) { return kKvSpan; }

int dlsm_kv_pair_read(const dlsm_data_chunk* chunks, uint32_t n_chunks, const dlsm_kv_handle* handle,
                      const uint8_t* user_key, uint64_t key_len, uint8_t* state, const uint8_t** value,
                      uint32_t* value_len) {
  if (value) *value = nullptr;
  if (value_len) *value_len = 0;
  if (!state || !handle || (!chunks && n_chunks) || (!user_key && key_len) || key_len > 0xffffffffull) return DLSM_E_ARG;
  if (*state != DLSM_GET_FOUND) return DLSM_OK;
  std::vector<uint64_t> end(n_chunks);
  std::vector<const uint8_t*> base(n_chunks);
  uint64_t at = 0;
  for (uint32_t c = 0; c < n_chunks; c++) {
    if ((chunks[c].len && !chunks[c].base) || at + chunks[c].len < at) return DLSM_E_ARG;
    end[c] = at += chunks[c].len;
    base[c] = chunks[c].base;
  }
  const uint8_t* v = nullptr;
  uint32_t vl = 0;
  const uint8_t* p = kv_pair_locate(KvChunks{end.data(), base.data(), n_chunks}, handle->offset, handle->size);
  *state = p ? kv_pair_decide(p, handle->size, user_key, static_cast<uint32_t>(key_len), &v, &vl) : kGetCorrupt;
  if (value) *value = v;
  if (value_len) *value_len = vl;
  return DLSM_OK;
}

int dlsm_kv_read_dev(dlsm_ctx* ctx, const dlsm_tabledata* td, const dlsm_keyset* keys, const uint32_t* gets_dev,
                     const uint64_t* count_dev, uint64_t cap, uint8_t* state_dev, const dlsm_kv_handle* handle_dev,
                     uint64_t* value_off_dev, uint8_t* values_dev, uint64_t values_cap, uint64_t* n_corrupt_dev) {
  if (!ctx || !td || !keys || td->device != ctx->device) return DLSM_E_ARG;
  DLSM_CHECK(validate_keyset(*keys));
  KvReadPlan P;
  DLSM_CHECK(plan_kv_read(cap, kSortMaxWgs, kKvCopyWgs, P));  // (the copy's grid: below, once the device is known)
  if (keys->n > 0xffffffffull) return DLSM_E_ARG;
  if (cap > 0 && (!state_dev || !handle_dev || !value_off_dev || (values_cap > 0 && !values_dev))) return DLSM_E_ARG;
  if (!aligned(values_dev, 16) || !aligned(handle_dev, 8) || !aligned(value_off_dev, 8) || !aligned(count_dev, 8) ||
      !aligned(gets_dev, 4) || !aligned(n_corrupt_dev, 8))
    return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  if (cap == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  if (!ctx->cus) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0)
      cus = kKvCopyWgs / kKvCopyWgsPerCu;
    ctx->cus = cus;
  }
  P.copy_wgs = plan_kv_copy_wgs(static_cast<uint32_t>(ctx->cus));
  for (hipEvent_t& e : ctx->ev_kv)
    if (!e) DLSM_TRY(hipEventCreate(&e));
  ctx->kv_timed = false;
  DLSM_CHECK(ctx->kv_ws.ensure(P.bytes));
  uint8_t* ws = ctx->kv_ws.p;
  KvReadDev a{};
  a.tables = td->t;
  a.keys = to_desc(*keys);
  a.gets = gets_dev;
  a.count = count_dev;
  a.cap = cap;
  a.state = state_dev;
  a.handle = reinterpret_cast<const KvHandle*>(handle_dev);
  a.value_off = value_off_dev;
  a.values = values_dev;
  a.values_cap = values_cap;
  a.n_corrupt = n_corrupt_dev;
  a.len = reinterpret_cast<uint32_t*>(ws + P.len_off);
  a.src = reinterpret_cast<uint64_t*>(ws + P.src_off);
  a.wg_sum = reinterpret_cast<uint64_t*>(ws + P.sum_off);
  a.wg_bad = reinterpret_cast<uint64_t*>(ws + P.bad_off);
  a.cpw = P.cpw;
  a.nwg = P.nwg;
  DLSM_TRY(launch_kv_read(a, P.copy_wgs, ctx->ev_kv, ctx->stream));
  ctx->kv_timed = true;
  return DLSM_OK;
}

int dlsm_kv_read_stats(const dlsm_ctx* ctx, double* launch_ms, uint32_t* copy_wgs) {
  if (!ctx) return DLSM_E_ARG;
  if (copy_wgs) *copy_wgs = ctx->cus ? plan_kv_copy_wgs(static_cast<uint32_t>(ctx->cus)) : 0;
  if (launch_ms) {
    launch_ms[0] = launch_ms[1] = launch_ms[2] = 0;
    if (!ctx->kv_timed) return DLSM_OK;
    DeviceGuard g(ctx->device);
    for (int j = 0; j < 3; j++) {
      float ms = 0;
      DLSM_TRY(hipEventElapsedTime(&ms, ctx->ev_kv[j], ctx->ev_kv[j + 1]));
      launch_ms[j] = ms;
    }
  }
  return DLSM_OK;
}

int dlsm_kv_read(dlsm_ctx* ctx, const dlsm_tabledata* td, const dlsm_keyset* keys, const uint32_t* gets,
                 const uint64_t* count, uint64_t cap, uint8_t* state, const dlsm_kv_handle* handle,
                 uint64_t* value_off, uint8_t* values, uint64_t values_cap, uint64_t* n_corrupt) {
  if (!ctx || !td || !keys || td->device != ctx->device || cap > 0xffffffffull) return DLSM_E_ARG;
  DLSM_CHECK(validate_keyset(*keys));
  if (keys->n > 0xffffffffull) return DLSM_E_ARG;
  const uint64_t m = count ? std::min(*count, cap) : cap;
  if (cap > 0 && (!value_off || (m > 0 && (!state || !handle)) || (values_cap > 0 && !values))) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  if (cap == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const dlsm_keyset* sets[1] = {keys};
  std::vector<dlsm_keyset> dk;
  DLSM_CHECK(stage_keys(ctx, sets, 1, dk));
  // staging: [gets | states | handles | value_off | corrupt count | values]; the call runs on the m items
  Layout L;
  const uint64_t go = L.take(4 * m), so = L.take(m), ho = L.take(16 * m), vo = L.take(8 * (m + 1)), co = L.take(8),
                 bo = L.take(values_cap);
  DLSM_CHECK(ctx->st_out.ensure(L.at + 256));
  uint8_t* st = ctx->st_out.p;
  if (m) {
    if (gets) DLSM_TRY(hipMemcpyAsync(st + go, gets, 4 * m, hipMemcpyHostToDevice, s));
    DLSM_TRY(hipMemcpyAsync(st + so, state, m, hipMemcpyHostToDevice, s));
    DLSM_TRY(hipMemcpyAsync(st + ho, handle, 16 * m, hipMemcpyHostToDevice, s));
  }
  uint64_t total = 0;
  if (m) {
    DLSM_CHECK(dlsm_kv_read_dev(ctx, td, &dk[0], gets ? reinterpret_cast<uint32_t*>(st + go) : nullptr, nullptr, m, st + so,
                                reinterpret_cast<dlsm_kv_handle*>(st + ho), reinterpret_cast<uint64_t*>(st + vo), st + bo,
                                values_cap, reinterpret_cast<uint64_t*>(st + co)));
    DLSM_TRY(hipMemcpyAsync(value_off, st + vo, 8 * (m + 1), hipMemcpyDeviceToHost, s));
    if (n_corrupt) DLSM_TRY(hipMemcpyAsync(n_corrupt, st + co, 8, hipMemcpyDeviceToHost, s));
    DLSM_TRY(ctx_sync(ctx, s));
    total = value_off[m];
  } else {
    value_off[0] = 0;
    if (n_corrupt) *n_corrupt = 0;
  }
  const uint64_t nb = std::min(total, values_cap);
  if (nb) DLSM_TRY(hipMemcpyAsync(values, st + bo, nb, hipMemcpyDeviceToHost, s));
  // the states, the call's only in-out array, are replaced once nothing can
  // fail any more: a caller that re-runs a failed call on the host (the
  // adapter) still holds the incoming ones
  std::vector<uint8_t> new_state(m);
  if (m) DLSM_TRY(hipMemcpyAsync(new_state.data(), st + so, m, hipMemcpyDeviceToHost, s));
  if (nb || m) DLSM_TRY(ctx_sync(ctx, s));
  if (m) memcpy(state, new_state.data(), m);
  return DLSM_OK;
}

// ---------------------------------------------------------------------------
// Legacy FilterPolicy format (util/bloom.cc)
// ---------------------------------------------------------------------------
int dlsm_bloom_legacy_build_dev(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs,
                                int bits_per_key, uint64_t* out_len_dev) {
  if (!ctx || n_jobs < 0 || (n_jobs > 0 && (!jobs || !out_len_dev))) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  if (n_jobs == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const int k = legacy_num_probes(bits_per_key);
  bool all_k20 = true, all_k28 = true;
  bool fits_a = k <= kLegacyKmaxA, fits_b = k <= kLegacyKmaxB;
  uint64_t ws = 0;
  std::vector<uint64_t> wpos(n_jobs), lens(n_jobs);
  std::vector<uint32_t> tiles(n_jobs), regions(n_jobs);
  for (int j = 0; j < n_jobs; j++) {
    DLSM_CHECK(validate_keyset(jobs[j].keys));
    if (!jobs[j].out) return DLSM_E_ARG;
    const uint64_t bits = legacy_bits(jobs[j].keys.n, bits_per_key);
    lens[j] = bits / 8 + 1;
    if (lens[j] > jobs[j].out_cap) return DLSM_E_CAPACITY;
    wpos[j] = ws;
    ws += (bits / 8 + 3 + 255) & ~uint64_t(255);
    all_k20 = all_k20 && is_k20(jobs[j].keys);
    all_k28 = all_k28 && is_k28(jobs[j].keys);
    // the LDS-tiled path: positions as u16 inside 2^16-bit tiles, one chunk's
    // region (k positions per key + up to 7 pads per tile) staged in LDS
    const uint64_t nt = (bits + (uint64_t(1) << kLegacyTileLg) - 1) >> kLegacyTileLg;
    const uint64_t reg = (static_cast<uint64_t>(k) * kLegacyChunk + 7 * nt + 7) & ~uint64_t(7);
    tiles[j] = static_cast<uint32_t>(std::min<uint64_t>(nt, 0xffffffffu));
    regions[j] = static_cast<uint32_t>(std::min<uint64_t>(reg, 0xffffffffu));
    const bool ok = bits <= 0xffffffffull && jobs[j].keys.n <= 0x7fffffffull * kLegacyChunk;
    fits_a = fits_a && ok && nt <= kLegacyTilesA && reg <= kLegacyStageA;
    fits_b = fits_b && ok && nt <= kLegacyTilesB && reg <= kLegacyStageB;
  }
  const int mode = all_k20 ? KM_K20 : (all_k28 ? KM_K28 : KM_GENERIC);
  if (ctx->path != 1 && fits_b) {
    const char* tps = getenv("DLSM_LEGACY_TPS_LG");  // A/B knob
    const int tps_lg = choose_legacy_tps_lg(tiles, tps ? atoi(tps) : -1);
    const JobTable<LegacyTileJobDev> T =
        plan_legacy_tile_jobs(jobs, n_jobs, bits_per_key, out_len_dev, tiles, regions, tps_lg, k);
    const std::vector<LegacyTileJobDev>& hj = T.hj;
    const std::vector<uint32_t>& starts = T.starts;
    const uint64_t entry = T.entry, tabw = T.tabw;
    const uint32_t chunk = T.chunk, slice = T.slice;
    DLSM_CHECK(ctx->ltjobs.ensure(n_jobs));
    DLSM_CHECK(ctx->ltstarts.ensure(2 * n_jobs));
    DLSM_CHECK(ctx->lentries.ensure(entry + 8));
    DLSM_CHECK(ctx->ltab.ensure(tabw + 1));
    DLSM_CHECK(ctx_upload(ctx, ctx->ltjobs.p, hj.data(), sizeof(LegacyTileJobDev) * n_jobs, s));
    DLSM_CHECK(ctx_upload(ctx, ctx->ltstarts.p, starts.data(), sizeof(uint32_t) * 2 * n_jobs, s));
    DLSM_TRY(launch_legacy_partition(ctx->ltjobs.p, ctx->ltstarts.p, n_jobs, chunk, ctx->lentries.p, ctx->ltab.p,
                                     fits_a ? 0 : 1, mode, s));
    DLSM_TRY(launch_legacy_slices(ctx->ltjobs.p, ctx->ltstarts.p + n_jobs, n_jobs, slice, ctx->lentries.p,
                                  ctx->ltab.p, tps_lg, s));
    return DLSM_OK;
  }
  // path 2 (sliced forced) with a batch the tiled kernels cannot take
  // (k > kLegacyKmaxB, i.e. bits_per_key >= 14, or too many tiles): the
  // direct kernel builds it -- the same bytes
  // Direct path: global atomics into an aligned workspace, then copies to the slots.
  DLSM_CHECK(ctx->st_filter.ensure(ws + 256));
  DLSM_TRY(hipMemsetAsync(ctx->st_filter.p, 0, ws, s));
  for (int j0 = 0; j0 < n_jobs; j0 += 256) {
    const int nj = std::min(256, n_jobs - j0);
    std::vector<LegacyJobDev> hj(nj);
    std::vector<uint64_t> key0s(nj);
    uint64_t tk = 0;
    for (int q = 0; q < nj; q++) {
      const dlsm_build_job& b = jobs[j0 + q];
      LegacyJobDev& d = hj[q];
      d.keys = to_desc(b.keys);
      d.out = ctx->st_filter.p + wpos[j0 + q];
      d.bits = legacy_bits(b.keys.n, bits_per_key);
      d.magic = d.bits <= 0xffffffffull ? fastmod_magic(static_cast<uint32_t>(d.bits)) : 0;
      d.k = k;
      d.key0 = tk;
      key0s[q] = tk;
      tk += b.keys.n;
    }
    DLSM_CHECK(ctx->ljobs.ensure(nj));
    DLSM_CHECK(ctx->lstarts.ensure(nj));
    DLSM_CHECK(ctx_upload(ctx, ctx->ljobs.p, hj.data(), sizeof(LegacyJobDev) * nj, s));
    DLSM_CHECK(ctx_upload(ctx, ctx->lstarts.p, key0s.data(), sizeof(uint64_t) * nj, s));
    DLSM_TRY(launch_legacy_scatter(ctx->ljobs.p, ctx->lstarts.p, nj, tk, mode == KM_K20 ? KM_K20 : KM_GENERIC, s));
    // the job table is reused by the next group: keep the stream ordered
  }
  for (int j = 0; j < n_jobs; j++) {
    DLSM_TRY(hipMemcpyAsync(jobs[j].out, ctx->st_filter.p + wpos[j], lens[j] - 1,
                            hipMemcpyDeviceToDevice, s));
    DLSM_TRY(hipMemsetAsync(jobs[j].out + lens[j] - 1, static_cast<int>(static_cast<uint8_t>(k)), 1, s));
  }
  DLSM_CHECK(ctx_upload(ctx, out_len_dev, lens.data(), sizeof(uint64_t) * n_jobs, s));
  return DLSM_OK;
}

int dlsm_bloom_legacy_build(dlsm_ctx* ctx, const dlsm_build_job* jobs, int n_jobs, int bits_per_key,
                            uint64_t* out_len) {
  if (!ctx || n_jobs < 0 || (n_jobs > 0 && (!jobs || !out_len))) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  if (n_jobs == 0) return DLSM_OK;
  DeviceGuard g(ctx->device);
  std::vector<const dlsm_keyset*> sets(n_jobs);
  for (int j = 0; j < n_jobs; j++) {
    DLSM_CHECK(validate_keyset(jobs[j].keys));
    if (!jobs[j].out) return DLSM_E_ARG;
    const uint64_t len = legacy_bits(jobs[j].keys.n, bits_per_key) / 8 + 1;
    if (len > jobs[j].out_cap) return DLSM_E_CAPACITY;
    sets[j] = &jobs[j].keys;
  }
  std::vector<dlsm_keyset> dk;
  DLSM_CHECK(stage_keys(ctx, sets.data(), n_jobs, dk));
  std::vector<dlsm_build_job> dj(n_jobs);
  std::vector<uint64_t> opos(n_jobs);
  uint64_t ob = 0;
  for (int j = 0; j < n_jobs; j++) {
    const uint64_t len = legacy_bits(jobs[j].keys.n, bits_per_key) / 8 + 1;
    opos[j] = ob;
    ob += (len + 255) & ~uint64_t(255);
    dj[j].keys = dk[j];
    dj[j].out_cap = len;
  }
  DLSM_CHECK(ctx->st_out.ensure(ob + 256));
  DLSM_CHECK(ctx->st_len.ensure(n_jobs));
  for (int j = 0; j < n_jobs; j++) dj[j].out = ctx->st_out.p + opos[j];
  DLSM_CHECK(dlsm_bloom_legacy_build_dev(ctx, dj.data(), n_jobs, bits_per_key, ctx->st_len.p));
  hipStream_t s = ctx->stream;
  for (int j = 0; j < n_jobs; j++) {
    out_len[j] = dj[j].out_cap;
    DLSM_TRY(hipMemcpyAsync(jobs[j].out, dj[j].out, out_len[j], hipMemcpyDeviceToHost, s));
  }
  DLSM_TRY(ctx_sync(ctx, s));
  return DLSM_OK;
}

int dlsm_bloom_legacy_probe_dev(dlsm_ctx* ctx, const uint8_t* filter_dev, uint64_t len,
                                const dlsm_keyset* keys, uint8_t* out_dev) {
  if (!ctx || !keys) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  DLSM_CHECK(validate_keyset(*keys));
  if (keys->n == 0) return DLSM_OK;
  if (!out_dev) return DLSM_E_ARG;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  // util/bloom.cc:57-81: len < 2 -> false; k (signed char -> size_t) > 30 -> true.
  int trivial = 0, k = 0;
  uint64_t bits = 0;
  if (len < 2 || !filter_dev) {
    trivial = 1;
  } else {
    uint8_t kb;
    DLSM_TRY(hipMemcpyAsync(&kb, filter_dev + len - 1, 1, hipMemcpyDeviceToHost, s));
    DLSM_TRY(ctx_sync(ctx, s));
    const int ks = static_cast<int>(static_cast<int8_t>(kb));
    if (ks < 0 || ks > 30) trivial = 2;
    else if (ks == 0) trivial = 2;  // zero probes -> match
    k = ks;
    bits = (len - 1) * 8;
  }
  const uint32_t magic = (bits && bits <= 0xffffffffull) ? fastmod_magic(static_cast<uint32_t>(bits)) : 0;
  const int mode = is_k20(*keys) ? KM_K20 : KM_GENERIC;
  DLSM_TRY(launch_legacy_probe(filter_dev, bits, magic, k, trivial, to_desc(*keys), out_dev, mode, s));
  return DLSM_OK;
}

int dlsm_bloom_legacy_probe(dlsm_ctx* ctx, const uint8_t* filter, uint64_t len,
                            const dlsm_keyset* keys, uint8_t* out) {
  if (!ctx || !keys) return DLSM_E_ARG;
  if (ctx->fault) return -ctx->fault;
  DLSM_CHECK(validate_keyset(*keys));
  if (keys->n == 0) return DLSM_OK;
  if (!out) return DLSM_E_ARG;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const dlsm_keyset* sets[1] = {keys};
  std::vector<dlsm_keyset> dk;
  DLSM_CHECK(stage_keys(ctx, sets, 1, dk));
  const uint8_t* fdev = nullptr;
  if (filter && len) {
    DLSM_CHECK(ctx->st_filter.ensure(len));
    DLSM_TRY(hipMemcpyAsync(ctx->st_filter.p, filter, len, hipMemcpyHostToDevice, s));
    fdev = ctx->st_filter.p;
  }
  DLSM_CHECK(ctx->st_out.ensure(keys->n));
  DLSM_CHECK(dlsm_bloom_legacy_probe_dev(ctx, fdev, len, &dk[0], ctx->st_out.p));
  DLSM_TRY(hipMemcpyAsync(out, ctx->st_out.p, keys->n, hipMemcpyDeviceToHost, s));
  DLSM_TRY(ctx_sync(ctx, s));
  return DLSM_OK;
}

}  // extern "C"
