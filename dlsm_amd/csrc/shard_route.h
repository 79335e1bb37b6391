// dlsm_amd/csrc/shard_route.h -- the shard route's constants and its shard
// search, shared by the kernels (shard_route.hip), the planner (host_plan.h)
// and the CPU test (tests/cpp/shard_route_test.cc).  Plain integer code: no
// device call.
#pragma once
#include <stdint.h>

#include "bloom_math.h"
#include "sort_pass.h"

namespace dlsm {

// The route is one stable counting-sort pass (sort_pass.h) of the Gets by shard:
// the bins are the shards plus the "no shard" bin, n_shards + 1 <= kSortBins
// (DLSM_MAX_SHARDS = 511).
constexpr int kRouteChunkLg = 13;
constexpr uint32_t kRouteChunk = 1u << kRouteChunkLg;  // Gets per workgroup-chunk
constexpr uint32_t kRouteWaveItems = kRouteChunk / kSortWaves;  // a wave's contiguous share of a chunk
constexpr int kRouteHold = kRouteWaveItems / 64;      // Gets a lane holds in registers per chunk
constexpr uint32_t kRouteAlign = 4;                   // DLSM_ROUTE_ALIGN: every bin's run starts at a multiple
constexpr uint32_t kRouteStageKeyMax = 32;            // longest fixed key the 16-byte-load path stages (bytes)

static_assert(kRouteWaveItems % 64 == 0, "a wave walks its share 64 Gets at a time");
static_assert(kRouteWaveItems < (1u << (32 - kSortBinLg)), "rank and bin share a register");

// The first 16 bytes of a key, zero-padded, as two big-endian u64 (formed as
// VersionDev::pre_small is).  If two keys' prefixes differ, their order is
// Slice::compare's: at the first differing byte either both keys have a byte
// there, or the shorter key has ended (a pad zero) and is a proper prefix of
// the longer one, which Slice::compare also orders first.
struct RoutePrefix {
  uint64_t hi, lo;
};

DLSM_HD bool route_prefix_lt(const RoutePrefix& a, const RoutePrefix& b) {
  return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo);
}

DLSM_HD RoutePrefix route_prefix(const uint8_t* p, uint64_t n) {
  RoutePrefix r{0, 0};
  for (uint64_t i = 0; i < 16 && i < n; i++) {
    if (i < 8) r.hi |= static_cast<uint64_t>(p[i]) << (56 - 8 * i);
    else r.lo |= static_cast<uint64_t>(p[i]) << (56 - 8 * (i - 8));
  }
  return r;
}

// Slice::compare (include/TimberSaw/slice.h:112-122): memcmp over the common
// length, then the shorter key first.
DLSM_HD int route_compare(const uint8_t* a, uint64_t an, const uint8_t* b, uint64_t bn) {
  const uint64_t n = an < bn ? an : bn;
  for (uint64_t j = 0; j < n; j++) {
    const int d = static_cast<int>(a[j]) - static_cast<int>(b[j]);
    if (d) return d;
  }
  return an < bn ? -1 : (an > bn ? 1 : 0);
}

// The shards' upper bounds as the search reads them: pre[0, n) the bounds'
// prefixes (the kernels hold them in LDS), bound i's bytes at
// bytes[off[i], off[i + 1]) (the tie path only).  Strictly ascending.
struct RouteBounds {
  const RoutePrefix* pre;
  const uint64_t* off;  // n + 1
  const uint8_t* bytes;
  uint32_t n;           // 1 .. kSortBins - 1
};

// Get_Target_Shard (db/db_impl_sharding.h:41-55): shards_pool.upper_bound(key)
// as the number of bounds b with b <= key -- the key's shard, or n when the key
// lies at or past the last bound.  q = route_prefix(key, len).  A branchless
// lower bound over the prefixes counts the bounds whose prefix sorts below q
// (all below the key); only the bounds whose prefix equals q are compared in
// full, in order, until one sorts above the key.
DLSM_HD uint32_t route_shard(const RouteBounds& b, const RoutePrefix& q, const uint8_t* key, uint64_t len) {
  uint32_t lo = 0;  // bounds [0, lo) have a prefix < q
#pragma unroll
  for (uint32_t step = kSortBins >> 1; step; step >>= 1) {
    const uint32_t m = lo + step;
    const bool in = m <= b.n;
    const RoutePrefix p = b.pre[in ? m - 1 : 0];
    lo = (in && route_prefix_lt(p, q)) ? m : lo;
  }
  while (lo < b.n && b.pre[lo].hi == q.hi && b.pre[lo].lo == q.lo &&
         route_compare(b.bytes + b.off[lo], b.off[lo + 1] - b.off[lo], key, len) <= 0)
    lo++;
  return lo;
}

}  // namespace dlsm
