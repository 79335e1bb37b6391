// tests/cpp/shard_route_test.cc -- the shard route on the CPU: the shard search
// the kernels run (dlsm_amd/csrc/shard_route.h) against
// std::map<std::string, int>::upper_bound on adversarial bounds, the planner
// (dlsm::plan::plan_shard_route, shard_route_cap, shard_route_offsets), the host
// model of the pass (sort_model.h) fed in the kernels' item order with the
// planner's numbers against a stable sort, and the map's argument checks
// (plan_shardmap).
// Prints "OK" on success; exits non-zero with a message otherwise.
#include <algorithm>
#include <map>
#include <random>
#include <set>
#include <string>

#include "sort_model.h"

using namespace dlsm;
using namespace dlsm::plan;

typedef std::vector<std::string> Strs;

static std::string hex(const std::string& s) {
  std::string o;
  char b[4];
  for (unsigned char c : s) {
    snprintf(b, sizeof b, "%02x", c);
    o += b;
  }
  return o.empty() ? "(empty)" : o;
}

// Random bounds that crowd a few 16-byte prefixes: most neighbours tie on the
// prefix and differ after it, some are prefixes of the next.
static Strs crowded(size_t want, uint32_t seed) {
  std::mt19937 rng(seed);
  std::set<std::string> s;
  const std::string pre[4] = {std::string(16, '\0'), std::string("0000000000000042", 16),
                              std::string(15, '\x80') + '\xff', std::string(16, '\xff')};
  const char alphabet[4] = {'\0', 'a', '\x80', '\xff'};
  while (s.size() < want) {
    std::string k = pre[rng() % 4];
    const uint32_t cut = rng() % 8;
    if (cut == 0) k.resize(rng() % 17);  // shorter than the prefix
    const uint32_t tail = rng() % 7;
    for (uint32_t i = 0; i < tail && cut != 0; i++) k.push_back(alphabet[rng() % 4]);
    s.insert(k);
  }
  return Strs(s.begin(), s.end());
}

static std::vector<Strs> bound_sets() {
  std::vector<Strs> sets;
  const std::string P(16, 'p');
  // share their first 16 bytes and differ after; each a prefix of a later one
  sets.push_back({P, P + std::string(1, '\0'), P + std::string(2, '\0'), P + "a", P + "ab", P + "\x80", P + "\xff"});
  // lengths 0, 1, 15, 16, 17 and 40; every bound a prefix of the next
  sets.push_back({"", "k", std::string(15, 'k'), std::string(16, 'k'), std::string(17, 'k'), std::string(40, 'k')});
  // embedded and trailing zero bytes, bytes >= 0x80
  sets.push_back({std::string(1, '\0'), std::string(2, '\0'), std::string("\0\1", 2), std::string("a\0", 2),
                  std::string("a\0\0", 3), std::string("a\0b", 3), "\x7f", "\x80", std::string("\x80\0", 2), "\xff",
                  "\xff\xff"});
  sets.push_back({"m"});                                  // 1 shard
  sets.push_back({std::string(20, 'g'), std::string(20, 't')});  // 2 shards
  sets.push_back(crowded(255, 7));
  sets.push_back(crowded(511, 11));
  return sets;
}

static Strs lookups(const Strs& bounds) {
  Strs keys;
  for (const std::string& b : bounds) {
    keys.push_back(b);                                   // equal to the bound
    if (!b.empty()) keys.push_back(b.substr(0, b.size() - 1));  // one byte short
    keys.push_back(b + std::string(1, '\0'));            // one byte longer
    keys.push_back(b + "\xff");
    if (!b.empty()) {
      std::string c = b;
      c.back() = static_cast<char>(static_cast<unsigned char>(c.back()) + 1);  // (0xff wraps to 0: still a case)
      keys.push_back(c);
    }
  }
  keys.push_back("");
  keys.push_back(bounds.back() + "\xff\xff");            // past the last bound
  keys.push_back(std::string(41, '\xff'));
  return keys;
}

static void test_search() {
  for (const Strs& bounds : bound_sets()) {
    const int n = static_cast<int>(bounds.size());
    std::map<std::string, int> pool;  // shards_pool: upper bound -> shard
    for (int i = 0; i < n; i++) pool[bounds[i]] = i;
    CHECK(static_cast<int>(pool.size()) == n, "the bounds are distinct");
    std::vector<const uint8_t*> ptr(n);
    std::vector<uint64_t> len(n);
    for (int i = 0; i < n; i++) {
      ptr[i] = reinterpret_cast<const uint8_t*>(bounds[i].data());
      len[i] = bounds[i].size();
    }
    ShardMapImage M;
    CHECK(plan_shardmap(ptr.data(), len.data(), n, M) == DLSM_OK, "%d bounds", n);
    CHECK(M.pre.size() == static_cast<size_t>(n) && M.off.size() == static_cast<size_t>(n) + 1, "image");
    CHECK(M.pre_off % 256 == 0 && M.off_off % 256 == 0 && M.bytes_off % 256 == 0, "aligned regions");
    CHECK(M.off_off >= sizeof(RoutePrefix) * n && M.bytes_off >= M.off_off + 8 * (n + 1) &&
              M.total >= M.bytes_off + M.bytes.size(),
          "regions do not overlap");
    const uint8_t none = 0;
    const RouteBounds B{M.pre.data(), M.off.data(), M.bytes.empty() ? &none : M.bytes.data(),
                        static_cast<uint32_t>(n)};
    for (const std::string& k : lookups(bounds)) {
      const auto it = pool.upper_bound(k);
      const uint32_t want = it == pool.end() ? static_cast<uint32_t>(n) : static_cast<uint32_t>(it->second);
      const uint8_t* kp = reinterpret_cast<const uint8_t*>(k.data());
      const uint32_t got = route_shard(B, route_prefix(kp, k.size()), kp, k.size());
      CHECK(got == want, "%d bounds, key %s: shard %u, upper_bound says %u", n, hex(k).c_str(), got, want);
    }
  }
}

// The kernels' passes on the host, in their item order, with the planner's
// numbers: returns gets / off / cnt.
static void model(const std::vector<uint16_t>& bin, const ShardRoute& R, std::vector<uint64_t>& off,
                  std::vector<uint64_t>& cnt, std::vector<uint32_t>& gets, uint64_t cap) {
  std::vector<std::vector<uint32_t>> of_wg(R.nwg);
  sort_model::walk(R.nwg, R.cpw, kRouteChunk, bin.size(), [&](uint32_t w, uint64_t i0, uint64_t i1) {
    for (uint64_t g = i0; g < i1; g++) of_wg[w].push_back(static_cast<uint32_t>(g));
  });
  sort_model::Pass<uint32_t> S = sort_model::run_pass(of_wg, R.bins, R.table_entries, kRouteAlign, cap, 0xffffffffu,
                                                      [&](uint32_t g) { return bin[g]; });
  cnt = S.count;
  off.assign(R.bins, 0);
  const uint64_t end = shard_route_offsets(cnt.data(), R.bins, off.data());
  CHECK(end <= cap, "end %llu cap %llu", (unsigned long long)end, (unsigned long long)cap);
  CHECK(off == S.begin && end == S.end, "the planner's offsets are the pass's");
  gets.swap(S.out);
}

static void test_planner() {
  const uint64_t C = kRouteChunk;
  const uint32_t small_cap = 4;  // workgroups
  const uint64_t sizes[] = {0, 1, C - 1, C, C + 1, 3 * C + 3, uint64_t(small_cap) * C * 3 + 5};
  for (int n_shards : {1, 2, 16, 511}) {
    for (uint64_t n : sizes) {
      for (uint32_t max_wgs : {small_cap, kSortMaxWgs}) {
        ShardRoute R;
        CHECK(plan_shard_route(n, n_shards, max_wgs, R) == DLSM_OK, "n %llu", (unsigned long long)n);
        CHECK(R.bins == static_cast<uint32_t>(n_shards) + 1, "bins");
        CHECK(R.chunks == (n + C - 1) / C, "chunks");
        CHECK(R.nwg <= max_wgs && uint64_t(R.nwg) * R.cpw >= R.chunks, "the grid covers the chunks");
        CHECK(n == 0 ? R.nwg == 0 : uint64_t(R.nwg - 1) * R.cpw < R.chunks, "no idle workgroup");
        if (n > uint64_t(max_wgs) * C) CHECK(R.cpw > 1, "past the workgroup cap: several chunks each");
        CHECK(R.table_entries == uint64_t(R.bins) * R.nwg, "table");
        CHECK(R.ids_bytes == 2 * n && R.cnt_bytes == 4 * R.table_entries && R.off_bytes == 8 * R.table_entries,
              "sizes");
        CHECK(R.ids_off % 256 == 0 && R.cnt_off % 256 == 0 && R.off_off % 256 == 0, "aligned");
        CHECK(R.cnt_off >= R.ids_off + R.ids_bytes && R.off_off >= R.cnt_off + R.cnt_bytes &&
                  R.bytes >= R.off_off + R.off_bytes,
              "regions do not overlap");
        const uint64_t cap = shard_route_cap(n, n_shards);
        CHECK(cap % kRouteAlign == 0 && cap >= n + 3ull * (n_shards + 1) && cap < n + 3ull * (n_shards + 1) + 4,
              "cap");
        // random bins, then the pass model against a stable sort
        std::mt19937 rng(static_cast<uint32_t>(n * 31 + n_shards));
        std::vector<uint16_t> bin(n);
        for (uint64_t g = 0; g < n; g++) bin[g] = static_cast<uint16_t>(rng() % R.bins);
        std::vector<uint64_t> off, cnt;
        std::vector<uint32_t> gets;
        model(bin, R, off, cnt, gets, cap);
        std::vector<uint32_t> order(n);
        for (uint64_t g = 0; g < n; g++) order[g] = static_cast<uint32_t>(g);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return bin[a] < bin[b]; });
        uint64_t at = 0, prev_end = 0;
        for (uint32_t b = 0; b < R.bins; b++) {
          CHECK(off[b] % kRouteAlign == 0, "offset %llu", (unsigned long long)off[b]);
          CHECK(off[b] == ((prev_end + kRouteAlign - 1) & ~uint64_t(kRouteAlign - 1)), "previous end rounded up");
          for (uint64_t q = 0; q < cnt[b]; q++, at++)
            CHECK(gets[off[b] + q] == order[at] && bin[order[at]] == b, "bin %u item %llu", b, (unsigned long long)q);
          for (uint64_t p = prev_end; p < off[b]; p++) CHECK(gets[p] == 0xffffffffu, "gap written");
          prev_end = off[b] + cnt[b];
        }
        CHECK(at == n, "every Get placed once");
        for (uint64_t p = prev_end; p < cap; p++) CHECK(gets[p] == 0xffffffffu, "tail written");
      }
    }
    // the worst case: every bin wastes kRouteAlign - 1 slots; cap is then exactly
    // the last offset plus the last count, rounded up
    const uint32_t bins = static_cast<uint32_t>(n_shards) + 1;
    std::vector<uint64_t> cnt(bins), off(bins);
    uint64_t n = 0;
    for (uint32_t b = 0; b < bins; b++) n += cnt[b] = 4 * (b % 3) + 1;
    const uint64_t end = shard_route_offsets(cnt.data(), bins, off.data());
    CHECK(end == ((off[bins - 1] + cnt[bins - 1] + 3) & ~uint64_t(3)), "end");
    CHECK(shard_route_cap(n, n_shards) == end, "cap %llu end %llu", (unsigned long long)shard_route_cap(n, n_shards),
          (unsigned long long)end);
  }
  ShardRoute R;
  CHECK(plan_shard_route(1ull << 32, 4, kSortMaxWgs, R) == DLSM_E_ARG, "n > UINT32_MAX");
  CHECK(plan_shard_route(0xffffffffull, 511, kSortMaxWgs, R) == DLSM_OK && R.nwg <= kSortMaxWgs, "largest n");
  CHECK(plan_shard_route(10, 0, kSortMaxWgs, R) == DLSM_E_ARG, "no shard");
  CHECK(plan_shard_route(10, 512, kSortMaxWgs, R) == DLSM_E_ARG, "512 shards");
}

static void test_map_args() {
  const uint8_t a[] = "a", b[] = "b", ab[] = "ab";
  ShardMapImage M;
  {
    const uint8_t* p[] = {a, b};
    const uint64_t l[] = {1, 1};
    CHECK(plan_shardmap(p, l, 2, M) == DLSM_OK, "ascending");
    CHECK(plan_shardmap(p, l, 0, M) == DLSM_E_ARG, "0 shards");
    CHECK(plan_shardmap(p, l, -1, M) == DLSM_E_ARG, "-1 shards");
    CHECK(plan_shardmap(nullptr, l, 2, M) == DLSM_E_ARG, "NULL bounds");
    CHECK(plan_shardmap(p, nullptr, 2, M) == DLSM_E_ARG, "NULL lens");
  }
  {
    const uint8_t* p[] = {b, a};
    const uint64_t l[] = {1, 1};
    CHECK(plan_shardmap(p, l, 2, M) == DLSM_E_ARG, "descending");
  }
  {
    const uint8_t* p[] = {a, a};
    const uint64_t l[] = {1, 1};
    CHECK(plan_shardmap(p, l, 2, M) == DLSM_E_ARG, "equal bounds");
  }
  {
    const uint8_t* p[] = {ab, a};
    const uint64_t l[] = {2, 1};
    CHECK(plan_shardmap(p, l, 2, M) == DLSM_E_ARG, "a prefix after its extension");
    const uint8_t* q[] = {a, ab};
    const uint64_t m[] = {1, 2};
    CHECK(plan_shardmap(q, m, 2, M) == DLSM_OK, "a prefix before its extension");
  }
  {
    const uint8_t* p[] = {nullptr, a};
    const uint64_t l[] = {0, 1};
    CHECK(plan_shardmap(p, l, 2, M) == DLSM_OK, "an empty first bound");
    const uint64_t l1[] = {1, 1};
    CHECK(plan_shardmap(p, l1, 2, M) == DLSM_E_ARG, "NULL bound with a length");
  }
  {
    std::vector<std::string> s;
    for (int i = 0; i < 512; i++) s.push_back(std::string(1, static_cast<char>(i >> 8)) + static_cast<char>(i & 255));
    std::vector<const uint8_t*> p;
    std::vector<uint64_t> l;
    for (auto& x : s) {
      p.push_back(reinterpret_cast<const uint8_t*>(x.data()));
      l.push_back(x.size());
    }
    CHECK(plan_shardmap(p.data(), l.data(), 511, M) == DLSM_OK, "511 shards");
    CHECK(plan_shardmap(p.data(), l.data(), 512, M) == DLSM_E_ARG, "512 shards");
  }
}

int main() {
  test_search();
  test_planner();
  sort_model::test_grid();
  test_map_args();
  printf("OK\n");
  return 0;
}
