// tests/cpp/adapter_shard_test.cc -- dlsm_adapter::ShardRouter.
//   (no argument)  host only: Shard and host::RouteShards against
//                  std::map<std::string, int>::upper_bound and a stable sort on
//                  adversarial bounds; the C ABI's argument checks, which need
//                  no device.  Prints "OK adapter shard host".
//   gpu            Route on the device against host::RouteShards (identical
//                  arrays, fallback counter 0), then with an injected fault
//                  (the host answers, counted once).  Prints "OK adapter shard gpu".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>

#include "dlsm_bloom_adapter.hpp"

using dlsm_adapter::ShardRouter;
using dlsm_adapter::Slice;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                \
      printf("\n");                                       \
      exit(1);                                            \
    }                                                     \
  } while (0)

typedef std::vector<std::string> Strs;

static Strs crowded(size_t want, uint32_t seed) {
  std::mt19937 rng(seed);
  std::set<std::string> s;
  const std::string pre[4] = {std::string(16, '\0'), std::string("0000000000000042", 16),
                              std::string(15, '\x80') + '\xff', std::string(16, '\xff')};
  const char alphabet[4] = {'\0', 'a', '\x80', '\xff'};
  while (s.size() < want) {
    std::string k = pre[rng() % 4];
    const uint32_t cut = rng() % 8;
    if (cut == 0) k.resize(rng() % 17);
    const uint32_t tail = rng() % 7;
    for (uint32_t i = 0; i < tail && cut != 0; i++) k.push_back(alphabet[rng() % 4]);
    s.insert(k);
  }
  return Strs(s.begin(), s.end());
}

static std::vector<Strs> bound_sets() {
  std::vector<Strs> sets;
  const std::string P(16, 'p');
  sets.push_back({P, P + std::string(1, '\0'), P + std::string(2, '\0'), P + "a", P + "ab", P + "\x80", P + "\xff"});
  sets.push_back({"", "k", std::string(15, 'k'), std::string(16, 'k'), std::string(17, 'k'), std::string(40, 'k')});
  sets.push_back({std::string(1, '\0'), std::string(2, '\0'), std::string("\0\1", 2), std::string("a\0", 2),
                  std::string("a\0\0", 3), std::string("a\0b", 3), "\x7f", "\x80", std::string("\x80\0", 2), "\xff",
                  "\xff\xff"});
  sets.push_back({"m"});
  sets.push_back({std::string(20, 'g'), std::string(20, 't')});
  sets.push_back(crowded(255, 7));
  sets.push_back(crowded(511, 11));
  return sets;
}

static Strs lookups(const Strs& bounds) {
  Strs keys;
  for (const std::string& b : bounds) {
    keys.push_back(b);
    if (!b.empty()) keys.push_back(b.substr(0, b.size() - 1));
    keys.push_back(b + std::string(1, '\0'));
    keys.push_back(b + "\xff");
  }
  keys.push_back("");
  keys.push_back(bounds.back() + "\xff\xff");
  keys.push_back(std::string(41, '\xff'));
  return keys;
}

// ShardInfo in a shuffled order with one repeated upper bound: the router sorts
// it as shards_pool does.
static ShardRouter::ShardInfo shuffled_info(const Strs& bounds, std::vector<size_t>* where) {
  std::vector<size_t> perm(bounds.size());
  for (size_t i = 0; i < perm.size(); i++) perm[i] = i;
  std::mt19937 rng(static_cast<uint32_t>(bounds.size()));
  std::shuffle(perm.begin(), perm.end(), rng);
  ShardRouter::ShardInfo info;
  where->assign(bounds.size(), 0);
  for (size_t i = 0; i < perm.size(); i++) {
    where->at(perm[i]) = i;
    info.push_back(std::make_pair(Slice(), Slice(bounds[perm[i]])));  // lower bounds are never read
  }
  info.push_back(std::make_pair(Slice(), Slice(bounds[0])));  // a repeat: the first entry stays
  return info;
}

// The yardstick's arrays: upper_bound per key, a stable sort, padded offsets.
struct Want {
  std::vector<uint64_t> off, cnt;
  std::vector<uint32_t> gets;
};
static Want want_route(const Strs& bounds, const Strs& keys, uint64_t cap) {
  std::map<std::string, int> pool;
  for (size_t i = 0; i < bounds.size(); i++) pool[bounds[i]] = static_cast<int>(i);
  const size_t bins = bounds.size() + 1;
  std::vector<uint32_t> bin(keys.size());
  Want w;
  w.cnt.assign(bins, 0);
  for (size_t g = 0; g < keys.size(); g++) {
    const auto it = pool.upper_bound(keys[g]);
    bin[g] = it == pool.end() ? static_cast<uint32_t>(bounds.size()) : static_cast<uint32_t>(it->second);
    w.cnt[bin[g]]++;
  }
  std::vector<uint32_t> order(keys.size());
  for (size_t g = 0; g < keys.size(); g++) order[g] = static_cast<uint32_t>(g);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return bin[a] < bin[b]; });
  w.off.assign(bins, 0);
  w.gets.assign(cap, 0xdeadbeefu);
  uint64_t end = 0, at = 0;
  for (size_t s = 0; s < bins; s++) {
    w.off[s] = (end + 3) & ~uint64_t(3);
    for (uint64_t q = 0; q < w.cnt[s]; q++) w.gets[w.off[s] + q] = order[at++];
    end = w.off[s] + w.cnt[s];
  }
  return w;
}

static void pack(const Strs& keys, std::string* bytes, std::vector<uint64_t>* offs) {
  offs->assign(1, 0);
  for (const std::string& k : keys) {
    bytes->append(k);
    offs->push_back(bytes->size());
  }
  bytes->push_back('\0');
}

static void test_host() {
  for (const Strs& bounds : bound_sets()) {
    const int n = static_cast<int>(bounds.size());
    std::vector<size_t> where;
    ShardRouter r(shuffled_info(bounds, &where));
    CHECK(r.n_shards() == n, "%d shards", r.n_shards());
    std::map<std::string, int> pool;
    for (int i = 0; i < n; i++) pool[bounds[i]] = i;
    const Strs keys = lookups(bounds);
    for (const std::string& k : keys) {
      const auto it = pool.upper_bound(k);
      const int want = it == pool.end() ? -1 : it->second;
      CHECK(r.Shard(Slice(k)) == want, "%d bounds: Shard %d, upper_bound %d", n, r.Shard(Slice(k)), want);
      if (want >= 0) CHECK(r.InfoIndex(want) == where[want], "InfoIndex");
    }
    // the host route, variable-length keys (indices only)
    std::string bytes;
    std::vector<uint64_t> offs;
    pack(keys, &bytes, &offs);
    const dlsm_keyset ks{reinterpret_cast<const uint8_t*>(bytes.data()), offs.data(), 0, 0, keys.size()};
    const uint64_t cap = ShardRouter::Cap(keys.size(), n);
    CHECK(cap == ((keys.size() + 3ull * (n + 1) + 3) & ~3ull), "cap");
    const Want w = want_route(bounds, keys, cap);
    std::vector<uint64_t> off(n + 1, 7), cnt(n + 1, 7);
    std::vector<uint32_t> gets(cap, 0xdeadbeefu);
    CHECK(dlsm_adapter::host::RouteShards(bounds, ks, off.data(), cnt.data(), gets.data(), nullptr, cap) == DLSM_OK,
          "host route");
    CHECK(off == w.off && cnt == w.cnt && gets == w.gets, "%d bounds: host route differs", n);
    uint8_t dummy;
    CHECK(dlsm_adapter::host::RouteShards(bounds, ks, off.data(), cnt.data(), gets.data(), &dummy, cap) == DLSM_E_ARG,
          "keys_out with offsets");
    CHECK(dlsm_adapter::host::RouteShards(bounds, ks, off.data(), cnt.data(), gets.data(), nullptr, cap - 1) ==
              DLSM_E_ARG,
          "short cap");
  }
  // fixed 28-byte internal keys: the bin from the user key, the whole key moved
  {
    const Strs bounds = {std::string(20, 'g'), std::string(20, 't')};
    Strs users = {std::string(20, 'a'), std::string(20, 't'), std::string(20, 'g'), std::string(19, 'g') + "f",
                  std::string(20, 'z'), std::string(20, 'h')};
    std::string bytes;
    Strs ikeys;
    for (size_t i = 0; i < users.size(); i++) {
      const std::string trailer(8, static_cast<char>(0xf0 + i));  // would sort past every bound if compared
      bytes += users[i] + trailer;
    }
    const dlsm_keyset ks{reinterpret_cast<const uint8_t*>(bytes.data()), nullptr, 28, 8, users.size()};
    const uint64_t cap = ShardRouter::Cap(users.size(), 2);
    const Want w = want_route(bounds, users, cap);
    std::vector<uint64_t> off(3), cnt(3);
    std::vector<uint32_t> gets(cap, 0xdeadbeefu);
    std::vector<uint8_t> out(cap * 28, 0xa5);
    CHECK(dlsm_adapter::host::RouteShards(bounds, ks, off.data(), cnt.data(), gets.data(), out.data(), cap) == DLSM_OK,
          "host route 28");
    CHECK(off == w.off && cnt == w.cnt && gets == w.gets, "internal keys");
    for (uint64_t p = 0; p < cap; p++) {
      if (gets[p] == 0xdeadbeefu) {
        for (int x = 0; x < 28; x++) CHECK(out[p * 28 + x] == 0xa5, "gap row written");
      } else {
        CHECK(memcmp(&out[p * 28], bytes.data() + 28 * gets[p], 28) == 0, "row %llu", (unsigned long long)p);
      }
    }
  }
  // the C ABI's checks that need no device
  {
    const uint8_t a[] = "a", b[] = "b";
    const uint8_t* up[] = {a, b};
    const uint8_t* down[] = {b, a};
    const uint64_t l[] = {1, 1};
    dlsm_shardmap* m = reinterpret_cast<dlsm_shardmap*>(1);
    CHECK(dlsm_shardmap_create(nullptr, down, l, 2, &m) == DLSM_E_ARG && m == nullptr, "out of order");
    CHECK(dlsm_shardmap_create(nullptr, up, l, 0, &m) == DLSM_E_ARG, "0 shards");
    CHECK(dlsm_shardmap_create(nullptr, up, l, 512, &m) == DLSM_E_ARG, "512 shards");
    CHECK(dlsm_shardmap_create(nullptr, nullptr, l, 2, &m) == DLSM_E_ARG, "NULL bounds");
    CHECK(dlsm_shardmap_create(nullptr, up, nullptr, 2, &m) == DLSM_E_ARG, "NULL lens");
    CHECK(dlsm_shardmap_create(nullptr, up, l, 2, nullptr) == DLSM_E_ARG, "NULL out");
    CHECK(dlsm_shardmap_create(nullptr, up, l, 2, &m) == DLSM_E_ARG, "NULL context");
    CHECK(dlsm_shardmap_destroy(nullptr) == DLSM_OK, "destroy NULL");
    CHECK(dlsm_shardmap_size(nullptr, nullptr) == DLSM_E_ARG, "size NULL");
    dlsm_keyset ks{a, nullptr, 1, 0, 1};
    uint64_t o[3], c[3];
    uint32_t g[16];
    CHECK(dlsm_shard_route_dev(nullptr, nullptr, &ks, o, c, g, nullptr, 16) == DLSM_E_ARG, "route NULL");
    CHECK(dlsm_shard_route(nullptr, nullptr, &ks, o, c, g, nullptr, 16) == DLSM_E_ARG, "host route NULL");
    CHECK(dlsm_shard_route_cap(0, 1) == 8 && dlsm_shard_route_cap(5, 16) == 56 && dlsm_shard_route_cap(1, 511) == 1540,
          "cap");
    CHECK(dlsm_shard_route_chunk() >= 64 && dlsm_shard_route_chunk() % 64 == 0, "chunk");
  }
  printf("OK adapter shard host\n");
}

static void test_gpu() {
  dlsm_ctx* ctx = nullptr;
  CHECK(dlsm_ctx_create(0, &ctx) == DLSM_OK, "context");
  const uint32_t C = dlsm_shard_route_chunk();
  // db_bench-shaped 20-byte keys, 16 shards, and the adversarial sets
  std::mt19937_64 rng(3);
  const uint64_t n = C + 65;
  std::string bytes(n * 20, '0');
  for (uint64_t g = 0; g < n; g++) {
    const uint64_t v = rng() % 1100000;
    for (int i = 0; i < 8; i++) bytes[g * 20 + i] = static_cast<char>(v >> (56 - 8 * i));
  }
  Strs bounds;
  for (uint64_t s = 1; s <= 16; s++) {
    std::string b(20, '0');
    const uint64_t v = s * 62500;
    for (int i = 0; i < 8; i++) b[i] = static_cast<char>(v >> (56 - 8 * i));
    bounds.push_back(b);
  }
  auto run = [&](const Strs& bnd, const dlsm_keyset& ks, bool with_keys, int fault) {
    std::vector<size_t> where;
    ShardRouter r(shuffled_info(bnd, &where), ctx);
    const int ns = r.n_shards();
    const uint64_t cap = ShardRouter::Cap(ks.n, ns);
    std::vector<uint64_t> off(ns + 1, 7), cnt(ns + 1, 7), off2(ns + 1, 9), cnt2(ns + 1, 9);
    std::vector<uint32_t> gets(cap, 0xdeadbeefu), gets2(cap, 0xdeadbeefu);
    std::vector<uint8_t> out(with_keys ? cap * ks.key_len : 1, 0xa5), out2(out);
    uint64_t fb0 = 0, fb1 = 0;
    dlsm_fallback_stats(ctx, &fb0, nullptr);
    if (fault) CHECK(dlsm_ctx_set_option(ctx, DLSM_OPT_FAULT_INJECT, fault) == DLSM_OK, "inject");
    const int st = r.Route(ks, off.data(), cnt.data(), gets.data(), with_keys ? out.data() : nullptr, cap);
    if (fault) CHECK(dlsm_ctx_set_option(ctx, DLSM_OPT_FAULT_INJECT, 0) == DLSM_OK, "inject off");
    CHECK(st == DLSM_OK, "Route: %d", st);
    CHECK(r.status() == (fault ? -fault : DLSM_OK), "device status %d", r.status());
    dlsm_fallback_stats(ctx, &fb1, nullptr);
    CHECK(fb1 - fb0 == (fault ? 1u : 0u), "fallbacks %llu", (unsigned long long)(fb1 - fb0));
    CHECK(dlsm_adapter::host::RouteShards(bnd, ks, off2.data(), cnt2.data(), gets2.data(),
                                          with_keys ? out2.data() : nullptr, cap) == DLSM_OK,
          "host route");
    CHECK(off == off2 && cnt == cnt2, "offsets / counts differ");
    CHECK(gets == gets2, "gets differ");
    CHECK(out == out2, "keys_out differs");
  };
  const dlsm_keyset k20{reinterpret_cast<const uint8_t*>(bytes.data()), nullptr, 20, 0, n};
  run(bounds, k20, true, 0);
  run(bounds, k20, false, 0);
  run(bounds, k20, true, 4);
  for (const Strs& bnd : bound_sets()) {
    const Strs keys = lookups(bnd);
    std::string kb;
    std::vector<uint64_t> offs;
    pack(keys, &kb, &offs);
    const dlsm_keyset ks{reinterpret_cast<const uint8_t*>(kb.data()), offs.data(), 0, 0, keys.size()};
    run(bnd, ks, false, 0);
  }
  uint64_t fb = 9;
  dlsm_fallback_stats(ctx, &fb, nullptr);
  CHECK(fb == 1, "only the injected fault fell back: %llu", (unsigned long long)fb);
  dlsm_ctx_destroy(ctx);
  printf("OK adapter shard gpu\n");
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "gpu") == 0) test_gpu();
  else test_host();
  return 0;
}
