// tests/cpp/index_seek_test.cc -- the table index on the CPU: the entry decoder,
// the comparator, the validation rules, the fence window and the state decision
// the kernels run (dlsm_amd/csrc/index_seek.h) against a linear scan over the
// pairs the blocks were written from, one block per rejection reason, and the
// open's planner (dlsm::plan::plan_index_open).  The writer below restates
// BlockBuilder at restart interval 1 (table/block_builder.cc:74-127) on its own.
// Prints "OK" on success; exits non-zero with a message otherwise.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "../../dlsm_amd/csrc/host_plan.h"

using namespace dlsm;
using namespace dlsm::plan;

#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); \
      printf(__VA_ARGS__);                              \
      printf("\n");                                     \
      exit(1);                                          \
    }                                                   \
  } while (0)

struct Pair {
  std::string user;
  uint64_t trailer;  // seq << 8 | type
  uint64_t off, size;
};

static bool pair_less(const Pair& a, const Pair& b) {  // InternalKeyComparator
  if (a.user != b.user) return a.user < b.user;         // std::string compares as unsigned bytes
  return a.trailer > b.trailer;
}

static void put_varint(std::string& o, uint64_t v) {
  while (v >= 128) {
    o.push_back(static_cast<char>((v & 127) | 128));
    v >>= 7;
  }
  o.push_back(static_cast<char>(v));
}
static void put32(std::string& o, uint32_t v) { o.append(reinterpret_cast<const char*>(&v), 4); }
static std::string ikey(const Pair& p) {
  std::string k = p.user;
  k.append(reinterpret_cast<const char*>(&p.trailer), 8);
  return k;
}

static std::string write_block(const std::vector<Pair>& ps, std::vector<uint32_t>* restarts = nullptr) {
  std::string o;
  std::vector<uint32_t> r;
  for (const Pair& p : ps) {
    std::string v;
    put_varint(v, p.off);
    put_varint(v, p.size);
    const std::string k = ikey(p);
    r.push_back(static_cast<uint32_t>(o.size()));
    put_varint(o, 0);
    put_varint(o, k.size());
    put_varint(o, v.size());
    o += k + v;
  }
  for (uint32_t x : r) put32(o, x);
  put32(o, static_cast<uint32_t>(r.size()));
  if (restarts) *restarts = r;
  return o;
}

static const uint8_t* U(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }

static bool block_valid(const std::string& c, uint32_t* n = nullptr) {
  // an exact-size heap copy: the sanitizer sees any read past the contents
  std::vector<uint8_t> d(c.begin(), c.end());
  IndexView v;
  if (!index_header_valid(d.data(), d.size(), &v)) return false;
  bool ok = true;
  for (uint32_t i = 0; i < v.n; i++) ok = index_entry_valid(v, i) && ok;  // every entry runs, as on the device
  if (n) *n = v.n;
  return ok;
}

// The linear scan: the first pair >= (user, trailer(snapshot)), then the rules.
static uint8_t scan(const std::vector<Pair>& ps, const std::string& user, uint64_t snapshot, uint32_t file, KvHandle* h) {
  *h = KvHandle{0, 0, 0};
  const Pair t{user, (snapshot << 8) | 1, 0, 0};
  size_t i = 0;
  while (i < ps.size() && pair_less(ps[i], t)) i++;
  if (i == ps.size()) return kGetNotFound;
  const uint32_t type = ps[i].trailer & 0xff;
  uint8_t st;
  if (type > 1) st = kGetCorrupt;
  else if (ps[i].user != user) return kGetNotFound;
  else st = type == 1 ? kGetFound : kGetDeleted;
  *h = KvHandle{ps[i].off, static_cast<uint32_t>(ps[i].size), file};
  return st;
}

static std::vector<Pair> random_pairs(uint32_t seed, size_t want) {
  std::mt19937_64 rng(seed);
  const std::string pre[4] = {std::string(16, '\0'), std::string("0000000000000042", 16),
                              std::string(15, '\x80') + '\xff', std::string(16, '\xff')};
  const char alphabet[4] = {'\0', 'a', '\x80', '\xff'};
  std::vector<Pair> ps;
  while (ps.size() < want) {
    std::string k = pre[rng() % 4];
    const uint32_t cut = rng() % 6;
    if (cut == 0) k.resize(rng() % 17);
    for (uint32_t i = 0, tail = rng() % 5; i < tail && cut != 0; i++) k.push_back(alphabet[rng() % 4]);
    if (rng() % 16 == 0) k = std::string(112 + rng() % 20, 'L') + k;  // internal keys around 128 bytes
    const uint32_t versions = 1 + (rng() % 4 == 0 ? rng() % 40 : 0);
    for (uint32_t s = 0; s < versions; s++) {
      const uint64_t type = rng() % 23 == 0 ? 2 + rng() % 3 : rng() % 2;
      ps.push_back(Pair{k, ((rng() % 1000) << 8) | type, rng() >> (rng() % 64), rng() % 70000});
    }
  }
  std::sort(ps.begin(), ps.end(), pair_less);
  ps.erase(std::unique(ps.begin(), ps.end(), [](const Pair& a, const Pair& b) { return !pair_less(a, b) && !pair_less(b, a); }),
           ps.end());
  return ps;
}

// Every seek path against the scan: the fence window at several S (the
// kernel's shape), the fence-free host path, and the window's own claim.
static void seek_cases(const std::vector<Pair>& ps, uint32_t seed) {
  const std::string c = write_block(ps);
  std::vector<uint8_t> d(c.begin(), c.end());
  uint32_t n = 0;
  CHECK(block_valid(c, &n) && n == ps.size(), "a written block is valid (%zu pairs)", ps.size());
  IndexView v;
  CHECK(index_view(d.data(), d.size(), &v), "view");
  std::vector<std::string> targets;
  for (const Pair& p : ps) {
    targets.push_back(p.user);
    targets.push_back(p.user + std::string(1, '\0'));
    if (!p.user.empty()) targets.push_back(p.user.substr(0, p.user.size() - 1));
  }
  targets.push_back("");
  targets.push_back(std::string(40, '\xff'));
  std::mt19937_64 rng(seed);
  const uint64_t snaps[] = {0, 1, 499, 500, 999, 1000, (uint64_t(1) << 56) - 1};
  for (uint32_t S : {2u, 3u, 8u, 16u, 64u}) {
    const uint32_t nf = index_fence_count(v.n, S);
    std::vector<RoutePrefix> fence(nf);
    for (uint32_t j = 0; j < nf; j++) fence[j] = index_entry_prefix(v, j * S);
    for (const std::string& t : targets) {
      const uint64_t snap = snaps[rng() % 7];
      KvHandle want, got, got2;
      const uint8_t ws = scan(ps, t, snap, 9, &want);
      uint32_t lo = 0, hi = 0;
      if (v.n) index_fence_window(fence.data(), nf, v.n, S, route_prefix(U(t), t.size()), &lo, &hi);
      CHECK(lo <= hi && hi <= v.n, "window [%u, %u] of %u", lo, hi, v.n);
      const uint32_t pos = index_window_search(v, lo, hi, U(t), static_cast<uint32_t>(t.size()), index_seek_trailer(snap));
      // the window's claim: everything before lo is below the target, hi is not
      const Pair tp{t, (snap << 8) | 1, 0, 0};
      size_t first = 0;
      while (first < ps.size() && pair_less(ps[first], tp)) first++;
      CHECK(lo <= first && first <= hi && pos == first, "S=%u: window [%u, %u], found %u, scan %zu", S, lo, hi, pos, first);
      const uint8_t gs = index_decide(v, pos, U(t), static_cast<uint32_t>(t.size()), 9, &got);
      const uint8_t gs2 = index_block_seek(v, U(t), static_cast<uint32_t>(t.size()), snap, 9, &got2);
      CHECK(gs == ws && gs2 == ws, "state %d / %d, scan %d", gs, gs2, ws);
      CHECK(got.offset == want.offset && got.size == want.size && got.file == want.file, "handle");
      CHECK(got2.offset == want.offset && got2.size == want.size && got2.file == want.file, "handle (host path)");
    }
  }
}

static void decoder_cases() {
  // the comparator, 8 bytes at a time and at the tails
  const std::string a = "0123456789abcdefXYZ", b = "0123456789abcdefXYz";
  CHECK(index_compare_bytes(U(a), 19, U(b), 19) < 0 && index_compare_bytes(U(b), 19, U(a), 19) > 0, "tail byte");
  CHECK(index_compare_bytes(U(a), 16, U(b), 19) < 0 && index_compare_bytes(U(a), 19, U(a), 19) == 0, "prefix first");
  const std::string hi = std::string("\x80", 1) + std::string(8, 'a'), lo7 = std::string("\x7f", 1) + std::string(8, 'a');
  CHECK(index_compare_bytes(U(hi), 9, U(lo7), 9) > 0, "bytes compare unsigned");
  CHECK(index_compare_bytes(U(a), 0, U(b), 0) == 0 && index_compare_bytes(U(a), 0, U(b), 1) < 0, "empty keys");
  // trailers descend
  const Pair p1{"k", (7 << 8) | 1, 0, 0}, p2{"k", (6 << 8) | 1, 0, 0};
  const std::string k1 = ikey(p1), k2 = ikey(p2);
  CHECK(index_compare_internal(U(k1), 9, U(k2), 9) < 0 && index_compare_internal(U(k2), 9, U(k1), 9) > 0 &&
            index_compare_internal(U(k1), 9, U(k1), 9) == 0,
        "a higher sequence sorts first");
  // DecodeEntry: the fast path and the varint path give the same entry
  for (size_t ul : {0, 1, 20, 119, 120, 121, 300}) {
    const std::vector<Pair> one = {Pair{std::string(ul, 'u'), (3 << 8) | 1, (uint64_t(1) << 35) + 1, 129}};
    const std::string c = write_block(one);
    IndexView v;
    CHECK(index_view(U(c), c.size(), &v) && v.n == 1, "view");
    IndexEntry e;
    CHECK(index_decode(v, 0, &e) && e.shared == 0 && e.key_len == ul + 8 && e.val_len == 6 + 2, "decode %zu", ul);
    CHECK(e.key == (ul + 8 < 128 ? 3u : 4u) && e.val + e.val_len == v.restarts, "header bytes %zu", ul);
    uint64_t off, size;
    CHECK(index_handle(v, e, &off, &size) && off == (uint64_t(1) << 35) + 1 && size == 129, "handle");
  }
  // varint32: five bytes at most, the bits past 32 lost, no read at the limit
  const uint8_t five[6] = {0xff, 0xff, 0xff, 0xff, 0x7f, 0};
  uint32_t x = 0;
  CHECK(index_varint32(five, 0, 5, &x) == 5 && x == 0xffffffffu, "five bytes");
  CHECK(index_varint32(five, 0, 4, &x) == 0, "cut at the limit");
  const uint8_t six[6] = {0x80, 0x80, 0x80, 0x80, 0x80, 0x01};
  CHECK(index_varint32(six, 0, 6, &x) == 0, "a sixth byte is an error");
}

static void validation_cases() {
  std::vector<Pair> ps;
  for (int i = 0; i < 40; i++) ps.push_back(Pair{"key" + std::to_string(100 + i), (5 << 8) | 1, 1000u * i + 200, 41});
  std::vector<uint32_t> r;
  const std::string good = write_block(ps, &r);
  const size_t r0 = good.size() - 4 * (ps.size() + 1);
  CHECK(block_valid(good), "the untouched block");
  auto edit = [&](const char* what, std::function<void(std::string&)> fn) {
    std::string d = good;
    fn(d);
    CHECK(!block_valid(d), "%s must be rejected", what);
  };
  auto set32 = [](std::string& d, size_t at, uint32_t v) { memcpy(&d[at], &v, 4); };
  CHECK(!block_valid(std::string(3, '\0')), "len < 4");
  CHECK(block_valid(std::string(4, '\0')), "num_restarts == 0 is an empty table");
  CHECK(block_valid(std::string("garbage\0\0\0\0", 11)), "an empty table's bytes are never read");
  edit("num_restarts > (len - 4) / 4", [&](std::string& d) { set32(d, d.size() - 4, (d.size() - 4) / 4 + 1); });
  edit("num_restarts past the bytes", [&](std::string& d) { set32(d, d.size() - 4, (d.size() - 4) / 4); });
  edit("num_restarts one short", [&](std::string& d) { set32(d, d.size() - 4, ps.size() - 1); });
  edit("restart[0] != 0", [&](std::string& d) { set32(d, r0, 1); });
  edit("restarts equal", [&](std::string& d) { set32(d, r0 + 8, r[1]); });
  edit("restarts descending", [&](std::string& d) { set32(d, r0 + 8, r[1] - 1); });
  edit("restart past the entries", [&](std::string& d) { set32(d, r0 + 4 * (ps.size() - 1), r0 + 1); });
  edit("restart at the entries' end", [&](std::string& d) { set32(d, r0 + 4 * (ps.size() - 1), r0); });
  edit("shared != 0", [&](std::string& d) { d[r[3]] = 1; });
  edit("entry overruns", [&](std::string& d) { d[r[3] + 1]++; });
  edit("entry ends early", [&](std::string& d) { d[r[3] + 1]--; });
  edit("value overruns", [&](std::string& d) { d[r[3] + 2]++; });
  edit("last entry overruns the restart array", [&](std::string& d) { d[r.back() + 2]++; });
  edit("varint header without end", [&](std::string& d) { memset(&d[r[3]], 0x80, 6); });
  edit("value not two varints", [&](std::string& d) {
    const size_t val = r[3] + 3 + 14;
    d[val + 1] |= 0x80;  // the offset swallows the size byte
  });
  {
    std::vector<Pair> q = {Pair{"a", (5 << 8) | 1, 1, uint64_t(1) << 32}};
    CHECK(!block_valid(write_block(q)), "a size of 2^32 does not fit the handle");
    q[0].size = 0xffffffffu;
    CHECK(block_valid(write_block(q)), "a size of 2^32 - 1 does");
  }
  {  // non_shared < 8: written by hand
    std::string d;
    d += std::string("\0\7\4", 3) + "1234567" + std::string("\x81\1\x81\1", 4);  // 18 bytes with its restart
    put32(d, 0);
    put32(d, 1);
    CHECK(!block_valid(d), "non_shared < 8");
    d[1] = 8;  // the same bytes with an 8-byte key (and a 3-byte value) are a valid entry
    d[2] = 3;
    CHECK(block_valid(d), "non_shared == 8");
  }
  for (int how = 0; how < 3; how++) {  // order: swapped, equal, a newer version behind an older one
    std::vector<Pair> q = ps;
    if (how == 0) std::swap(q[7], q[8]);
    if (how == 1) q[8] = q[7];
    if (how == 2) {
      q[8].user = q[7].user;
      q[8].trailer = q[7].trailer + 256;
    }
    CHECK(!block_valid(write_block(q)), "order case %d", how);
  }
  // a varint-path header that spells the fast path's values is as valid as the reference finds it
  {
    std::string d;
    d += std::string("\x80\0", 2);  // shared = 0 in two bytes
    d += std::string("\x09\x02", 2) + std::string("k") + std::string(8, '\1') + std::string("\1\1", 2);
    put32(d, 0);
    put32(d, 1);
    CHECK(block_valid(d), "two-byte varint of 0");
  }
}

static void planner_cases() {
  const uint64_t lens[5] = {5 + 4 + 17 * 100, 0, 3, 5 + 4, 5 + 4 + 16};
  const uint8_t present[5] = {1, 0, 1, 1, 1};
  IndexOpen P;
  CHECK(plan_index_open(lens, present, 5, 16, P) == DLSM_OK, "plan");
  CHECK(P.held == 4 && P.slots == 100 && P.fences == 7 && P.slot0[0] == 0 && P.slot0[1] == 100 && P.slot0[5] == 100,
        "slots %llu fences %llu", (unsigned long long)P.slots, (unsigned long long)P.fences);
  CHECK(P.rec[0] == 0 && P.rec[2] == 1 && P.rec[3] == 2 && P.rec[4] == 3, "records");
  CHECK(P.arena_off[0] == 0 && P.arena_off[2] == 1792 && P.arena_off[3] == 2048 && P.arena_bytes == 2560, "arena");
  for (int f = 0; f < 5; f++) CHECK(P.arena_off[f] % 256 == 0, "aligned");
  const uint64_t big[1] = {uint64_t(1) << 32};
  CHECK(plan_index_open(big, present, 1, 16, P) == DLSM_E_ARG, "a block past 4 GiB");
  CHECK(plan_index_open(lens, present, 5, 0, P) == DLSM_E_ARG && plan_index_open(nullptr, present, 1, 16, P) == DLSM_E_ARG,
        "arguments");
  CHECK(plan_index_open(nullptr, nullptr, 0, 16, P) == DLSM_OK && P.slot0.size() == 1, "no files");
  CHECK(plan_index_seek_wgs(0, 2048) == 1 && plan_index_seek_wgs(256, 2048) == 1 && plan_index_seek_wgs(257, 2048) == 2 &&
            plan_index_seek_wgs(uint64_t(1) << 40, 2048) == 2048,
        "seek grid");
}

int main() {
  decoder_cases();
  validation_cases();
  planner_cases();
  seek_cases({}, 1);
  seek_cases({Pair{"", (1 << 8) | 1, 0, 0}}, 2);
  seek_cases({Pair{"only", (1 << 8) | 0, 5, 6}}, 3);
  for (uint32_t seed = 0; seed < 6; seed++) seek_cases(random_pairs(seed, 30 + 150 * seed), seed);
  {  // fixed 20-byte keys, one version each: the db_bench shape
    std::vector<Pair> ps;
    char b[32];
    for (int i = 0; i < 2000; i++) {
      snprintf(b, sizeof b, "%020d", 3 * i);
      ps.push_back(Pair{b, (uint64_t(i + 1) << 8) | 1, 64u * i, 128});
    }
    seek_cases(ps, 77);
  }
  printf("OK index seek\n");
  return 0;
}
