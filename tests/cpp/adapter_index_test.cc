// tests/cpp/adapter_index_test.cc -- dlsm_adapter::TableIndex and
// host::IndexBlockSeek.
//   (no argument)  host only: IndexBlockSeek and TableIndex::Seek against a
//                  linear scan over the pairs the blocks were written from;
//                  host::SeekPlan against the same scan; FromBlocks' status
//                  codes; SeekPlan on whatever the machine has (without a
//                  device the host answers).  Prints "OK adapter index host".
//   gpu            SeekPlan on the device against the scan (fallback counter
//                  0), then with an injected fault (the host answers, counted
//                  once).  Prints "OK adapter index gpu".
// The writer restates BlockBuilder at restart interval 1
// (table/block_builder.cc:74-127) by hand.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "dlsm_bloom_adapter.hpp"

using dlsm_adapter::Slice;
using dlsm_adapter::TableIndex;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                \
      printf("\n");                                       \
      exit(1);                                            \
    }                                                     \
  } while (0)

struct Pair {
  std::string user;
  uint64_t trailer;
  uint64_t off, size;
};
static bool pair_less(const Pair& a, const Pair& b) {
  if (a.user != b.user) return a.user < b.user;
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

static std::string write_contents(const std::vector<Pair>& ps) {
  std::string o;
  std::vector<uint32_t> r;
  for (const Pair& p : ps) {
    std::string k = p.user, v;
    k.append(reinterpret_cast<const char*>(&p.trailer), 8);
    put_varint(v, p.off);
    put_varint(v, p.size);
    r.push_back(static_cast<uint32_t>(o.size()));
    put_varint(o, 0);
    put_varint(o, k.size());
    put_varint(o, v.size());
    o += k + v;
  }
  for (uint32_t x : r) put32(o, x);
  put32(o, static_cast<uint32_t>(r.size()));
  return o;
}
static std::string sealed(std::string c) {
  const uint64_t n = c.size();
  c.resize(n + 5);
  dlsm_adapter::host::SealBlock(&c[0], n);
  return c;
}

static uint8_t scan(const std::vector<Pair>& ps, const std::string& user, uint64_t snapshot, uint32_t file,
                    dlsm_kv_handle* h) {
  *h = dlsm_kv_handle{0, 0, 0};
  const Pair t{user, (snapshot << 8) | 1, 0, 0};
  size_t i = 0;
  while (i < ps.size() && pair_less(ps[i], t)) i++;
  if (i == ps.size()) return DLSM_GET_NOTFOUND;
  const uint32_t type = ps[i].trailer & 0xff;
  uint8_t st;
  if (type > 1) st = DLSM_GET_CORRUPT;
  else if (ps[i].user != user) return DLSM_GET_NOTFOUND;
  else st = type == 1 ? DLSM_GET_FOUND : DLSM_GET_DELETED;
  *h = dlsm_kv_handle{ps[i].off, static_cast<uint32_t>(ps[i].size), file};
  return st;
}

static std::vector<Pair> table(uint32_t seed, size_t want) {
  std::mt19937_64 rng(seed);
  std::vector<Pair> ps;
  const std::string p16 = "0123456789abcdef";
  while (ps.size() < want) {
    std::string k;
    switch (rng() % 4) {
      case 0: k = p16 + std::string(1 + rng() % 3, static_cast<char>(rng() % 256)); break;
      case 1: k = std::string(rng() % 18, static_cast<char>('a' + rng() % 3)); break;
      case 2: k = std::string(110 + rng() % 20, 'L') + std::to_string(rng() % 50); break;
      default: {
        char b[32];
        snprintf(b, sizeof b, "%020llu", (unsigned long long)(rng() % 5000));
        k = b;
      }
    }
    const uint32_t versions = rng() % 5 == 0 ? 1 + rng() % 40 : 1;
    for (uint32_t s = 0; s < versions; s++)
      ps.push_back(Pair{k, ((rng() % 900) << 8) | (rng() % 29 == 0 ? 2 : rng() % 2), rng() >> (rng() % 60), rng() % 70000});
  }
  std::sort(ps.begin(), ps.end(), pair_less);
  ps.erase(std::unique(ps.begin(), ps.end(), [](const Pair& a, const Pair& b) { return !pair_less(a, b) && !pair_less(b, a); }),
           ps.end());
  return ps;
}

static std::vector<std::string> targets(const std::vector<Pair>& ps) {
  std::vector<std::string> t;
  for (const Pair& p : ps) {
    t.push_back(p.user);
    t.push_back(p.user + std::string(1, '\0'));
    if (!p.user.empty()) t.push_back(p.user.substr(0, p.user.size() - 1));
  }
  t.push_back("");
  t.push_back(std::string(30, '\xff'));
  return t;
}

static void pack(const std::vector<std::string>& keys, std::string* bytes, std::vector<uint64_t>* offs) {
  offs->assign(1, 0);
  for (const std::string& k : keys) {
    *bytes += k;
    offs->push_back(bytes->size());
  }
  bytes->append(16, '\0');
}

static bool same(const dlsm_kv_handle& a, const dlsm_kv_handle& b) {
  return a.offset == b.offset && a.size == b.size && a.file == b.file;
}

struct Fixture {
  std::vector<std::vector<Pair>> tabs;
  std::vector<std::string> blocks;
  std::vector<Slice> slices, contents;
  std::vector<std::string> keys;
  std::string kb;
  std::vector<uint64_t> offs, begin;
  std::vector<uint32_t> gets;
  dlsm_keyset ks;
};

// Four files (the third not held), every target of every held file as a task
// of that file, Get indices in a scrambled order.
static void make_fixture(Fixture* F) {
  F->tabs = {table(1, 300), table(2, 40), {}, table(3, 1)};
  for (size_t f = 0; f < F->tabs.size(); f++) F->blocks.push_back(f == 2 ? std::string() : sealed(write_contents(F->tabs[f])));
  for (size_t f = 0; f < F->tabs.size(); f++) {
    F->slices.push_back(f == 2 ? Slice(nullptr, 0) : Slice(F->blocks[f]));
    F->contents.push_back(f == 2 ? Slice(nullptr, 0) : Slice(F->blocks[f].data(), F->blocks[f].size() - 5));
  }
  F->begin.assign(1, 0);
  std::mt19937 rng(9);
  for (size_t f = 0; f < F->tabs.size(); f++) {
    const std::vector<std::string> t = targets(F->tabs[f == 2 ? 1 : f]);
    std::vector<uint32_t> g;
    for (const std::string& k : t) {
      g.push_back(static_cast<uint32_t>(F->keys.size()));
      F->keys.push_back(k);
    }
    std::shuffle(g.begin(), g.end(), rng);
    F->gets.insert(F->gets.end(), g.begin(), g.end());
    F->begin.push_back(F->gets.size());
  }
  pack(F->keys, &F->kb, &F->offs);
  F->ks = dlsm_keyset{reinterpret_cast<const uint8_t*>(F->kb.data()), F->offs.data(), 0, 0, F->keys.size()};
}

struct Arrays {
  std::vector<uint8_t> ts, gs;
  std::vector<dlsm_kv_handle> th, gh;
  Arrays(size_t cap, size_t n) : ts(cap, 0xee), gs(n, 0), th(cap, dlsm_kv_handle{7, 7, 7}), gh(n, dlsm_kv_handle{0, 0, 0}) {}
  bool operator==(const Arrays& o) const {
    if (ts != o.ts || gs != o.gs) return false;
    for (size_t i = 0; i < th.size(); i++)
      if (!same(th[i], o.th[i])) return false;
    for (size_t i = 0; i < gh.size(); i++)
      if (!same(gh[i], o.gh[i])) return false;
    return true;
  }
};

// The scan's arrays for the fixture's plan.
static Arrays scan_plan(const Fixture& F, uint64_t snap, uint64_t cap) {
  Arrays A(cap, F.keys.size());
  const uint64_t limit = std::min<uint64_t>(F.begin.back(), cap);
  for (size_t f = 0; f < F.tabs.size(); f++)
    for (uint64_t t = F.begin[f]; t < std::min<uint64_t>(F.begin[f + 1], limit); t++) {
      const uint32_t g = F.gets[t];
      dlsm_kv_handle h{0, 0, 0};
      const uint8_t st = f == 2 ? DLSM_GET_NOTFOUND : scan(F.tabs[f], F.keys[g], snap, static_cast<uint32_t>(f), &h);
      A.ts[t] = st;
      A.th[t] = h;
      if (st) {
        A.gs[g] = st;
        A.gh[g] = h;
      }
    }
  return A;
}

static void run_plan(TableIndex* ti, dlsm_ctx* ctx, const Fixture& F, uint64_t snap, uint64_t cap, int fault) {
  Arrays got(cap, F.keys.size());
  uint64_t fb0 = 0, fb1 = 0;
  dlsm_fallback_stats(ctx, &fb0, nullptr);
  if (fault) CHECK(dlsm_ctx_set_option(ctx, DLSM_OPT_FAULT_INJECT, fault) == DLSM_OK, "inject");
  const int st = ti->SeekPlan(F.ks, snap, F.begin.data(), F.gets.data(), cap, got.ts.data(), got.th.data(), got.gs.data(),
                              got.gh.data());
  if (fault) CHECK(dlsm_ctx_set_option(ctx, DLSM_OPT_FAULT_INJECT, 0) == DLSM_OK, "inject off");
  CHECK(st == DLSM_OK, "SeekPlan: %d", st);
  CHECK(ti->status() == (fault ? -fault : DLSM_OK), "device status %d", ti->status());
  dlsm_fallback_stats(ctx, &fb1, nullptr);
  CHECK(fb1 - fb0 == (fault ? 1u : 0u), "fallbacks %llu", (unsigned long long)(fb1 - fb0));
  CHECK(got == scan_plan(F, snap, cap), "arrays differ from the scan (snapshot %llu, cap %llu, fault %d)",
        (unsigned long long)snap, (unsigned long long)cap, fault);
}

static void test_host() {
  Fixture F;
  make_fixture(&F);
  const uint64_t snaps[] = {0, 1, 450, 899, (uint64_t(1) << 56) - 1};
  // IndexBlockSeek and TableIndex::Seek against the scan
  std::vector<uint8_t> status;
  TableIndex* ti = TableIndex::FromBlocks(F.slices, true, nullptr, &status);
  CHECK(ti && ti->n_files() == 4 && status == std::vector<uint8_t>(4, DLSM_BLOCK_OK), "FromBlocks");
  for (size_t f = 0; f < F.tabs.size(); f++)
    for (const std::string& k : targets(F.tabs[f == 2 ? 0 : f]))
      for (uint64_t snap : snaps) {
        dlsm_kv_handle want{0, 0, 0}, got{9, 9, 9}, got2{9, 9, 9};
        uint8_t st = 99, st2 = 99;
        uint8_t ws = DLSM_GET_NOTFOUND;  // file 2 is not held
        if (f != 2) ws = scan(F.tabs[f], k, snap, static_cast<uint32_t>(f), &want);
        CHECK(ti->Seek(static_cast<int>(f), Slice(k), snap, &st, &got) == DLSM_OK, "Seek");
        CHECK(st == ws && same(got, want), "Seek: file %zu state %d, scan %d", f, st, ws);
        if (f == 2) continue;
        CHECK(dlsm_adapter::host::IndexBlockSeek(F.contents[f], Slice(k), snap, &st2, &got2, static_cast<uint32_t>(f)) ==
                  DLSM_OK,
              "IndexBlockSeek");
        CHECK(st2 == ws && same(got2, want), "IndexBlockSeek: state %d, scan %d", st2, ws);
      }
  uint8_t st = 0;
  CHECK(ti->Seek(4, Slice("k", 1), 1, &st, nullptr) == DLSM_E_ARG && ti->Seek(-1, Slice("k", 1), 1, &st, nullptr) == DLSM_E_ARG,
        "file out of range");
  // host::SeekPlan against the scan, at several capacities
  for (uint64_t cap : {F.begin.back() + 5, F.begin.back(), F.begin.back() - 1, uint64_t(1), uint64_t(0)})
    for (uint64_t snap : snaps) {
      Arrays got(cap, F.keys.size());
      CHECK(dlsm_adapter::host::SeekPlan(F.contents, F.ks, snap, F.begin.data(), F.gets.data(), cap, got.ts.data(),
                                         got.th.data(), got.gs.data(), got.gh.data()) == DLSM_OK,
            "host SeekPlan");
      CHECK(got == scan_plan(F, snap, cap), "host SeekPlan differs from the scan");
    }
  delete ti;
  // FromBlocks' status codes, in the caller's order
  {
    std::string crc = F.blocks[0], typ = F.blocks[1], bad = write_contents(F.tabs[1]);
    crc[crc.size() / 2] ^= 1;
    typ[typ.size() - 5] = 1;  // the type byte, under a crc that covers it
    dlsm_adapter::host::PutFixed32(&typ[typ.size() - 4], dlsm_crc32c_mask(dlsm_crc32c_extend(0, typ.data(), typ.size() - 4)));
    bad[0] = 1;  // shared != 0
    const std::string short_block = "abc", bad_block = sealed(bad);
    const std::vector<Slice> bl = {Slice(crc), Slice(F.blocks[0]), Slice(short_block), Slice(nullptr, 0), Slice(typ),
                                   Slice(bad_block)};
    CHECK(TableIndex::FromBlocks(bl, true, nullptr, &status) == nullptr, "bad blocks give no index");
    const std::vector<uint8_t> want = {DLSM_BLOCK_CHECKSUM, DLSM_BLOCK_OK, DLSM_BLOCK_SHORT, DLSM_BLOCK_OK, DLSM_BLOCK_TYPE,
                                       DLSM_BLOCK_INDEX};
    CHECK(status == want, "status codes");
    CHECK(TableIndex::FromBlocks(bl, false, nullptr, &status) == nullptr && status[0] != DLSM_BLOCK_CHECKSUM &&
              status[4] == DLSM_BLOCK_TYPE && status[5] == DLSM_BLOCK_INDEX,
          "without checksums the flipped byte is judged by the contents' rules alone");
  }
  // SeekPlan with whatever this machine has: on the device, or (no device, so
  // no thread context) in host::SeekPlan -- the arrays are the scan's either way
  {
    TableIndex* t2 = TableIndex::FromBlocks(F.slices, true);
    CHECK(t2 != nullptr, "FromBlocks");
    const uint64_t cap = F.begin.back();
    Arrays got(cap, F.keys.size());
    CHECK(t2->SeekPlan(F.ks, 450, F.begin.data(), F.gets.data(), cap, got.ts.data(), got.th.data(), got.gs.data(),
                       got.gh.data()) == DLSM_OK,
          "SeekPlan");
    CHECK(got == scan_plan(F, 450, cap), "SeekPlan differs from the scan (device status %d)", t2->status());
    CHECK(t2->SeekPlan(F.ks, 450, nullptr, F.gets.data(), cap, nullptr, nullptr, nullptr, nullptr) == DLSM_E_ARG,
          "bad arguments stay bad");
    delete t2;
  }
  // the C ABI's checks that need no device
  {
    dlsm_tableindex* h = reinterpret_cast<dlsm_tableindex*>(1);
    CHECK(dlsm_tableindex_create_blocks(nullptr, nullptr, nullptr, 1, 0, 1, nullptr, &h) == DLSM_E_ARG && h == nullptr,
          "NULL context");
    CHECK(dlsm_tableindex_destroy(nullptr) == DLSM_OK && dlsm_tableindex_size(nullptr, nullptr, nullptr, nullptr) == DLSM_E_ARG,
          "NULL index");
    CHECK(dlsm_index_seek_dev(nullptr, nullptr, &F.ks, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == DLSM_E_ARG,
          "seek NULL");
    uint64_t n = 7;
    CHECK(dlsm_index_block_check(reinterpret_cast<const uint8_t*>("\0\0\0"), 3, &n) == DLSM_E_CORRUPT && n == 0, "len < 4");
    CHECK(dlsm_index_block_seek(reinterpret_cast<const uint8_t*>("\0\0\0"), 3, nullptr, 0, 0, 0, &st, nullptr) == DLSM_E_CORRUPT,
          "seek in contents Block's ctor rejects");
    CHECK(dlsm_index_block_seek(nullptr, 0, nullptr, 0, uint64_t(1) << 56, 0, &st, nullptr) == DLSM_E_ARG, "snapshot");
  }
  printf("OK adapter index host\n");
}

// SeekPlan on the device against the scan, then with a fault injected on the
// context (every device call of the adapter returns it: the host answers).
static void test_gpu() {
  dlsm_ctx* ctx = nullptr;
  CHECK(dlsm_ctx_create(0, &ctx) == DLSM_OK, "context");
  Fixture F;
  make_fixture(&F);
  TableIndex* ti = TableIndex::FromBlocks(F.slices, true, ctx);
  CHECK(ti != nullptr, "FromBlocks");
  const uint64_t total = F.begin.back();
  for (uint64_t cap : {total + 3, total, total - 1, uint64_t(300)})
    for (uint64_t snap : {uint64_t(0), uint64_t(450), (uint64_t(1) << 56) - 1}) run_plan(ti, ctx, F, snap, cap, 0);
  run_plan(ti, ctx, F, 450, total, 4);
  run_plan(ti, ctx, F, 450, total, 0);  // the device path is back
  // a fault at the first call: the open itself is refused, the host still answers
  TableIndex* t2 = TableIndex::FromBlocks(F.slices, true, ctx);
  CHECK(t2 != nullptr, "FromBlocks");
  run_plan(t2, ctx, F, 899, total, 5);
  run_plan(t2, ctx, F, 899, total, 0);
  uint64_t fb = 9;
  dlsm_fallback_stats(ctx, &fb, nullptr);
  CHECK(fb == 2, "only the injected faults fell back: %llu", (unsigned long long)fb);
  delete t2;
  delete ti;
  dlsm_ctx_destroy(ctx);
  printf("OK adapter index gpu\n");
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "gpu") == 0) test_gpu();
  else test_host();
  return 0;
}
