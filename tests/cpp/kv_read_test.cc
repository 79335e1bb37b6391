// tests/cpp/kv_read_test.cc -- the value read on the CPU: the chunk lookup and
// the pair decision the kernels run (dlsm_amd/csrc/kv_read.h) against a linear
// scan, one pair per rejection reason; the copy's unit (kv_copy_unit) driven
// span by span with a staged window the way kv_copy_kernel drives it, against
// a plain concatenation, every value in an allocation of its own so that a
// sanitizer sees a read past a value; and the planner (dlsm::plan::plan_kv_read,
// plan_tabledata) against brute force.  The writer below restates
// TableBuilder_BACS::Add (table/table_builder_bacs.cpp:221-226) on its own.
// Prints "OK" on success; exits non-zero with a message otherwise.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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

static void put32(std::string& o, uint32_t v) { o.append(reinterpret_cast<const char*>(&v), 4); }
static std::string ikey(const std::string& user, uint64_t seq, uint8_t type) {
  std::string k = user;
  const uint64_t t = (seq << 8) | type;
  k.append(reinterpret_cast<const char*>(&t), 8);
  return k;
}
static std::string raw_pair(uint32_t ks, uint32_t vs, const std::string& key, const std::string& value) {
  std::string o;
  put32(o, ks);
  put32(o, vs);
  return o + key + value;
}
static std::string pair_of(const std::string& key, const std::string& value) {
  return raw_pair(static_cast<uint32_t>(key.size()), static_cast<uint32_t>(value.size()), key, value);
}

// ---- chunk lookup ---------------------------------------------------------------
static void lookup_cases() {
  std::mt19937_64 rng(1);
  for (int round = 0; round < 200; round++) {
    const uint32_t n = round < 3 ? round : 1 + rng() % 80;
    std::vector<uint64_t> len(n), end(n);
    uint64_t at = 0;
    for (uint32_t c = 0; c < n; c++) {
      len[c] = rng() % 4 == 0 ? 0 : rng() % 40;  // empty chunks too
      end[c] = at += len[c];
    }
    for (uint64_t off = 0; off <= at + 2; off++) {
      uint32_t want = 0;  // the linear scan: the first chunk with end > off
      while (want < n && end[want] <= off) want++;
      CHECK(kv_chunk_find(end.data(), n, off) == want, "round %d off %llu", round, (unsigned long long)off);
    }
    CHECK(kv_chunk_find(end.data(), n, ~uint64_t(0)) == n, "the largest offset");
  }
  // locate: chunks in allocations of their own, every (offset, size) against the scan
  std::vector<std::string> chunks = {std::string(40, 'a'), std::string(16, 'b'), std::string(), std::string(33, 'c')};
  std::vector<uint64_t> end;
  std::vector<const uint8_t*> base;
  uint64_t at = 0;
  for (auto& c : chunks) {
    end.push_back(at += c.size());
    base.push_back(reinterpret_cast<const uint8_t*>(c.data()));
  }
  const KvChunks f{end.data(), base.data(), 4};
  for (uint64_t off = 0; off <= at + 1; off++)
    for (uint32_t size = 0; size <= 60; size++) {
      const uint8_t* want = nullptr;
      uint64_t start = 0;
      for (uint32_t c = 0; c < 4 && size >= 16; c++) {
        if (off >= start && off < end[c] && off + size <= end[c]) want = base[c] + (off - start);
        start = end[c];
      }
      CHECK(kv_pair_locate(f, off, size) == want, "locate %llu %u", (unsigned long long)off, size);
    }
  CHECK(kv_pair_locate(f, ~uint64_t(0) - 3, 16) == nullptr && kv_pair_locate(f, 0, 0xffffffffu) == nullptr, "wide handles");
  CHECK(kv_pair_locate(KvChunks{nullptr, nullptr, 0}, 0, 16) == nullptr, "no data held");
}

// ---- the decision -----------------------------------------------------------------
static uint8_t decide(const std::string& p, uint32_t size, const std::string& user, std::string* value) {
  const uint8_t* v = nullptr;
  uint32_t vl = 0;
  // the pair in an allocation of exactly its bytes
  std::unique_ptr<uint8_t[]> mem(new uint8_t[p.size()]);
  memcpy(mem.get(), p.data(), p.size());
  const uint8_t st = kv_pair_decide(mem.get(), size, reinterpret_cast<const uint8_t*>(user.data()),
                                    static_cast<uint32_t>(user.size()), &v, &vl);
  CHECK((st == kGetFound) == (v != nullptr) && (st == kGetFound || vl == 0), "value only with FOUND");
  if (value) value->assign(reinterpret_cast<const char*>(v ? v : mem.get()), vl);
  return st;
}

static void decide_cases() {
  const std::string k = ikey("key", 7, 1);
  std::string v;
  CHECK(decide(pair_of(k, "value"), 8 + 11 + 5, "key", &v) == kGetFound && v == "value", "found");
  CHECK(decide(pair_of(k, ""), 8 + 11, "key", &v) == kGetFound && v.empty(), "found, empty value");
  CHECK(decide(pair_of(ikey("", 7, 1), ""), 16, "", &v) == kGetFound && v.empty(), "the least pair");
  CHECK(decide(pair_of(ikey("key", 7, 0), "gone"), 8 + 11 + 4, "key", &v) == kGetDeleted && v.empty(), "type 0");
  CHECK(decide(raw_pair(7, 9, "1234567", "123456789"), 24, "", nullptr) == kGetCorrupt, "key_size < 8");
  CHECK(decide(raw_pair(0, 8, "", "12345678"), 16, "", nullptr) == kGetCorrupt, "key_size 0");
  CHECK(decide(raw_pair(11, 6, k, "value"), 24, "key", nullptr) == kGetCorrupt, "lengths past the size");
  CHECK(decide(raw_pair(11, 4, k, "value"), 24, "key", nullptr) == kGetCorrupt, "lengths short of the size");
  CHECK(decide(raw_pair(9, 0xffffffffu, ikey("k", 7, 1), ""), 16, "k", nullptr) == kGetCorrupt, "a sum that wraps in 32 bits");
  CHECK(decide(raw_pair(0xfffffff8u, 16, k, ""), 16, "key", nullptr) == kGetCorrupt, "a key_size that wraps");
  CHECK(decide(pair_of(ikey("key", 7, 2), "v"), 8 + 11 + 1, "key", nullptr) == kGetCorrupt, "type byte 2");
  CHECK(decide(pair_of(ikey("key", 7, 255), "v"), 8 + 11 + 1, "key", nullptr) == kGetCorrupt, "type byte 255");
  CHECK(decide(pair_of(k, "v"), 8 + 11 + 1, "kez", nullptr) == kGetCorrupt, "user key differs");
  CHECK(decide(pair_of(k, "v"), 8 + 11 + 1, "ke", nullptr) == kGetCorrupt, "user key shorter");
  CHECK(decide(pair_of(k, "v"), 8 + 11 + 1, "keyy", nullptr) == kGetCorrupt, "user key longer");
  CHECK(decide(pair_of(k, "v"), 8 + 11 + 1, "", nullptr) == kGetCorrupt, "empty user key");
  // long keys take the 8-bytes-at-a-time compare
  const std::string lk(37, 'q');
  CHECK(decide(pair_of(ikey(lk, 1, 1), "x"), 8 + 45 + 1, lk, &v) == kGetFound && v == "x", "long key");
  CHECK(decide(pair_of(ikey(lk, 1, 1), "x"), 8 + 45 + 1, lk.substr(0, 36) + "r", nullptr) == kGetCorrupt, "long key differs");

  // kv_item_decide: the file rules in front
  std::string c0 = pair_of(k, "first") + pair_of(ikey("b", 1, 1), "second!"), c1 = pair_of(ikey("c", 2, 1), "third");
  const uint64_t end[2] = {c0.size(), c0.size() + c1.size()};
  const uint8_t* base[2] = {reinterpret_cast<const uint8_t*>(c0.data()), reinterpret_cast<const uint8_t*>(c1.data())};
  const uint32_t begin[4] = {0, 0, 2, 2};  // files 0 and 2 hold no data
  const KvTables T{begin, end, base, 3};
  auto item = [&](uint64_t off, uint32_t size, uint32_t file, const char* user, std::string* out) {
    const uint8_t* pv;
    uint32_t vl;
    const uint8_t st = kv_item_decide(T, KvHandle{off, size, file}, reinterpret_cast<const uint8_t*>(user),
                                      static_cast<uint32_t>(strlen(user)), &pv, &vl);
    if (out) out->assign(reinterpret_cast<const char*>(pv ? pv : base[0]), vl);
    return st;
  };
  const uint32_t s0 = 8 + 11 + 5, s1 = 8 + 9 + 7, s2 = 8 + 9 + 5;
  CHECK(item(0, s0, 1, "key", &v) == kGetFound && v == "first", "first pair");
  CHECK(item(s0, s1, 1, "b", &v) == kGetFound && v == "second!", "last pair of a chunk");
  CHECK(item(s0 + s1, s2, 1, "c", &v) == kGetFound && v == "third", "an offset equal to a chunk's end");
  CHECK(item(0, s0, 0, "key", nullptr) == kGetCorrupt && item(0, s0, 2, "key", nullptr) == kGetCorrupt, "no data held");
  CHECK(item(0, s0, 3, "key", nullptr) == kGetCorrupt && item(0, s0, 0xffffffffu, "key", nullptr) == kGetCorrupt, "file >= n_files");
  CHECK(item(s0 + s1 + s2, 16, 1, "c", nullptr) == kGetCorrupt, "past every chunk");
  CHECK(item(s0, s1 + 1, 1, "b", nullptr) == kGetCorrupt && item(s0 + 4, s1 + s2 - 4, 1, "b", nullptr) == kGetCorrupt, "a straddle");
  CHECK(item(0, 15, 1, "key", nullptr) == kGetCorrupt, "size < 16");
}

// ---- the copy ------------------------------------------------------------------------
// kv_copy_kernel's walk with `wgs` workgroups, spans of `span` bytes and a
// window of `window` items: the staging and the choice between the window and
// value_off are restated here; the unit is the kernel's own.
static void copy_walk(const std::vector<uint64_t>& off, const std::vector<uint64_t>& src, uint64_t values_cap,
                      uint8_t* values, uint32_t span, uint32_t window, uint32_t wgs, uint64_t* window_spans,
                      uint64_t* direct_spans) {
  const uint64_t m = off.size() - 1;
  if (m == 0) return;
  const uint64_t total = off[m], limit = std::min(total, values_cap);
  const uint64_t spans = (limit + span - 1) / span, per = (spans + wgs - 1) / wgs;
  std::vector<uint64_t> soff(window + 1), ssrc(window + 1);
  for (uint32_t w = 0; w < wgs; w++) {
    const uint64_t s0 = per * w, s1 = std::min(s0 + per, spans);
    if (s0 >= s1) continue;
    uint64_t first = kv_last_le(off.data(), m, s0 * span);
    for (uint64_t s = s0; s < s1; s++) {
      const uint64_t p0 = s * span, p1 = std::min<uint64_t>(p0 + span, limit);
      for (uint32_t j = 0; j <= window; j++) {
        const uint64_t idx = first + j;
        soff[j] = idx <= m ? off[idx] : ~uint64_t(0);
        ssrc[j] = (idx < m && soff[j] < p1) ? src[idx] : 0;  // (0: a use of an unstaged address faults)
      }
      const uint64_t last = soff[window];
      for (uint64_t u = p0; u < p1; u += 16) {
        if (last >= p1) kv_copy_unit(soff.data(), ssrc.data(), window, u, p1, values);
        else kv_copy_unit(off.data() + first, src.data() + first, m - first, u, p1, values);
      }
      (last >= p1 ? *window_spans : *direct_spans)++;
      if (s + 1 < s1)
        first = last > p1 ? first + kv_last_le(soff.data(), window, p1)
                          : first + kv_last_le(off.data() + first, m - first, p1);
    }
  }
}

static void copy_case(const std::vector<uint32_t>& lens, uint32_t seed, uint32_t span, uint32_t window, uint32_t wgs,
                      bool want_both) {
  std::mt19937 rng(seed);
  const uint64_t m = lens.size();
  std::vector<std::unique_ptr<uint8_t[]>> vals(m);  // a value in an allocation of exactly its bytes, at any alignment
  std::vector<uint64_t> off(m + 1, 0), src(m);
  std::string blob;
  for (uint64_t i = 0; i < m; i++) {
    vals[i].reset(new uint8_t[lens[i] ? lens[i] : 1]);
    for (uint32_t j = 0; j < lens[i]; j++) vals[i][j] = static_cast<uint8_t>(rng());
    blob.append(reinterpret_cast<const char*>(vals[i].get()), lens[i]);
    src[i] = lens[i] ? reinterpret_cast<uint64_t>(vals[i].get()) : 0;
    off[i + 1] = off[i] + lens[i];
  }
  const uint64_t total = off[m];
  std::vector<uint64_t> caps = {total, total + 100, 0};
  if (total) caps.insert(caps.end(), {total - 1, total / 2, total / 3 | 1, std::min<uint64_t>(total, 16), std::min<uint64_t>(total, 17)});
  uint64_t ws = 0, ds = 0;
  for (uint64_t cap : caps) {
    const uint64_t room = std::max(total, cap) + 64;
    uint8_t* out = static_cast<uint8_t*>(aligned_alloc(16, (room + 15) & ~uint64_t(15)));
    memset(out, 0xCD, room);
    copy_walk(off, src, cap, out, span, window, wgs, &ws, &ds);
    const uint64_t k = std::min(total, cap);
    CHECK(memcmp(out, blob.data(), k) == 0, "bytes differ: seed %u cap %llu", seed, (unsigned long long)cap);
    for (uint64_t p = k; p < room; p++) CHECK(out[p] == 0xCD, "byte %llu written, cap %llu total %llu", (unsigned long long)p,
                                              (unsigned long long)cap, (unsigned long long)total);
    free(out);
  }
  if (want_both) CHECK(ws > 0 && ds > 0, "both the window and the direct search ran (%llu, %llu)", (unsigned long long)ws, (unsigned long long)ds);
}

static void copy_cases() {
  std::mt19937 rng(9);
  const uint32_t S = kKvSpan;
  {  // every pair of (destination residue, source residue), around the unit and the span
    std::vector<uint32_t> lens;
    const uint32_t base[] = {0, 1, 15, 16, 17, 31, 32, 33, 64 - 1, 64, 64 + 1, 3 * 64 + 5};
    for (int r = 0; r < 16; r++) {
      for (uint32_t l : base) lens.push_back(l);
      lens.push_back(1);
    }
    copy_case(lens, 1, 64, 7, 3, true);
    copy_case(lens, 2, 64, 1, 5, true);
    copy_case(lens, 3, 16, 3, 2, true);
    copy_case(lens, 4, S, kKvWindow, kKvCopyWgs, false);
  }
  {  // empty and 1-byte runs longer than the window, between non-empty values
    std::vector<uint32_t> lens = {40};
    lens.insert(lens.end(), 300, 0);
    lens.push_back(25);
    lens.insert(lens.end(), 200, 1);
    lens.insert(lens.end(), {0, 0, 7});
    copy_case(lens, 5, 64, 15, 4, true);
    copy_case(lens, 6, 32, 31, 1, true);
    copy_case(std::vector<uint32_t>(500, 0), 7, 64, 15, 4, false);  // a total of 0
    copy_case({}, 8, 64, 15, 4, false);
    copy_case({5}, 8, 64, 15, 4, false);
    copy_case({0}, 8, 64, 15, 4, false);
  }
  {  // the real span and window: 1-byte values that overflow the window, a value of several spans
    std::vector<uint32_t> lens = {100};
    lens.insert(lens.end(), 2 * S, 1);
    lens.insert(lens.end(), 3000, 0);
    lens.insert(lens.end(), {3 * S + 5, 400, 0, 436, S - 1, S, S + 1, 9});
    copy_case(lens, 10, S, kKvWindow, kKvCopyWgs, true);
    copy_case(lens, 11, S, kKvWindow, 3, true);
  }
  for (uint32_t seed = 20; seed < 60; seed++) {  // random lengths, skewed
    std::vector<uint32_t> lens(rng() % 400);
    for (auto& l : lens) l = rng() % 5 == 0 ? 0 : (rng() % 7 == 0 ? rng() % 700 : rng() % 20);
    const uint32_t span = 16u << (rng() % 5), window = 1 + rng() % 40, wgs = 1 + rng() % 9;
    copy_case(lens, seed, span, window, wgs, false);
  }
}

// ---- the planner ------------------------------------------------------------------
static void planner_cases() {
  for (uint64_t cap : {uint64_t(0), uint64_t(1), uint64_t(kKvChunk - 1), uint64_t(kKvChunk), uint64_t(kKvChunk + 1),
                       uint64_t(3 * kKvChunk + 17), uint64_t(512) * kKvChunk, uint64_t(512) * kKvChunk + 3,
                       uint64_t(1000) * kKvChunk + 1, uint64_t(10'000'000), uint64_t(0xffffffffu)}) {
    KvReadPlan P;
    CHECK(plan_kv_read(cap, kSortMaxWgs, kKvCopyWgs, P) == DLSM_OK, "plan %llu", (unsigned long long)cap);
    // brute force: the fewest chunks per workgroup that fit kSortMaxWgs workgroups
    const uint64_t chunks = (cap + kKvChunk - 1) / kKvChunk;
    uint64_t cpw = 1;
    while (cpw * kSortMaxWgs < chunks) cpw++;
    CHECK(P.chunks == chunks && P.cpw == cpw && P.nwg <= kSortMaxWgs, "grid of %llu", (unsigned long long)cap);
    CHECK(uint64_t(P.nwg) * P.cpw >= chunks && (P.nwg == 0 || uint64_t(P.nwg - 1) * P.cpw < chunks), "every chunk once, no idle workgroup");
    CHECK((cap == 0) == (P.nwg == 0) && P.copy_wgs == kKvCopyWgs, "nothing to do only at 0");
    const uint64_t o[5] = {P.len_off, P.src_off, P.sum_off, P.bad_off, P.bytes};
    const uint64_t b[4] = {4 * cap, 8 * cap, 8ull * P.nwg, 8ull * P.nwg};
    CHECK(o[0] == 0, "starts at 0");
    for (int r = 0; r < 4; r++) {
      CHECK(o[r] % 256 == 0 && o[r] + b[r] <= o[r + 1] && o[r + 1] - (o[r] + b[r]) < 256, "region %d of %llu", r, (unsigned long long)cap);
    }
    CHECK(P.len_bytes == b[0] && P.src_bytes == b[1] && P.sum_bytes == b[2] && P.bad_bytes == b[3], "sizes");
    CHECK(P.bytes <= 12 * cap + 4 * 256 + 16ull * kSortMaxWgs, "12 bytes per item and the partial sums");
  }
  KvReadPlan P;
  CHECK(plan_kv_read(uint64_t(1) << 32, kSortMaxWgs, kKvCopyWgs, P) == DLSM_E_ARG, "cap past 32 bits");
  CHECK(plan_kv_copy_wgs(256) == 512 && plan_kv_copy_wgs(64) == 128 && plan_kv_copy_wgs(0) == 2 &&
            plan_kv_copy_wgs(kKvCopyWgs / kKvCopyWgsPerCu) == kKvCopyWgs,
        "two workgroups per compute unit");
  CHECK(plan_kv_read(5, 0, 1, P) == DLSM_E_ARG && plan_kv_read(5, 1, 0, P) == DLSM_E_ARG, "grids of 0");

  uint8_t mem[8];
  const dlsm_data_chunk ch[5] = {{mem, 40}, {mem, 0}, {mem, 17}, {mem, 33}, {nullptr, 0}};
  const uint32_t begin[5] = {0, 3, 3, 4, 5};
  TableDataPlan T;
  CHECK(plan_tabledata(ch, begin, 4, T) == DLSM_OK, "tables");
  CHECK(T.end == (std::vector<uint64_t>{40, 40, 57, 33, 0}), "running ends per file");
  CHECK(T.arena_off == (std::vector<uint64_t>{0, 48, 48, 80, 128}) && T.arena_bytes == 128 && T.data_bytes == 90, "arena");
  const uint32_t down[3] = {0, 2, 1}, late[2] = {1, 2};
  const dlsm_data_chunk null_base[1] = {{nullptr, 4}};
  const uint32_t one[2] = {0, 1};
  const dlsm_data_chunk wrap[2] = {{mem, ~uint64_t(0)}, {mem, 2}};
  const uint32_t two[2] = {0, 2};
  CHECK(plan_tabledata(ch, down, 2, T) == DLSM_E_ARG && plan_tabledata(ch, late, 1, T) == DLSM_E_ARG, "chunk_begin");
  CHECK(plan_tabledata(null_base, one, 1, T) == DLSM_E_ARG && plan_tabledata(wrap, two, 1, T) == DLSM_E_ARG, "chunks");
  CHECK(plan_tabledata(nullptr, one, 1, T) == DLSM_E_ARG && plan_tabledata(ch, nullptr, 0, T) == DLSM_E_ARG, "null");
  const uint32_t none[1] = {0};
  CHECK(plan_tabledata(nullptr, none, 0, T) == DLSM_OK && T.end.empty(), "no files");
}

int main() {
  lookup_cases();
  decide_cases();
  copy_cases();
  planner_cases();
  printf("OK kv read\n");
  return 0;
}
