// tests/cpp/host_plan_test.cc -- the C ABI's host-side planning
// (dlsm_amd/csrc/host_plan.h) on the CPU.  Every expected value is brute
// force written from the comments in the code, not a second planner.
// Prints "OK" on success; exits non-zero with a message otherwise.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>

#include "../../dlsm_amd/csrc/host_plan.h"

using namespace dlsm;
using namespace dlsm::plan;
typedef unsigned __int128 u128;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                \
      printf("\n");                                       \
      exit(1);                                            \
    }                                                     \
  } while (0)

static u128 to128(const ulonglong2& p) { return (static_cast<u128>(p.x) << 64) | p.y; }
// the first 16 bytes of a key, zero-padded, big-endian
static u128 prefix_of(const std::string& k) {
  u128 r = 0;
  for (size_t i = 0; i < 16; i++) r = (r << 8) | (i < k.size() ? static_cast<uint8_t>(k[i]) : 0);
  return r;
}

// ---- version index -----------------------------------------------------------
struct VFiles {
  std::vector<std::string> keys;  // 2 per file: smallest, largest (stable storage)
  std::vector<dlsm_version_file> files;
  void add(int level, const std::string& lo, const std::string& hi, uint64_t number) {
    keys.push_back(lo);
    keys.push_back(hi);
    dlsm_version_file F{};
    F.level = level;
    F.number = number;
    F.largest_trailer = number * 256 + 1;
    files.push_back(F);
  }
  void seal() {
    for (size_t f = 0; f < files.size(); f++) {
      files[f].smallest_user_key = reinterpret_cast<const uint8_t*>(keys[2 * f].data());
      files[f].smallest_len = keys[2 * f].size();
      files[f].largest_user_key = reinterpret_cast<const uint8_t*>(keys[2 * f + 1].data());
      files[f].largest_len = keys[2 * f + 1].size();
    }
  }
};

static std::string random_key(std::mt19937& rng, const std::string& prev) {
  static const char alpha[3] = {0x10, 0x40, 0x70};
  std::string k;
  // a third of the keys extend the previous key's 16-byte prefix: equal prefixes, distinct keys
  if (prev.size() >= 16 && rng() % 3 == 0) k = prev.substr(0, 16);
  const size_t len = k.empty() ? rng() % 25 : 17 + rng() % 8;
  while (k.size() < len) k.push_back(alpha[rng() % 3]);
  return k;
}

// A witness strictly inside interval j of bnd (below bnd[0], between two
// bounds, above the last); false when the interval holds no 128-bit value.
static bool witness(const std::vector<ulonglong2>& bnd, uint32_t j, u128* w) {
  const uint32_t n = static_cast<uint32_t>(bnd.size());
  if (n == 0) return *w = 12345, true;
  if (j == 0) {
    const u128 hi = to128(bnd[0]);
    if (hi == 0) return false;
    return *w = hi / 2, true;
  }
  const u128 lo = to128(bnd[j - 1]);
  if (j == n) return *w = lo + 1, lo + 1 > lo;
  const u128 hi = to128(bnd[j]);
  if (hi - lo < 2) return false;
  return *w = lo + (hi - lo) / 2, true;
}

// Interval j of the plan against a scan of the files with witness w.
static void check_interval(const VersionPlan& P, int n_files, uint32_t j, u128 w, const char* what) {
  const VIntervalDev& r = P.ivl[j];
  auto small = [&](uint32_t f) { return to128(P.pre[f]); };
  auto large = [&](uint32_t f) { return to128(P.pre[n_files + f]); };
  uint64_t mask = 0;
  for (int f = 0; f < P.n_l0; f++)
    if (small(f) < w && w < large(f)) mask |= 1ull << f;
  CHECK(r.l0mask == mask, "%s interval %u", what, j);
  for (int lv = 1; lv < kNumLevels; lv++) {
    uint16_t want = 0xffffu;
    const uint32_t b = P.begin[lv], c = P.count[lv];
    if (c && b + c <= 0xffffu) {
      uint32_t q = c - 1;
      for (uint32_t t = 0; t + 1 < c; t++)
        if (large(b + t) > w) {
          q = t;
          break;
        }
      if (small(b + q) < w) want = static_cast<uint16_t>(b + q);  // the pick is a search-order index
    }
    CHECK(r.pick[lv - 1] == want, "%s interval %u level %d: %u want %u", what, j, lv, r.pick[lv - 1], want);
  }
  CHECK(r.reserved[0] == 0 && r.reserved[1] == 0 && r.reserved[2] == 0, "%s interval %u", what, j);
}

static void check_bounds(const VersionPlan& P, const char* what) {
  for (size_t j = 1; j < P.bnd.size(); j++) CHECK(to128(P.bnd[j - 1]) < to128(P.bnd[j]), "%s bnd %zu", what, j);
  CHECK(P.ivl.size() == P.bnd.size() + 1, "%s", what);
}

static void test_version_index() {
  bool saw_empty_key = false, saw_point_file = false, saw_prefix_tie = false;
  for (int seed = 0; seed < 20; seed++) {
    std::mt19937 rng(seed);
    VFiles V;
    const int n0 = rng() % 9;
    for (int f = 0; f < n0; f++) {
      std::string a = random_key(rng, ""), b = random_key(rng, a);
      if (b < a) std::swap(a, b);
      V.add(0, a, b, rng() % 4);  // few distinct numbers: the sort must be stable
    }
    for (int lv = 1; lv <= 5; lv++) {
      const int cnt = rng() % 41;
      std::set<std::string> pool;
      std::string prev;
      for (int i = 0; i < 3 * cnt; i++) pool.insert(prev = random_key(rng, prev));
      std::vector<std::string> d(pool.begin(), pool.end());  // sorted bytewise (char_traits: unsigned)
      size_t p = 0;
      for (int f = 0; f < cnt && p < d.size(); f++) {
        const bool point = rng() % 4 == 0 || p + 1 == d.size();
        V.add(lv, d[p], d[point ? p : p + 1], 100 + f);
        saw_point_file = saw_point_file || point;
        p += point ? 1 : 2;
      }
    }
    V.seal();
    for (const std::string& k : V.keys) saw_empty_key = saw_empty_key || k.empty();
    const int n = static_cast<int>(V.files.size());
    VersionPlan P;
    CHECK(plan_version(V.files.data(), n, nullptr, false, 0, P) == DLSM_OK, "seed %d", seed);
    check_bounds(P, "seed");
    // level 0: by file number, descending, stable; levels >= 1 in the caller's order
    CHECK(P.n_l0 == n0, "seed %d", seed);
    for (int i = 0; i + 1 < n0; i++) {
      const dlsm_version_file &A = V.files[P.order[i]], &B = V.files[P.order[i + 1]];
      CHECK(A.number > B.number || (A.number == B.number && P.order[i] < P.order[i + 1]), "seed %d l0 %d", seed, i);
    }
    for (int lv = 1; lv < kNumLevels; lv++)
      for (uint32_t i = 0; i < P.count[lv]; i++) {
        CHECK(V.files[P.order[P.begin[lv] + i]].level == lv, "seed %d", seed);
        if (i) CHECK(P.order[P.begin[lv] + i - 1] < P.order[P.begin[lv] + i], "seed %d", seed);
      }
    for (int j = 0; j < n; j++) {
      CHECK(to128(P.pre[j]) == prefix_of(V.keys[2 * P.order[j]]), "seed %d file %d", seed, j);
      CHECK(to128(P.pre[n + j]) == prefix_of(V.keys[2 * P.order[j] + 1]), "seed %d file %d", seed, j);
      if (j && V.keys[2 * P.order[j]].size() > 16 && P.pre[j].x == P.pre[n + j - 1].x && P.pre[j].y == P.pre[n + j - 1].y)
        saw_prefix_tie = true;
    }
    // Every interval has a witness: no two distinct prefixes of this alphabet
    // are adjacent integers.  The one exception is by construction empty, not
    // skipped: nothing lies below bnd[0] == 0, the zero-length key's prefix.
    int skipped = 0;
    for (uint32_t j = 0; j <= P.bnd.size(); j++) {
      u128 w;
      if (!witness(P.bnd, j, &w)) {
        if (!(j == 0 && to128(P.bnd[0]) == 0)) skipped++;
        continue;
      }
      check_interval(P, n, j, w, "seed");
    }
    CHECK(skipped == 0, "seed %d: %d intervals without witness", seed, skipped);
  }
  CHECK(saw_empty_key && saw_point_file && saw_prefix_tie, "coverage %d %d %d", saw_empty_key, saw_point_file,
        saw_prefix_tie);
}

// key i of a sorted family: 11 base-3 digits of i over the alphabet
static std::string digit_key(uint32_t i) {
  static const char alpha[3] = {0x10, 0x40, 0x70};
  std::string k(11, 0);
  for (int d = 10; d >= 0; d--, i /= 3) k[d] = alpha[i % 3];
  return k;
}

static void test_version_large() {
  {  // one level of 60,000 files, 2,000 evenly spaced intervals
    VFiles V;
    const uint32_t n = 60000;
    for (uint32_t f = 0; f < n; f++) V.add(2, digit_key(2 * f), digit_key(2 * f + 1), f);
    V.seal();
    VersionPlan P;
    CHECK(plan_version(V.files.data(), n, nullptr, false, 0, P) == DLSM_OK, "60k");
    check_bounds(P, "60k");
    CHECK(P.bnd.size() == 2 * n, "60k");
    for (uint32_t q = 0; q < 2000; q++) {
      const uint32_t j = static_cast<uint32_t>(static_cast<uint64_t>(q) * P.bnd.size() / 1999);
      u128 w;
      CHECK(witness(P.bnd, j, &w), "60k interval %u", j);
      check_interval(P, n, j, w, "60k");
    }
  }
  {  // a level whose files end past search-order index 65,535 is never picked
    VFiles V;
    for (uint32_t f = 0; f < 100; f++) V.add(1, digit_key(2 * f), digit_key(2 * f + 1), f);
    for (uint32_t f = 0; f < 65500; f++) V.add(2, digit_key(2 * f), digit_key(2 * f + 1), f);
    V.seal();
    const int n = static_cast<int>(V.files.size());
    VersionPlan P;
    CHECK(plan_version(V.files.data(), n, nullptr, false, 0, P) == DLSM_OK, "65k");
    CHECK(P.begin[2] + P.count[2] > 65535u, "65k");
    for (size_t j = 0; j < P.ivl.size(); j++) CHECK(P.ivl[j].pick[1] == 0xffffu, "65k interval %zu", j);
    for (uint32_t j = 0; j <= P.bnd.size(); j += 97) {
      u128 w;
      CHECK(witness(P.bnd, j, &w), "65k interval %u", j);
      check_interval(P, n, j, w, "65k");  // level 1 is still picked
    }
  }
}

// ---- version layout ----------------------------------------------------------
struct Filt {
  int level, k;
  uint32_t L;
  bool lg0;  // a tail the reader takes with log2_cache_line_size_ 0
};

static int layout_plan(const std::vector<Filt>& fl, bool have_tails, uint64_t min_bytes, VersionPlan& P,
                       VFiles& V) {
  static const uint8_t dummy = 0;
  std::vector<uint8_t> tails;
  for (size_t f = 0; f < fl.size(); f++) {
    V.add(fl[f].level, digit_key(2 * f), digit_key(2 * f + 1), f);
    dlsm_version_file& F = V.files.back();
    const uint32_t L = fl[f].L;
    if (fl[f].k) {
      F.filter = &dummy;  // never read: the planner sees the tails only
      F.filter_len = fl[f].lg0 ? 128 * uint64_t(L) + 5 : 64 * uint64_t(L) + 5;
    }
    const uint8_t t[5] = {uint8_t(fl[f].k), uint8_t(L), uint8_t(L >> 8), uint8_t(L >> 16), uint8_t(L >> 24)};
    tails.insert(tails.end(), t, t + 5);
  }
  V.seal();
  return plan_version(V.files.data(), static_cast<int>(fl.size()), tails.data(), have_tails, min_bytes, P);
}

static void check_extents(const VersionPlan& P, const VFiles& V, const char* what) {
  const size_t n = V.files.size();
  std::vector<std::pair<uint64_t, uint64_t>> ext;  // [begin, end)
  const uint64_t sect[5] = {sizeof(VFileDev) * n, sizeof(ulonglong2) * P.pre.size(), P.keys.size(),
                            sizeof(ulonglong2) * P.bnd.size(), sizeof(VIntervalDev) * P.ivl.size()};
  const uint64_t padded[5] = {P.files_bytes, P.pre_bytes, P.keys_bytes, P.bnd_bytes, P.ivl_bytes};
  uint64_t at = 0;
  for (int q = 0; q < 5; q++) {
    CHECK(padded[q] % 256 == 0 && padded[q] >= sect[q], "%s section %d", what, q);
    ext.push_back({at, at + sect[q]});
    at += padded[q];
  }
  for (size_t j = 0; j < n; j++) {
    const dlsm_version_file& F = V.files[P.order[j]];
    if (!F.filter) continue;
    const int q = P.lvl_sliced[F.level];
    if (q < 0) {
      CHECK(P.foff[j] % 256 == 0 && P.copy_len[j] == F.filter_len, "%s file %zu", what, j);
    } else {  // a sliced level's filters lie line to line inside its 256-byte aligned image
      CHECK(P.image_off[q] % 256 == 0, "%s", what);
      CHECK(P.foff[j] == P.image_off[q] + 64ull * P.h[j].line0, "%s file %zu", what, j);
      CHECK(P.copy_len[j] == 64ull * P.h[j].f.L, "%s file %zu", what, j);
    }
    ext.push_back({P.foff[j], P.foff[j] + P.copy_len[j]});
  }
  std::sort(ext.begin(), ext.end());
  for (size_t i = 0; i < ext.size(); i++) {
    CHECK(ext[i].second <= P.total, "%s extent %zu", what, i);
    if (i) CHECK(ext[i - 1].second <= ext[i].first, "%s extents %zu overlap", what, i);
  }
}

static void test_version_layout() {
  // level 1: three small filters; level 3: big ones around a table without a filter
  const std::vector<Filt> base = {{0, 6, 3, false},   {1, 6, 5, false},   {1, 6, 7, false}, {1, 6, 1, false},
                                  {3, 6, 100, false}, {3, 0, 0, false},   {3, 6, 37, false}, {3, 6, 250, false},
                                  {4, 6, 2, false}};
  const uint64_t min_bytes = 64 * 100;  // only level 3 (387 lines) holds more
  {
    VersionPlan P;
    VFiles V;
    CHECK(layout_plan(base, true, min_bytes, P, V) == DLSM_OK, "layout");
    check_extents(P, V, "sliced");
    CHECK(P.sliced.size() == 1 && P.sliced[0].level == 3 && P.sliced[0].k == 6 && P.sliced[0].lines == 387, "layout");
    for (int lv = 0; lv < kNumLevels; lv++) CHECK(P.lvl_sliced[lv] == (lv == 3 ? 0 : -1), "level %d", lv);
    uint32_t line0 = 0;
    bool first = true;
    for (uint32_t j = P.begin[3]; j < P.begin[3] + P.count[3]; j++) {
      if (!V.files[P.order[j]].filter) continue;
      CHECK(P.h[j].line0 == line0 && P.copy_len[j] == 64ull * P.h[j].f.L, "file %u", j);
      if (first) CHECK(P.image_off[0] == P.foff[j], "image_off");
      first = false;
      line0 += P.h[j].f.L;
    }
    CHECK(line0 == 387 && P.k_all == 6, "layout");
    for (size_t j = 0; j < base.size(); j++) {
      const Filt& f = base[P.order[j]];
      CHECK(P.h[j].f.k == f.k && P.h[j].f.L == f.L && P.h[j].f.data == nullptr, "file %zu", j);
      if (f.k) CHECK(P.h[j].f.lg == 6 && P.h[j].f.magic == fastmod_magic(f.L), "file %zu", j);
    }
  }
  {  // mixed probe counts: not sliced, and k_all is 0
    std::vector<Filt> fl = base;
    fl[6].k = 7;
    VersionPlan P;
    VFiles V;
    CHECK(layout_plan(fl, true, min_bytes, P, V) == DLSM_OK, "mixed k");
    CHECK(P.sliced.empty() && P.lvl_sliced[3] == -1 && P.k_all == 0, "mixed k");
    check_extents(P, V, "mixed k");
  }
  {  // a filter with lg != 6: not sliced
    std::vector<Filt> fl = base;
    fl[6].lg0 = true;
    VersionPlan P;
    VFiles V;
    CHECK(layout_plan(fl, true, min_bytes, P, V) == DLSM_OK, "lg 0");
    CHECK(P.sliced.empty() && P.lvl_sliced[3] == -1, "lg 0");
    int lg0 = 0;
    for (const VFileDev& d : P.h) lg0 += d.f.L && d.f.lg == 0;
    CHECK(lg0 == 1, "lg 0");
    check_extents(P, V, "lg 0");
  }
  {  // sealed blocks: no tails, nothing parsed, nothing sliced
    VersionPlan P;
    VFiles V;
    CHECK(layout_plan(base, false, min_bytes, P, V) == DLSM_OK, "no tails");
    CHECK(P.sliced.empty() && P.k_all == 0, "no tails");
    for (int lv = 0; lv < kNumLevels; lv++) CHECK(P.lvl_sliced[lv] == -1, "no tails");
    for (const VFileDev& d : P.h) CHECK(d.f.L == 0 && d.f.k == 0 && d.line0 == 0, "no tails");
    check_extents(P, V, "no tails");
  }
  {  // min_slice_bytes 0: nothing sliced
    VersionPlan P;
    VFiles V;
    CHECK(layout_plan(base, true, 0, P, V) == DLSM_OK && P.sliced.empty(), "min 0");
  }
  {  // the argument checks and the tail's codes
    std::vector<Filt> fl = base;
    fl[2].level = 6;
    VersionPlan P;
    VFiles V;
    CHECK(layout_plan(fl, true, 0, P, V) == DLSM_E_ARG, "level");
    fl = base;
    fl[2].k = -3;  // FullFilterBlockReader: num_probes < 1
    VersionPlan P2;
    VFiles V2;
    CHECK(layout_plan(fl, true, 0, P2, V2) == DLSM_E_CORRUPT, "k < 1");
    fl.assign(60, Filt{0, 6, 1, false});  // 60 level-0 files leave no slot for levels 1..5
    VersionPlan P3;
    VFiles V3;
    CHECK(layout_plan(fl, true, 0, P3, V3) == DLSM_E_ARG, "n_l0");
  }
}

// ---- probe groups ------------------------------------------------------------
static void test_filter_groups() {
  const uint32_t Ls[3] = {100, 101, 3005};
  const int ks[2] = {6, 7};
  for (int F : {1, 2, 7, 8, 9, 16, 17, 64})
    for (int seed = 0; seed < 6; seed++) {
      std::mt19937 rng(1000 * F + seed);
      std::vector<FilterDev> h(F);
      for (FilterDev& f : h) {
        f = FilterDev{nullptr, Ls[rng() % 3], 0, ks[rng() % 2], 6};
        f.magic = fastmod_magic(f.L);
      }
      const FilterGroupPlan P = plan_filter_groups(h, true);
      CHECK(P.groups.size() == P.members.size() && !P.groups.empty(), "F %d", F);
      std::vector<int> seen(F, 0);
      std::set<int> bytes_seen;
      for (size_t g = 0; g < P.groups.size(); g++) {
        const ProbeGroup& G = P.groups[g];
        const std::vector<int>& m = P.members[g];
        const int nm = static_cast<int>(m.size());
        CHECK(nm >= 1 && nm <= 8 && G.stacked == nullptr, "F %d group %zu", F, g);
        for (int f : m) {
          seen[f]++;
          CHECK(f / 8 == G.mask_byte && h[f].L == G.L && h[f].k == G.k, "F %d group %zu", F, g);
        }
        CHECK(G.magic == fastmod_magic(G.L), "F %d group %zu", F, g);
        CHECK(G.lgw == (nm == 1 ? 0 : nm == 2 ? 1 : nm <= 4 ? 2 : 3), "F %d group %zu: %d members", F, g, nm);
        for (int j = 0; j < nm && G.lgw < 3; j++)
          CHECK(((G.slotmap >> (4 * j)) & 15u) == static_cast<uint32_t>(m[j] % 8), "F %d group %zu", F, g);
        if (G.lgw == 3) CHECK(G.slotmap == 0, "F %d group %zu", F, g);
        CHECK(G.first_of_byte == bytes_seen.insert(G.mask_byte).second, "F %d group %zu", F, g);
      }
      for (int f = 0; f < F; f++) CHECK(seen[f] == 1, "F %d filter %d in %d groups", F, f, seen[f]);
      CHECK(static_cast<int>(bytes_seen.size()) == (F + 7) / 8, "F %d", F);
      const FilterGroupPlan U = plan_filter_groups(h, false);
      CHECK(U.members == P.members, "F %d", F);
      for (const ProbeGroup& G : U.groups) CHECK(G.lgw == 3 && G.slotmap == 0, "F %d unpacked", F);
      h[rng() % F].lg = 0;  // one filter outside the reader's common case: direct probe only
      CHECK(plan_filter_groups(h, true).groups.empty(), "F %d", F);
    }
}

// ---- one-pass layout -----------------------------------------------------------
static uint64_t image_word;  // any non-null image address: the planner never reads through it

static ProbeGroup group_of(uint32_t L, int lgw, int k, int mask_byte) {
  ProbeGroup g;
  g.stacked = &image_word;
  g.L = L;
  g.magic = L ? fastmod_magic(L) : 0;
  g.k = k;
  g.lgw = lgw;
  g.mask_byte = mask_byte;
  g.slotmap = lgw < 3 ? 0x3210u & ((1u << (4 << lgw)) - 1u) : 0;
  return g;
}

static void test_mg_layout() {
  constexpr uint32_t C = kMGChunk;
  for (int G : {2, 3, 12, 16})
    for (int seed = 0; seed < 4; seed++) {
      std::mt19937 rng(77 * G + seed);
      std::vector<ProbeGroup> gs;
      for (int j = 0; j < G; j++) {
        const int lgw = (j + seed) % 4;
        const uint32_t R = 1u << (11 - lgw);
        // 1..40 slices, the last one partial; widths 0 and 1 keep k = 6 in even seeds
        const uint32_t L = (1 + rng() % 40) * R - rng() % R;
        gs.push_back(group_of(L, lgw, (seed % 2 == 0 && lgw < 2) || rng() % 2 ? 6 : 7, j / 3));
      }
      const MGLayout M = plan_mg_layout(gs, 256);
      CHECK(M.ok && static_cast<int>(M.md.size()) == G, "G %d", G);
      // ordered by width, stable: the input indices with lgw = 0, then 1, ...
      std::vector<int> order;
      for (int w = 0; w < 4; w++)
        for (int j = 0; j < G; j++)
          if (gs[j].lgw == w) order.push_back(j);
      uint32_t sbase = 0, eoff = 0, aoff = 0, stage = 0, pair = 0;
      for (int j = 0; j < G; j++) {
        const ProbeGroup& g = gs[order[j]];
        const MGroupDev& d = M.md[j];
        const uint32_t R = 1u << (11 - g.lgw), S = (g.L + R - 1) / R;
        CHECK(d.image == reinterpret_cast<const uint8_t*>(g.stacked) && d.L == g.L && d.magic == g.magic &&
                  d.k == g.k && d.lgw == g.lgw && d.mask_byte == g.mask_byte && d.slotmap == g.slotmap,
              "G %d group %d", G, j);
        CHECK(d.R == R && d.rmagic == fastmod_magic(R) && d.S == S && d.reserved == 0, "G %d group %d", G, j);
        CHECK(d.sbase == sbase && d.tcol == sbase + j && d.eoff == eoff && d.aoff == aoff, "G %d group %d", G, j);
        sbase += S;
        eoff += mg_sub_entries(C, S);
        aoff += mg_sub_abytes(C, S, g.lgw);
        pair = (j % 2 ? pair : 0) + 4u * mg_sub_entries(C, S);  // sets of kMGSetSize = 2 groups
        stage = std::max(stage, pair);
      }
      static_assert(kMGSetSize == 2, "the staging sets are pairs");
      CHECK(M.slices == sbase && M.region == eoff && M.abytes == aoff && M.stage_bytes == stage, "G %d", G);
      // the classes: one per width present, in order, covering every slice
      uint32_t s0 = 0;
      int j = 0;
      for (const MGClass& cl : M.classes) {
        CHECK(j < G && cl.lgw == M.md[j].lgw && cl.s0 == s0, "G %d class", G);
        bool all6 = true;
        std::vector<double> share;
        for (; j < G && M.md[j].lgw == cl.lgw; j++) {
          all6 = all6 && M.md[j].k == 6;
          for (uint32_t t = 0; t < M.md[j].S; t++)
            share.push_back(static_cast<double>(std::min(M.md[j].R, M.md[j].L - t * M.md[j].R)) / M.md[j].L);
        }
        CHECK(cl.S == share.size() && cl.K == (all6 ? 6 : 0), "G %d class lgw %d", G, cl.lgw);
        const uint32_t* plan = M.plan.data() + cl.plan_off;
        CHECK(cl.plan_off + cl.S + 1 <= M.plan.size() && plan[0] == 0 && plan[cl.S] == cl.wgs, "G %d class", G);
        for (uint32_t t = 0; t < cl.S; t++) CHECK(plan[t] < plan[t + 1], "G %d class lgw %d slice %u", G, cl.lgw, t);
        CHECK(cl.wgs >= std::max(256u, cl.S), "G %d class lgw %d: %u", G, cl.lgw, cl.wgs);
        double W = 0, least = 1e30;
        for (double x : share) W += x;
        for (double x : share) least = std::min(least, 256 * x / W);
        if (least >= 1.0 + 1e-9) CHECK(cl.wgs == 256, "G %d class lgw %d: %u", G, cl.lgw, cl.wgs);
        s0 += cl.S;
      }
      CHECK(j == G && s0 == sbase, "G %d", G);
    }
  // the refusals, each with the nearest layout that is accepted
  const uint32_t R3 = 256;
  CHECK(plan_mg_layout({group_of(256 * R3, 3, 6, 0), group_of(100, 0, 6, 0)}, 256).ok, "256 slices");
  CHECK(!plan_mg_layout({group_of(256 * R3 + 1, 3, 6, 0), group_of(100, 0, 6, 0)}, 256).ok, "257 slices");
  CHECK(!plan_mg_layout({group_of(0, 3, 6, 0), group_of(100, 0, 6, 0)}, 256).ok, "no slice");
  {
    std::vector<ProbeGroup> gs(2, group_of(100, 1, 6, 0));
    gs[1].stacked = nullptr;
    CHECK(!plan_mg_layout(gs, 256).ok, "no image");
  }
  CHECK(plan_mg_layout(std::vector<ProbeGroup>(4, group_of(256 * R3, 3, 6, 0)), 256).ok, "1,024 slices");
  CHECK(!plan_mg_layout(std::vector<ProbeGroup>(5, group_of(205 * R3, 3, 6, 0)), 256).ok, "1,025 slices");
  // eoff > 65,535 (u16 table offsets): 30 one-bit groups of 20 slices hold 30 x
  // 2,208 = 66,240 entries per chunk (600 slices, 8,640 answer bytes, 17,664 B staged)
  CHECK(plan_mg_layout(std::vector<ProbeGroup>(30, group_of(2048, 0, 6, 0)), 256).ok, "30 x 2,056 entries");
  CHECK(!plan_mg_layout(std::vector<ProbeGroup>(30, group_of(20 * 2048, 0, 6, 0)), 256).ok, "eoff");
  // aoff > 96 KiB and stage > 64 KiB cannot be reached on their own with these
  // constants: a group has at most kMaxSlices slices, so a pair stages at most
  // 2 x (C + 8 x 256) x 4 B, and its answers take at most its entries + 15 B,
  // so aoff <= eoff + 15 G stays below 96 KiB while eoff <= 65,535.
  static_assert(2u * mg_sub_entries(C, kMaxSlices) * 4u <= 64u * 1024u, "stage bound");
  static_assert(mg_sub_abytes(C, kMaxSlices, 3) <= mg_sub_entries(C, kMaxSlices) + 15u, "answer bound");
  static_assert(65535u + 15u * (65535u / C) <= 96u * 1024u, "aoff bound");
}

// ---- slice geometry, rounds, job tables ---------------------------------------
static void test_geometry() {
  int lgR = 0;
  uint32_t R = 0;
  CHECK(group_slices(8, 31251, 3, &lgR, &R) == 128 && R == 245 && lgR == 8, "worked example: R %u", R);
  for (uint32_t nC : {32u, 33u, 1000u}) CHECK(slice_parts(128, nC, 8) == 2, "parts at %u chunks", nC);
  CHECK(slice_parts(128, 16, 8) == 1 && slice_parts(128, 1, 8) == 1, "a part has a chunk per wave");
  for (int lgw = 0; lgw < 3; lgw++) {
    CHECK(group_slices(8, 5000, lgw, &lgR, &R) != 0 && lgR == 11 - lgw && R <= (1u << lgR), "lgw %d", lgw);
    CHECK(group_slices(7, 5000, lgw, &lgR, &R) != 0 && lgR == 11 - lgw, "lgw %d", lgw);
    CHECK(group_slices(8, 0, lgw, &lgR, &R) == 0, "L 0");
    CHECK(group_slices(8, (256u << (11 - lgw)) + 1, lgw, &lgR, &R) == 0, "257 slices, lgw %d", lgw);
  }
  CHECK(group_slices(8, 0, 3, &lgR, &R) == 0, "L 0");
  CHECK(group_slices(8, 256 * 256, 3, &lgR, &R) == 256 && R == 256, "256 slices");
  CHECK(group_slices(8, 256 * 256 + 1, 3, &lgR, &R) == 0, "257 slices of 128 KiB");
  CHECK(group_slices(7, 256 * 256 + 1, 3, &lgR, &R) == 0 && lgR == 8, "257 slices of 128 KiB from 64 KiB");
  CHECK(group_slices(7, 256 * 128 + 1, 3, &lgR, &R) != 0 && lgR == 8, "more than 256 slices of 64 KiB");
  for (uint32_t L : {1u, 100u, 3005u, 31251u, 60000u})  // every line in exactly one slice
    for (int lgw = 0; lgw <= 3; lgw++)
      for (int plg : {7, 8}) {
        const uint32_t S = group_slices(plg, L, lgw, &lgR, &R);
        CHECK(S >= 1 && S <= 256 && R >= 1 && R <= (1u << lgR), "L %u lgw %d", L, lgw);
        CHECK(static_cast<uint64_t>(S - 1) * R < L && L <= static_cast<uint64_t>(S) * R, "L %u lgw %d", L, lgw);
      }

  for (uint64_t C : {2048ull, 4096ull, 8192ull, 16384ull})
    for (uint64_t n : {1ull, 4095ull, 4096ull, 4097ull, 100000ull, 1000003ull, 100000000ull})
      for (uint64_t pr : {0ull, 1ull, 4096ull, 10000ull, 65536ull, 99999ull, 100000ull, 1ull << 40})
        for (bool serial : {false, true}) {
          const ProbeRounds r = probe_rounds(n, pr, serial, C);
          if (pr == 0 || pr >= n) {
            CHECK(r.round == n && r.n_rounds == 1 && !r.pipe && r.nbuf == 1, "n %llu pr %llu",
                  (unsigned long long)n, (unsigned long long)pr);
          } else {
            CHECK(r.round % C == 0 && r.round >= C && r.round <= std::max(C, pr), "n %llu pr %llu",
                  (unsigned long long)n, (unsigned long long)pr);
          }
          CHECK((r.n_rounds - 1) * r.round < n && n <= r.n_rounds * r.round, "n %llu pr %llu",
                (unsigned long long)n, (unsigned long long)pr);
          CHECK(r.pipe == (r.n_rounds > 1 && !serial) && r.nbuf == (r.pipe ? kProbeBufs : 1), "pipe");
          CHECK(r.nCmax == (std::min(r.round, n) + C - 1) / C, "nCmax");
        }
  const uint64_t offs[8] = {0, 3, 3, 10, 11, 20, 21, 30};
  const uint8_t blob[64] = {};
  KeyDesc kd{blob, nullptr, 7, 9, 0};
  KeyDesc kr = round_keys(kd, 2, 4);
  CHECK(kr.bytes == blob + 18 && kr.offsets == nullptr && kr.n == 4 && kr.key_len == 9 && kr.suffix == 0, "fixed");
  kd.offsets = offs;
  kr = round_keys(kd, 2, 4);
  CHECK(kr.bytes == blob && kr.offsets == offs + 2 && kr.n == 4, "offsets");

  for (int seed = 0; seed < 200; seed++) {
    std::mt19937 rng(seed);
    const int n_jobs = 1 + rng() % 12, G = 1 + rng() % 6, bpk = 10;
    std::vector<dlsm_build_job> jobs(n_jobs);
    std::vector<uint32_t> Ls(n_jobs);
    for (int j = 0; j < n_jobs; j++) {
      jobs[j] = dlsm_build_job{{blob, nullptr, 20, 0, rng() % 3 ? rng() % 40000 : 0}, nullptr, 64};
      Ls[j] = full_num_lines(jobs[j].keys.n, bpk, nullptr);
    }
    const int lgR = choose_build_lgR(Ls);
    CHECK(lgR >= 7 && lgR <= 11, "lgR %d", lgR);
    uint64_t out_len[12];
    const JobTable<FullJobDev> T = plan_full_jobs(jobs.data(), n_jobs, bpk, out_len, Ls, lgR, true, seed % 2);
    uint64_t entry = 0, tabw = 0;
    uint32_t chunk = 0, slice = 0;
    for (int j = 0; j < n_jobs; j++) {
      const FullJobDev& d = T.hj[j];
      const uint32_t nc = static_cast<uint32_t>((jobs[j].keys.n + kBuildChunk - 1) / kBuildChunk);
      const uint32_t ns = std::max(1u, (Ls[j] + (1u << lgR) - 1) >> lgR);
      CHECK(d.entry0 == entry && d.tab0 == tabw && d.chunk0 == chunk && d.slice0 == slice, "job %d", j);
      CHECK(d.n_chunks == nc && d.n_slices == ns && d.L_spec == Ls[j] && d.out_len == out_len + j, "job %d", j);
      CHECK(d.k == full_num_probes(bpk) && d.bpk == bpk && d.exact == seed % 2 && d.keys.n == jobs[j].keys.n, "job");
      CHECK(T.starts[j] == chunk && T.starts[n_jobs + j] == slice, "job %d", j);
      entry += static_cast<uint64_t>(nc) * kBuildRegion;
      tabw += static_cast<uint64_t>(ns + 1) * nc;
      chunk += nc;
      slice += ns;
    }
    CHECK(T.entry == entry && T.tabw == tabw && T.chunk == chunk && T.slice == slice, "totals");
    const std::vector<int> cut = job_group_cuts(T.starts, T.chunk, n_jobs, G);
    CHECK(cut.front() == 0 && cut.back() == n_jobs && static_cast<int>(cut.size()) - 1 <= G, "cuts: %zu", cut.size());
    for (size_t i = 1; i < cut.size(); i++) CHECK(cut[i - 1] < cut[i], "cut %zu", i);
  }
}

int main() {
  test_version_index();
  test_version_large();
  test_version_layout();
  test_filter_groups();
  test_mg_layout();
  test_geometry();
  printf("OK host plan\n");
  return 0;
}
