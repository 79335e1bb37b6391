// tests/cpp/read_plan_test.cc -- the read plan on the CPU: the task decoder
// (dlsm_amd/csrc/read_plan.h) against brute force, the planner
// (dlsm::plan::plan_read) and the host model of a pass (sort_model.h) per
// digit, fed in the kernels' item order with the planner's numbers, against a
// stable sort.
// Prints "OK" on success; exits non-zero with a message otherwise.
#include <random>

#include "sort_model.h"

using namespace dlsm;
using namespace dlsm::plan;

// A version as explicit lists: level-0 files in search order, then each level's
// files; ids are positions in search order.
struct Lists {
  std::vector<uint32_t> l0;
  std::vector<uint32_t> lvl[kPlanLevels];
  PlanShape shape{};
  uint32_t n_files = 0;
};

static Lists make_lists(uint32_t n_l0, const uint32_t (&counts)[kPlanLevels]) {
  Lists L;
  uint32_t id = 0;
  for (uint32_t j = 0; j < n_l0; j++) L.l0.push_back(id++);
  uint32_t begin[kNumLevels] = {}, count[kNumLevels] = {};
  count[0] = n_l0;
  for (int lv = 0; lv < kPlanLevels; lv++) {
    begin[lv + 1] = id;
    count[lv + 1] = counts[lv];
    for (uint32_t q = 0; q < counts[lv]; q++) L.lvl[lv].push_back(id++);
  }
  L.n_files = id;
  L.shape = plan_shape(n_l0, begin, count);
  return L;
}

// The issue's words, restated on the lists.
static uint32_t brute_task(const Lists& L, uint32_t slot, uint32_t pick) {
  const uint32_t n_slots = static_cast<uint32_t>(L.l0.size()) + kPlanLevels;
  if (slot >= n_slots) return kPlanNoFile;
  if (slot < L.l0.size()) return L.l0[slot];
  const std::vector<uint32_t>& files = L.lvl[slot - L.l0.size()];
  if (pick >= files.size()) return kPlanNoFile;
  return files[pick];
}

static void test_decoder() {
  const uint32_t shapes[][kPlanLevels] = {{0, 0, 0, 0, 0}, {1, 1, 1, 1, 1}, {8, 16, 0, 2, 1}, {0, 0, 0, 0, 7},
                                          {70000, 0, 3, 0, 0}, {1, 0, 0, 0, 0}};
  for (uint32_t n_l0 : {0u, 1u, 4u, 59u})
    for (const auto& counts : shapes) {
      const Lists L = make_lists(n_l0, counts);
      CHECK(L.shape.n_slots == n_l0 + 5 && L.shape.n_slots <= 64, "slots");
      for (uint32_t slot = 0; slot < 64; slot++) {
        std::vector<uint32_t> picks = {0u, 1u, 0xffffffffu, 0xfffffffeu, 0x80000000u};
        for (uint32_t c : counts) {
          picks.push_back(c);
          picks.push_back(c - 1);  // (count 0: UINT32_MAX again)
          picks.push_back(c + 1);
        }
        for (uint32_t pick : picks) {
          const uint32_t want = brute_task(L, slot, pick);
          const uint32_t got = plan_task_file(L.shape, slot, pick);
          CHECK(got == want, "n_l0 %u slot %u pick %u: %u != %u", n_l0, slot, pick, got, want);
          CHECK(got == kPlanNoFile || got < L.n_files, "range");
        }
      }
      // slots the decoder can never be asked for by a u64 mask, but must survive
      for (uint32_t slot : {64u, 65u, 1000u, 0xffffffffu}) CHECK(plan_task_file(L.shape, slot, 0) == kPlanNoFile, "high");
    }
}

static void test_planner() {
  const uint64_t nfs[] = {0, 1, kSortBins - 1, kSortBins, kSortBins + 1, 70001, 1ull << 24};
  const uint64_t ns[] = {0, 1, 0xffffffffull};
  std::mt19937_64 rng(5);
  for (uint64_t nf : nfs)
    for (uint64_t n : ns)
      for (int mode : {DLSM_PLAN_FIRST, DLSM_PLAN_ALL})
        for (uint32_t tpg : {1u, 9u, 64u}) {
          ReadPlan R;
          CHECK(plan_read(n, nf, tpg, mode, R) == DLSM_OK, "plan_read");
          CHECK(R.passes >= 1 && R.passes <= kPlanMaxPasses, "passes");
          CHECK((nf <= kSortBins) == (R.passes == 1), "one pass iff the files fit the bins (%llu)",
                (unsigned long long)nf);
          // the digits cover the file ids: they put every id back together
          std::vector<uint64_t> ids = {0, nf ? nf - 1 : 0, nf / 2};
          for (int q = 0; q < 50 && nf; q++) ids.push_back(rng() % nf);
          for (uint64_t f : ids) {
            uint64_t back = 0;
            for (int p = 0; p < R.passes; p++) {
              CHECK(R.pass[p].shift == static_cast<uint32_t>(p) * kSortBinLg, "shift");
              back |= static_cast<uint64_t>(plan_digit(static_cast<uint32_t>(f), R.pass[p].shift)) << R.pass[p].shift;
            }
            CHECK(back == f, "digits of %llu", (unsigned long long)f);
          }
          CHECK(R.tasks_max == (mode == DLSM_PLAN_FIRST ? n : n * tpg), "tasks_max");
          // geometry: the chunks cover the items, no workgroup is empty, table indices in range
          for (int p = 0; p < R.passes; p++) {
            const ReadPlanPass& P = R.pass[p];
            CHECK(P.items_max == (p == 0 ? n : R.tasks_max), "items");
            CHECK(P.nwg <= kSortMaxWgs && P.nwg <= R.table_wgs && P.cpw >= 1, "grid");
            CHECK(static_cast<unsigned __int128>(P.nwg) * P.cpw * kPlanChunk >= P.items_max, "cover");
            if (P.nwg)
              CHECK(static_cast<unsigned __int128>(P.nwg - 1) * P.cpw * kPlanChunk < P.items_max, "empty workgroup");
            CHECK((P.items_max == 0) == (P.nwg == 0), "nwg");
            // a (workgroup, bin) count fits its u32: the Gets of a workgroup times the tasks of a Get
            CHECK(static_cast<unsigned __int128>(P.cpw) * kPlanChunk * (p == 0 ? tpg : 1) < (1ull << 32), "count");
            if (P.nwg) {
              const uint64_t hi = static_cast<uint64_t>(kSortBins - 1) * P.nwg + (P.nwg - 1);
              CHECK(hi < R.table_entries, "table index");
              CHECK(hi * sizeof(uint32_t) < R.cnt_bytes && hi * sizeof(uint64_t) < R.off_bytes, "table extent");
              CHECK((P.nwg - 1) * sizeof(uint64_t) < R.drop_bytes, "drop extent");
            }
          }
          CHECK(R.table_entries == static_cast<uint64_t>(kSortBins) * R.table_wgs && R.table_entries % 4 == 0, "table");
          // workspace regions: aligned, inside, disjoint
          std::vector<std::pair<uint64_t, uint64_t>> ext = {
              {R.cnt_off, R.cnt_bytes},         {R.off_off, R.off_bytes},         {R.drop_off, R.drop_bytes},
              {R.total_off, R.total_bytes},     {R.keys_off[0], R.keys_bytes[0]}, {R.vals_off[0], R.vals_bytes[0]},
              {R.keys_off[1], R.keys_bytes[1]}, {R.vals_off[1], R.vals_bytes[1]}};
          for (auto& e : ext) {
            CHECK(e.first % 256 == 0 && e.first + e.second <= R.bytes, "region");
            e.second += e.first;
          }
          std::sort(ext.begin(), ext.end());
          for (size_t i = 1; i < ext.size(); i++) CHECK(ext[i - 1].second <= ext[i].first, "regions overlap");
          // which pair buffers exist: FIRST's ids in keys[1]; pairs only for several passes
          const uint64_t pb = sizeof(uint32_t) * R.tasks_max;
          CHECK(R.keys_bytes[1] == ((R.passes > 1 || mode == DLSM_PLAN_FIRST) ? pb : 0), "keys[1]");
          CHECK(R.keys_bytes[0] == (R.passes > 1 ? pb : 0) && R.vals_bytes[0] == R.keys_bytes[0], "buffer 0");
          CHECK(R.vals_bytes[1] == (R.passes > 2 ? pb : 0), "vals[1]");
        }
  ReadPlan R;
  CHECK(plan_read(1ull << 32, 10, 1, DLSM_PLAN_FIRST, R) == DLSM_E_ARG, "n > UINT32_MAX");
  CHECK(plan_read(10, 10, 1, 7, R) == DLSM_E_ARG && plan_read(10, 10, 1, -1, R) == DLSM_E_ARG, "mode");
  CHECK(read_plan_passes(70001) == 2 && read_plan_passes(1ull << 24) == 3 && read_plan_passes(1) == 1, "passes");
  CHECK(read_plan_passes((1ull << 24) + 1) == 3 && read_plan_passes((1ull << 27) + 1) == 4, "passes");
}

// ---- host model of the passes -------------------------------------------------
struct Item {
  uint32_t key, val;
};

// Pass 0's items in the kernels' order: each wave's share of a chunk 64 Gets
// at a time; FIRST: a Get's lowest set slot; ALL: slot by slot over the 64 Gets.
static void walk_masks_model(const Lists& L, const std::vector<uint32_t>& order, const std::vector<uint64_t>& mask,
                             const std::vector<uint32_t>& pick, bool all, uint64_t i0, uint64_t i1,
                             std::vector<Item>& out, uint64_t& dropped) {
  auto decode = [&](uint64_t g, uint32_t s) {
    const uint32_t p = s >= L.shape.n_l0 && s < L.shape.n_slots ? pick[g * kPlanLevels + (s - L.shape.n_l0)] : 0;
    const uint32_t f = plan_task_file(L.shape, s, p);
    return f == kPlanNoFile ? kPlanNoFile : order[f];
  };
  for (uint64_t r = i0; r < i1; r += 64) {
    const uint64_t e = std::min(r + 64, i1);
    if (!all) {
      for (uint64_t g = r; g < e; g++) {
        if (!mask[g]) continue;
        const uint32_t k = decode(g, static_cast<uint32_t>(__builtin_ctzll(mask[g])));
        if (k == kPlanNoFile) dropped++;
        else out.push_back({k, static_cast<uint32_t>(g)});
      }
    } else {
      for (uint64_t g = r; g < e; g++)
        if (L.shape.n_slots < 64) dropped += static_cast<uint64_t>(__builtin_popcountll(mask[g] >> L.shape.n_slots));
      for (uint32_t s = 0; s < L.shape.n_slots; s++)
        for (uint64_t g = r; g < e; g++) {
          if (!((mask[g] >> s) & 1)) continue;
          const uint32_t k = decode(g, s);
          if (k == kPlanNoFile) dropped++;
          else out.push_back({k, static_cast<uint32_t>(g)});
        }
    }
  }
}

struct Model {
  std::vector<uint64_t> file_begin;
  std::vector<uint32_t> gets;
  uint64_t dropped = 0;
};

static Model run_model(const Lists& L, const std::vector<uint32_t>& order, const std::vector<uint64_t>& mask,
                       const std::vector<uint32_t>& pick, int mode) {
  const uint64_t n = mask.size();
  ReadPlan R;
  CHECK(plan_read(n, L.n_files, plan_tasks_per_get(L.shape), mode, R) == DLSM_OK, "plan");
  Model M;
  std::vector<Item> cur;
  uint64_t total = 0;
  for (int p = 0; p < R.passes; p++) {
    const ReadPlanPass& P = R.pass[p];
    // every workgroup's items, in walk order
    std::vector<std::vector<Item>> of_wg(P.nwg);
    sort_model::walk(P.nwg, P.cpw, kPlanChunk, p == 0 ? n : total, [&](uint32_t w, uint64_t i0, uint64_t i1) {
      if (p == 0) walk_masks_model(L, order, mask, pick, mode == DLSM_PLAN_ALL, i0, i1, of_wg[w], M.dropped);
      else of_wg[w].insert(of_wg[w].end(), cur.begin() + i0, cur.begin() + i1);
    });
    sort_model::Pass<Item> S = sort_model::run_pass(of_wg, kSortBins, R.table_entries, 1, 0, Item{0, 0},
                                                    [&](const Item& it) { return plan_digit(it.key, P.shift); });
    total = S.end;
    CHECK(total <= R.tasks_max, "tasks bound");
    if (R.passes == 1) {
      M.file_begin.assign(S.begin.begin(), S.begin.begin() + L.n_files);
      M.file_begin.push_back(total);
    }
    cur.swap(S.out);
  }
  if (R.passes > 1) {
    M.file_begin.assign(L.n_files + 1, 0);
    for (uint64_t f = 0; f <= L.n_files; f++)
      M.file_begin[f] = static_cast<uint64_t>(
          std::lower_bound(cur.begin(), cur.end(), f, [](const Item& it, uint64_t v) { return it.key < v; }) -
          cur.begin());
  }
  for (const Item& it : cur) M.gets.push_back(it.val);
  return M;
}

// The yardstick: (Get, file) pairs Get by Get, slot by slot; a stable sort by file.
static Model brute_plan(const Lists& L, const std::vector<uint32_t>& order, const std::vector<uint64_t>& mask,
                        const std::vector<uint32_t>& pick, int mode) {
  Model M;
  std::vector<Item> pairs;
  for (uint64_t g = 0; g < mask.size(); g++)
    for (uint32_t s = 0; s < 64; s++) {
      if (!((mask[g] >> s) & 1)) continue;
      const uint32_t p = s >= L.l0.size() && s < L.l0.size() + 5 ? pick[g * 5 + (s - L.l0.size())] : 0;
      const uint32_t f = brute_task(L, s, p);
      if (f == kPlanNoFile) M.dropped++;
      else pairs.push_back({order[f], static_cast<uint32_t>(g)});
      if (mode == DLSM_PLAN_FIRST) break;
    }
  std::stable_sort(pairs.begin(), pairs.end(), [](const Item& a, const Item& b) { return a.key < b.key; });
  M.file_begin.assign(L.n_files + 1, 0);
  for (const Item& it : pairs) M.file_begin[it.key + 1]++;
  for (uint32_t f = 0; f < L.n_files; f++) M.file_begin[f + 1] += M.file_begin[f];
  for (const Item& it : pairs) M.gets.push_back(it.val);
  return M;
}

static void test_model(uint32_t n_l0, const uint32_t (&counts)[kPlanLevels], uint64_t n, bool malformed,
                       uint32_t seed) {
  const Lists L = make_lists(n_l0, counts);
  std::mt19937_64 rng(seed);
  std::vector<uint32_t> order(L.n_files);
  for (uint32_t f = 0; f < L.n_files; f++) order[f] = f;
  std::shuffle(order.begin(), order.end(), rng);  // search order -> the caller's index
  std::vector<uint64_t> mask(n);
  std::vector<uint32_t> pick(n * 5);
  for (uint64_t g = 0; g < n; g++) {
    uint64_t m = rng() & rng();
    if (rng() % 4 == 0) m = 0;
    if (!malformed) m &= L.shape.n_slots < 64 ? (1ull << L.shape.n_slots) - 1 : ~0ull;
    for (int lv = 0; lv < 5; lv++) {
      uint32_t p = 0xffffffffu;
      if (counts[lv]) p = static_cast<uint32_t>(rng() % counts[lv]);
      else if (!malformed) m &= ~(1ull << (n_l0 + lv));
      if (malformed && rng() % 8 == 0) p = counts[lv] + static_cast<uint32_t>(rng() % 3);
      if (malformed && rng() % 16 == 0) p = 0xffffffffu;
      pick[g * 5 + lv] = p;
    }
    mask[g] = m;
  }
  for (int mode : {DLSM_PLAN_FIRST, DLSM_PLAN_ALL}) {
    const Model want = brute_plan(L, order, mask, pick, mode);
    const Model got = run_model(L, order, mask, pick, mode);
    CHECK(got.file_begin == want.file_begin, "file_begin (files %u, mode %d)", L.n_files, mode);
    CHECK(got.gets == want.gets, "gets (files %u, mode %d)", L.n_files, mode);
    CHECK(got.dropped == want.dropped && (malformed || want.dropped == 0), "dropped");
    CHECK(malformed || !want.gets.empty(), "the case has tasks");
    for (uint32_t f = 0; f < L.n_files; f++)
      for (uint64_t q = want.file_begin[f] + 1; q < want.file_begin[f + 1]; q++)
        CHECK(want.gets[q - 1] < want.gets[q], "strictly ascending");
  }
}

int main() {
  test_decoder();
  test_planner();
  sort_model::test_grid();
  const uint64_t C = kPlanChunk;
  test_model(4, {8, 16, 0, 2, 1}, 3 * C + 3, false, 1);                   // one pass
  test_model(4, {kSortBins - 4 - 5, 1, 1, 1, 1}, C + 1, false, 2);        // bins - 1 files
  test_model(4, {kSortBins - 4 - 3, 1, 1, 1, 1}, 3 * C + 3, false, 3);    // bins + 1: two passes
  test_model(59, {1, 1, 1, 1, 1}, 257, false, 4);                         // 64 slots
  test_model(1, {70000, 0, 0, 0, 0}, C + 65, false, 5);                   // 70,001 files
  test_model(3, {600, 0, 5, 0, 1}, 2 * C + 7, true, 6);                   // malformed masks and picks: dropped
  test_model(0, {0, 0, 0, 0, 0}, 100, true, 7);                           // no file at all
  printf("OK\n");
  return 0;
}
