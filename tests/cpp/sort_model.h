// tests/cpp/sort_model.h -- a host model of one counting-sort pass
// (dlsm_amd/csrc/sort_pass.h) for the CPU tests: the items walked in the
// kernels' (workgroup, chunk, wave) order with the planner's numbers, the
// bin-major (bin, workgroup) table, its exclusive offsets (each bin's start
// rounded up to an alignment) and the stable scatter; and the checks of the
// grid every user of the pass relies on.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dlsm_amd/csrc/host_plan.h"

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                \
      printf("\n");                                       \
      exit(1);                                            \
    }                                                     \
  } while (0)

namespace sort_model {

// f(w, i0, i1) for every wave's share [i0, i1) of every chunk, in walk order.
template <class F>
void walk(uint32_t nwg, uint32_t cpw, uint32_t chunk, uint64_t items, F&& f) {
  const uint32_t wave_items = chunk / dlsm::kSortWaves;
  for (uint32_t w = 0; w < nwg; w++)
    for (uint64_t c = uint64_t(w) * cpw; c < uint64_t(w + 1) * cpw; c++) {
      const uint64_t c0 = c * chunk;
      if (c0 >= items) break;
      for (int wave = 0; wave < dlsm::kSortWaves; wave++) {
        const uint64_t i0 = c0 + uint64_t(wave) * wave_items;
        const uint64_t i1 = std::min(i0 + wave_items, items);
        if (i0 < i1) f(w, i0, i1);
      }
    }
}

template <class Item>
struct Pass {
  std::vector<uint64_t> begin, count;  // per bin: its first output position, its items
  uint64_t end = 0;                    // the last bin's end, rounded up to the alignment
  std::vector<Item> out;               // max(cap, end) slots; `fill` where nothing was written
};

// of_wg[w]: workgroup w's items in walk order; bin_of(item) < bins.  The table
// has bins x nwg of the table_entries the planner sized.
template <class Item, class BinOf>
Pass<Item> run_pass(const std::vector<std::vector<Item>>& of_wg, uint32_t bins, uint64_t table_entries, uint64_t align,
                    uint64_t cap, Item fill, BinOf&& bin_of) {
  const uint64_t nwg = of_wg.size();
  CHECK(uint64_t(bins) * nwg <= table_entries, "table extent");
  std::vector<uint64_t> cnt(table_entries, 0), off(table_entries, 0);
  for (uint64_t w = 0; w < nwg; w++)
    for (const Item& it : of_wg[w]) {
      const uint64_t e = uint64_t(bin_of(it)) * nwg + w;
      CHECK(e < table_entries, "table index");
      cnt[e]++;
    }
  Pass<Item> P;
  P.begin.assign(bins, 0);
  P.count.assign(bins, 0);
  uint64_t at = 0;
  for (uint32_t b = 0; b < bins; b++) {
    P.begin[b] = at;
    for (uint64_t w = 0; w < nwg; w++) {
      off[b * nwg + w] = at;
      at += cnt[b * nwg + w];
    }
    P.count[b] = at - P.begin[b];
    at = (at + align - 1) / align * align;
  }
  P.end = at;
  P.out.assign(std::max(cap, at), fill);
  for (uint64_t w = 0; w < nwg; w++)
    for (const Item& it : of_wg[w]) P.out[off[uint64_t(bin_of(it)) * nwg + w]++] = it;
  return P;
}

// The grid of a pass: it covers the chunks, no workgroup is idle, and past the
// cap every workgroup takes several chunks.
inline void check_grid(uint64_t items, uint32_t chunk, uint32_t max_wgs) {
  const dlsm::plan::SortGrid g = dlsm::plan::sort_grid(items, chunk, max_wgs);
  CHECK(g.chunks == (items + chunk - 1) / chunk, "chunks");
  CHECK(g.cpw >= 1 && g.nwg <= max_wgs && uint64_t(g.nwg) * g.cpw >= g.chunks, "the grid covers the chunks");
  CHECK(items == 0 ? g.nwg == 0 : uint64_t(g.nwg - 1) * g.cpw < g.chunks, "no idle workgroup");
  if (items > uint64_t(max_wgs) * chunk) CHECK(g.cpw > 1, "past the workgroup cap: several chunks each");
}

inline void test_grid() {
  for (uint32_t chunk : {dlsm::kPlanChunk, dlsm::kRouteChunk})
    for (uint32_t max_wgs : {4u, 512u})
      for (uint64_t items : std::vector<uint64_t>{0, 1, chunk - 1u, chunk, chunk + 1u,
                                                  uint64_t(max_wgs) * chunk * 3 + 5, 0xffffffffull})
        check_grid(items, chunk, max_wgs);
}

}  // namespace sort_model
