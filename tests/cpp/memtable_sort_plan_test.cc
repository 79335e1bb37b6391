// tests/cpp/memtable_sort_plan_test.cc -- the memtable sort's host planning
// (plan_memtable_sort in host_plan.h, the geometry of memtable_sort.h) against
// brute force.  argv[1..]: batch sizes.  For each of them, and for sizes near
// UINT32_MAX made here: the pairs of every pass tile [0, n) exactly once with
// a0 <= b0 <= b1 and tile0 the pair's first tile; the last pass, and none
// before it, leaves one segment; the grid covers every tile; the workspace
// regions are aligned, ordered and large enough; the argument rules.
// Prints "OK ..." and exits 0 when everything holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dlsm_amd/csrc/host_plan.h"

using namespace dlsm;
using namespace dlsm::plan;

static int fails = 0;
#define EXPECT(c)                                                            \
  do {                                                                       \
    if (!(c)) {                                                              \
      if (fails++ < 20) printf("FAIL %s:%d %s (n = %llu)\n", __FILE__, __LINE__, #c, static_cast<unsigned long long>(n)); \
    }                                                                        \
  } while (0)

static void check(uint64_t n) {
  MemtableSortPlan P;
  EXPECT(plan_memtable_sort(n, kSortMaxWgs, P) == DLSM_OK);
  EXPECT(P.n == n && P.tab.n_runs == 1 && P.tab.n_passes == 0 && P.tab.base[0] == 0 && P.tab.base[1] == n);
  EXPECT(P.tiles == (n + kMsTile - 1) / kMsTile && P.passes <= kMsMaxPasses);
  EXPECT((static_cast<uint64_t>(kMsTile) << P.passes) >= n);
  EXPECT(P.passes == 0 || (static_cast<uint64_t>(kMsTile) << (P.passes - 1)) < n);
  EXPECT(P.nwg >= 1 && P.nwg <= kSortMaxWgs && static_cast<uint64_t>(P.nwg) * P.cpw >= P.tiles);
  for (uint32_t pass = 0; pass < P.passes; pass++) {
    const uint64_t w = static_cast<uint64_t>(kMsTile) << pass;
    uint64_t end = 0;  // the records the pairs so far cover
    for (uint32_t t = 0; t < P.tiles;) {
      const CmPair p = ms_pair(n, pass, t);
      EXPECT(p.tile0 == t && p.a0 == end && p.a0 == static_cast<uint64_t>(t) * kMsTile);
      EXPECT(p.a0 <= p.b0 && p.b0 <= p.b1 && p.b1 <= n && p.b1 > p.a0);
      EXPECT(p.b0 == std::min<uint64_t>(p.a0 + w, n) && p.b1 == std::min<uint64_t>(p.a0 + 2 * w, n));
      const uint32_t own = static_cast<uint32_t>((static_cast<uint64_t>(p.b1) - p.a0 + kMsTile - 1) / kMsTile);
      const CmPair last = ms_pair(n, pass, t + own - 1);  // every tile of the pair names it
      EXPECT(last.a0 == p.a0 && last.b0 == p.b0 && last.b1 == p.b1 && last.tile0 == p.tile0);
      end = p.b1;
      t += own;
    }
    EXPECT(end == n);
  }
  const uint64_t offs[] = {P.tab_off, P.tot_off, P.rec_off[0], P.rec_off[1], P.ko_off,   P.vo_off,
                           P.flag_off, P.cnt_off, P.kb_off,    P.vb_off,     P.split_off};
  for (size_t j = 0; j < sizeof(offs) / sizeof(offs[0]); j++) EXPECT(offs[j] % 256 == 0 && (j == 0 || offs[j] >= offs[j - 1]));
  EXPECT(P.rec_off[1] - P.rec_off[0] >= sizeof(CmRec) * n && P.ko_off - P.rec_off[1] >= sizeof(CmRec) * n);
  EXPECT(P.vo_off - P.ko_off >= 8 * (n + 1) && P.flag_off - P.vo_off >= 8 * (n + 1));
  EXPECT(P.cnt_off - P.flag_off >= 8ull * P.nwg && P.split_off - P.vb_off >= 8ull * P.nwg);
  EXPECT(P.bytes - P.split_off >= 4 * (static_cast<uint64_t>(P.tiles) + 1));
}

int main(int argc, char** argv) {
  for (int j = 1; j < argc; j++) check(strtoull(argv[j], nullptr, 10));
  for (uint64_t n : {0xffffffffull, 0xffffffffull - kMsTile, 0xfffffc01ull, 0xfffffc00ull, 0x80000001ull, 0x80000000ull}) check(n);
  const uint64_t n = 0x100000000ull;
  MemtableSortPlan P;
  EXPECT(plan_memtable_sort(n, kSortMaxWgs, P) == DLSM_E_ARG && plan_memtable_sort(10, 0, P) == DLSM_E_ARG);
  if (fails) return 1;
  printf("OK %d sizes\n", argc - 1);
  return 0;
}
