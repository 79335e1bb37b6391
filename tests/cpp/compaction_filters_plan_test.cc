// tests/cpp/compaction_filters_plan_test.cc -- the compaction filters' host
// planning (dlsm::plan in host_plan.h, the geometry of compaction_filters.h)
// against brute force.  argv[1]: a text file of cuts, one per line:
//   bits_per_key  n_files  size_0 ... size_{n_files-1}
// For every cut, and for a few extreme ones made here, with every file taken at
// its most lines (no duplicate) and at a distinct count of half its pairs:
//   - no chunk's bins pass cf_bins_bound / kCfMaxBins;
//   - the flat slices stay inside the slice grid;
//   - the padded blocks stay inside dlsm_compaction_filters_bound's capacity;
//   - the workspace regions are ordered, aligned and inside `bytes`.
// Prints "OK ..." and exits 0 when everything holds.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <vector>

#include "../../dlsm_amd/csrc/host_plan.h"

using namespace dlsm;
using namespace dlsm::plan;

static int fails = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) {                                                    \
      fails++;                                                     \
      printf("FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #c, what); \
    }                                                              \
  } while (0)

static void check_cut(const std::vector<uint64_t>& sizes, int bpk, int distinct_div, const char* what) {
  uint64_t n = 0;
  for (uint64_t s : sizes) n += s;
  const uint64_t F = sizes.size();
  CompactionFiltersPlan P;
  EXPECT(plan_compaction_filters(n, F, bpk, P) == DLSM_OK);
  EXPECT(P.lgR >= kCfMinLgR && P.lgR <= kCfMaxLgR && P.lgR == filters_lgR(n, F, bpk));
  EXPECT(P.chunks == std::max<uint64_t>((n + kCfChunk - 1) / kCfChunk, 1));
  EXPECT(cf_bins_bound(bpk, P.lgR) <= kCfMaxBins);
  uint64_t cap = 0;
  EXPECT(plan_compaction_filters_bound(n, F, bpk, &cap) == DLSM_OK);
  // brute force: every file's lines, slices and block, every chunk's bins
  std::vector<uint64_t> bins(P.chunks, 0);
  uint64_t at = 0, slices = 0, bytes = 0;
  for (uint64_t s : sizes) {
    const uint64_t D = std::max<uint64_t>(s / distinct_div, 1);
    const uint32_t L = full_num_lines(D, bpk, nullptr);
    EXPECT(L <= filters_max_lines(s, bpk));
    uint32_t ns = cf_slices(L, P.lgR);
    if (ns > kCfMaxSlices) ns = 0;  // flagged, not built
    slices += ns;
    bytes += co_pad16(cf_block_bytes(L));
    for (uint64_t c = at / kCfChunk; c <= (at + s - 1) / kCfChunk; c++) bins[c] += ns;
    at += s;
  }
  for (uint64_t b : bins) EXPECT(b <= cf_bins_bound(bpk, P.lgR));
  EXPECT(slices <= P.slice_wgs && P.slice_wgs == filters_slice_bound(n, F, bpk, P.lgR));
  EXPECT(bytes <= cap);
  const uint64_t offs[] = {P.tot_off,  P.hash_off,   P.ccnt_off, P.cscan_off, P.gpre_off, P.cut_off,    P.fL_off,
                           P.fmagic_off, P.fsl0_off, P.fbase_off, P.clo_off,  P.tab_off,  P.region_off, P.partial_off};
  for (size_t j = 0; j < sizeof(offs) / sizeof(offs[0]); j++)
    EXPECT(offs[j] % 256 == 0 && offs[j] < P.bytes && (j == 0 || offs[j] > offs[j - 1]));
  EXPECT(P.bytes - P.partial_off >= 4ull * P.slice_wgs && P.partial_off - P.region_off >= 4ull * P.chunks * kCfRegion);
}

int main(int argc, char** argv) {
  int cuts = 0;
  const char* what = "args";
  EXPECT(argc == 2);
  if (argc != 2) return 1;
  std::ifstream in(argv[1]);
  for (std::string line; std::getline(in, line);) {
    std::istringstream ls(line);
    int bpk = 0;
    uint64_t nf = 0;
    ls >> bpk >> nf;
    std::vector<uint64_t> sizes(nf);
    for (uint64_t& s : sizes) ls >> s;
    what = line.c_str();
    EXPECT(!ls.fail() && nf > 0);
    for (int div : {1, 2}) check_cut(sizes, bpk, div, line.substr(0, 60).c_str());
    cuts++;
  }
  // the extremes of the bins bound: a chunk of one-pair files between two files at the slice maximum, at the
  // smallest and the largest bits per key; whole files of several slices each inside a chunk
  for (int bpk : {1, 10, kCfMaxBpk}) {
    const uint64_t big = static_cast<uint64_t>(kCfMaxSlices) * 128 * 512 / bpk - 1024;
    std::vector<uint64_t> s{big / kCfChunk * kCfChunk + 1};
    for (int j = 0; j < 4094; j++) s.push_back(1);
    s.push_back(big);
    check_cut(s, bpk, 1, "one-pair files between two large files");
    check_cut(std::vector<uint64_t>(4096, 1), bpk, 1, "4096 one-pair files");
    check_cut(std::vector<uint64_t>(64, 127), bpk, 1, "files of 127 pairs");
    check_cut({3000000}, bpk, 1, "one file");
  }
  const char* none = "arguments";
  what = none;
  CompactionFiltersPlan P;
  uint64_t cap;
  EXPECT(plan_compaction_filters(0x100000000ull, 1, 10, P) == DLSM_E_ARG);
  EXPECT(plan_compaction_filters(10, kCoMaxFiles + 1, 10, P) == DLSM_E_ARG);
  EXPECT(plan_compaction_filters(10, 1, 0, P) == DLSM_E_ARG && plan_compaction_filters(10, 1, kCfMaxBpk + 1, P) == DLSM_E_ARG);
  EXPECT(plan_compaction_filters_bound(10, kCoMaxFiles + 1, 10, &cap) == DLSM_E_ARG);
  EXPECT(plan_compaction_filters(0, 0, 10, P) == DLSM_OK && P.chunks == 1 && P.slice_wgs >= 1);
  if (fails) return 1;
  printf("OK %d cuts\n", cuts);
  return 0;
}
