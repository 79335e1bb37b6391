// tests/cpp/compaction_output_test.cc -- the compaction output's rules on the CPU
// (dlsm_amd/csrc/compaction_output.h): the cut against the reference's loop
// (DoCompactionWork closes a file once FileSize() >= MaxOutputFileSize(),
// db/db_impl.cc:3562-3573), the file of a pair, and a file's region through both
// views against a plain writer.  Keys and values live in allocations of their
// exact size so that a sanitizer sees a read past an end.
// Prints "OK" on success; exits non-zero with a message otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../dlsm_amd/csrc/compaction_output.h"

using namespace dlsm;

#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); \
      printf(__VA_ARGS__);                              \
      printf("\n");                                     \
      exit(1);                                          \
    }                                                   \
  } while (0)

// The cuts of a run, the reference's way: pair by pair.
static std::vector<uint32_t> walk(const std::vector<uint64_t>& size, uint64_t max_file_bytes) {
  std::vector<uint32_t> first;
  uint64_t file = 0;
  for (size_t i = 0; i < size.size(); i++) {
    if (file == 0) first.push_back(static_cast<uint32_t>(i));
    file += size[i];
    if (max_file_bytes && file >= max_file_bytes) file = 0;
  }
  return first;
}

static void test_cut(const std::vector<uint64_t>& size, uint64_t max_file_bytes) {
  const uint64_t n = size.size();
  std::vector<uint64_t> off(n + 1, 0);
  for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + size[i];
  std::vector<uint32_t> want = walk(size, max_file_bytes), got;
  for (uint64_t at = 0; at < n; at = co_cut_next(off.data(), n, at, max_file_bytes)) got.push_back(static_cast<uint32_t>(at));
  CHECK(got == want, "n %zu max %zu: %zu files, %zu wanted", size_t(n), size_t(max_file_bytes), got.size(), want.size());
  got.push_back(static_cast<uint32_t>(n));
  const uint32_t nf = static_cast<uint32_t>(want.size());
  for (uint32_t f = 0; f < nf; f++)
    for (uint64_t i = got[f]; i < got[f + 1]; i++) CHECK(co_file_of(got.data(), nf, i) == f, "pair %zu", size_t(i));
}

// A run whose keys and values are separate exact allocations is not what
// TbSource addresses (it wants them packed), so the packed arrays are exact too.
struct Run {
  std::unique_ptr<uint8_t[]> keys, values;
  std::vector<uint64_t> koff, voff, off;
  uint64_t n;
  Run(uint64_t n_, uint64_t (*kl)(uint64_t), uint64_t (*vl)(uint64_t)) : koff(n_ + 1, 0), voff(n_ + 1, 0), off(n_ + 1, 0), n(n_) {
    for (uint64_t i = 0; i < n; i++) {
      koff[i + 1] = koff[i] + kl(i);
      voff[i + 1] = voff[i] + vl(i);
      off[i + 1] = off[i] + 8 + kl(i) + vl(i);
    }
    keys.reset(new uint8_t[koff[n]]);
    values.reset(new uint8_t[voff[n]]);
    for (uint64_t b = 0; b < koff[n]; b++) keys[b] = static_cast<uint8_t>(b * 7 + 1);
    for (uint64_t b = 0; b < voff[n]; b++) values[b] = static_cast<uint8_t>(b * 13 + 5);
  }
  std::string region(uint64_t a, uint64_t e) const {  // Add, table_builder_bacs.cpp:221-226, for pairs [a, e)
    std::string o;
    for (uint64_t i = a; i < e; i++) {
      const uint32_t ks = static_cast<uint32_t>(koff[i + 1] - koff[i]), vs = static_cast<uint32_t>(voff[i + 1] - voff[i]);
      o.append(reinterpret_cast<const char*>(&ks), 4).append(reinterpret_cast<const char*>(&vs), 4);
      o.append(reinterpret_cast<const char*>(keys.get() + koff[i]), ks).append(reinterpret_cast<const char*>(values.get() + voff[i]), vs);
    }
    return o;
  }
};

// Every file of the run through the view (and the fixed view where the lengths
// are uniform), every unit, clipped at every limit near the file's end.
static void test_files(const Run& r, uint64_t max_file_bytes, uint32_t klen, uint32_t vlen) {
  TbSource var{r.keys.get(), r.koff.data(), r.values.get(), r.voff.data(), 0, 0, r.off.data()};
  TbSource fix{r.keys.get(), nullptr, r.values.get(), nullptr, klen, vlen, r.off.data()};
  for (uint64_t a = 0, e; a < r.n; a = e) {
    e = co_cut_next(r.off.data(), r.n, a, max_file_bytes);
    const std::string want = r.region(a, e);
    CHECK(want.size() == r.off[e] - r.off[a], "file at %zu", size_t(a));
    for (uint64_t limit : {uint64_t(want.size()), uint64_t(want.size()) - 1, uint64_t(want.size()) / 2}) {
      for (int fixed = 0; fixed <= (klen ? 1 : 0); fixed++) {
        std::unique_ptr<uint8_t[]> got(new uint8_t[limit]);  // exact: a write past the limit is seen
        alignas(16) uint8_t slot[16];
        for (uint64_t u = 0; u < limit; u += 16) {
          const uint64_t p1 = u + 16 < limit ? u + 16 : limit;
          if (fixed) co_region_unit_fixed(fix, a, u, limit, slot);
          else tb_region_unit(CoFileView{var, a, r.off[a]}, e - a, u, limit, slot);
          memcpy(got.get() + u, slot, p1 - u);
        }
        CHECK(memcmp(got.get(), want.data(), limit) == 0, "file at %zu, limit %zu, fixed %d", size_t(a), size_t(limit), fixed);
      }
    }
  }
}

int main() {
  test_cut({}, 100);
  test_cut({64}, 100);
  test_cut({64, 64, 64}, 0);
  test_cut(std::vector<uint64_t>(25, 64), 640);   // the tenth pair lands on the threshold
  test_cut(std::vector<uint64_t>(25, 64), 641);   // one byte short: the eleventh joins
  test_cut(std::vector<uint64_t>(25, 64), 1);     // every pair a file
  test_cut({64, 64, 5000, 64, 64, 64}, 100);      // a pair larger than the threshold
  test_cut({64, 64, 64}, ~uint64_t(0));           // the limit saturates
  for (uint64_t max = 16; max < 700; max += 37) {
    std::vector<uint64_t> s;
    for (uint64_t i = 0; i < 500; i++) s.push_back(16 + (i * 131 + max) % 300);
    test_cut(s, max);
  }
  CHECK(co_pad16(0) == 0 && co_pad16(1) == 16 && co_pad16(16) == 16 && co_left(5, 7) == 0 && co_left(7, 5) == 2, "placement");
  CHECK(co_seal_parts(0) == 1 && co_seal_parts(16ull * kCoSealPieces + 15) == 1 && co_seal_parts(16ull * kCoSealPieces + 16) == 2, "parts");
  test_files(Run(60, [](uint64_t i) { return 8 + (i * 29) % 140; }, [](uint64_t i) { return i % 4 ? (i * 67) % 90 : 0; }), 700, 0, 0);
  test_files(Run(40, [](uint64_t) { return uint64_t(28); }, [](uint64_t) { return uint64_t(400); }), 436 * 7, 28, 400);
  test_files(Run(70, [](uint64_t) { return uint64_t(8); }, [](uint64_t) { return uint64_t(1); }), 17 * 9 + 3, 8, 1);
  test_files(Run(33, [](uint64_t) { return uint64_t(8); }, [](uint64_t) { return uint64_t(0); }), 1, 8, 0);
  printf("OK compaction output rules\n");
  return 0;
}
