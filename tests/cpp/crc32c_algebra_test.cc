// tests/cpp/crc32c_algebra_test.cc -- the host-callable half of
// dlsm_amd/csrc/crc32c_dev.h on the CPU: known answers, the table of squares,
// x^bits, the word step against the byte step, the concatenation identity and
// the leading-zero rule at the lengths where a piece, a pass and a tail meet,
// and Mask.  Stand-alone: prints OK and returns 0, or the first failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../dlsm_amd/csrc/crc32c_dev.h"

namespace c = dlsm::crc32c;

static int g_fail = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      if (g_fail++ < 20) {                   \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);            \
        std::printf("\n");                   \
      }                                      \
    }                                        \
  } while (0)

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // splitmix64
  uint64_t z = (g_seed += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return static_cast<uint32_t>((z ^ (z >> 31)) >> 16);
}

static uint32_t raw_of(const std::vector<uint8_t>& d, uint32_t r = 0) {
  for (uint8_t b : d) r = c::raw_byte(r, b);
  return r;
}

// x^bits by a square-and-multiply of its own: squares made on the way, no table.
static uint32_t pow_ref(uint64_t bits) {
  uint32_t r = 0x80000000u, sq = 0x40000000u;
  for (; bits; bits >>= 1, sq = c::mulmod(sq, sq))
    if (bits & 1u) r = c::mulmod(r, sq);
  return r;
}

int main() {
  const c::XPow xp = c::make_xpow();

  // util/crc32c_test.cc:12-40 (RFC 3720 B.4), as tests/test_oracle_golden.py pins them
  {
    std::vector<uint8_t> z(32, 0), f(32, 0xff), up(32), down(32);
    for (int i = 0; i < 32; i++) {
      up[i] = static_cast<uint8_t>(i);
      down[i] = static_cast<uint8_t>(31 - i);
    }
    CHECK(c::value(raw_of(z), 32, xp) == 0x8a9136aau, "zeros: %08x", c::value(raw_of(z), 32, xp));
    CHECK(c::value(raw_of(f), 32, xp) == 0x62a8ab43u, "ones: %08x", c::value(raw_of(f), 32, xp));
    CHECK(c::value(raw_of(up), 32, xp) == 0x46dd794eu, "ascending: %08x", c::value(raw_of(up), 32, xp));
    CHECK(c::value(raw_of(down), 32, xp) == 0x113fdb5cu, "descending: %08x", c::value(raw_of(down), 32, xp));
  }

  // the table of squares
  CHECK(xp.p[0] == 0x40000000u, "p[0]");
  for (int k = 0; k + 1 < 40; k++) CHECK(xp.p[k + 1] == c::mulmod(xp.p[k], xp.p[k]), "p[%d] is not p[%d] squared", k + 1, k);
  CHECK(xp.p[3] == c::raw_byte(0x80000000u, 0), "p[3] %08x, a byte step of x^0 %08x", xp.p[3], c::raw_byte(0x80000000u, 0));

  // x^bits
  {
    uint32_t r = 0x80000000u;
    for (uint64_t bits = 0; bits <= 2100; bits++, r = c::mulmod(r, xp.p[0]))
      CHECK(c::xpow(xp, bits) == r, "x^%llu: %08x, by single steps %08x", (unsigned long long)bits, c::xpow(xp, bits), r);
    const uint64_t big[] = {8ull * 65536, 8ull * ((1ull << 32) + 5), (1ull << 39) + 8};
    for (uint64_t bits : big)
      CHECK(c::xpow(xp, bits) == pow_ref(bits), "x^%llu: %08x, reference %08x", (unsigned long long)bits, c::xpow(xp, bits), pow_ref(bits));
  }

  // the word step over the host-filled tables
  {
    std::vector<uint32_t> T(1024);
    c::fill_tables(T.data());
    for (int i = 0; i < 1000; i++) {
      const uint32_t r = rnd(), w = rnd();
      uint32_t b = r;
      for (int j = 0; j < 4; j++) b = c::raw_byte(b, (w >> (8 * j)) & 0xffu);
      CHECK(c::raw_word(r, w, T.data()) == b, "word step r %08x w %08x: %08x, four byte steps %08x", r, w, c::raw_word(r, w, T.data()), b);
    }
  }

  // r(A||B) = r(A) x^(8|B|) ^ r(B), r(0^z || D) = r(D), and Value through both
  {
    const size_t lens[] = {0, 1, 15, 16, 17, 4096};
    for (size_t la : lens)
      for (size_t lb : lens) {
        std::vector<uint8_t> A(la), B(lb);
        for (auto& x : A) x = static_cast<uint8_t>(rnd());
        for (auto& x : B) x = static_cast<uint8_t>(rnd());
        std::vector<uint8_t> AB(A);
        AB.insert(AB.end(), B.begin(), B.end());
        const uint32_t ra = raw_of(A), rb = raw_of(B), rab = raw_of(AB);
        CHECK(rab == (c::mulmod(ra, c::xpow(xp, static_cast<uint64_t>(lb) << 3)) ^ rb), "concatenation |A| %zu |B| %zu", la, lb);
        // the standard register (starts at all ones, inverted at the end) over A||B
        CHECK(c::value(rab, la + lb, xp) == ~raw_of(AB, 0xffffffffu), "value |A| %zu |B| %zu", la, lb);
        for (size_t z : lens) {
          std::vector<uint8_t> ZAB(z, 0);
          ZAB.insert(ZAB.end(), AB.begin(), AB.end());
          CHECK(raw_of(ZAB) == rab, "%zu leading zeros, |A| %zu |B| %zu", z, la, lb);
        }
      }
  }

  // Mask of the first known answer: the value dlsm_amd.crc32c_mask gives for it
  CHECK(c::mask(0x8a9136aau) == 0x0fd7fffau, "mask: %08x", c::mask(0x8a9136aau));

  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
