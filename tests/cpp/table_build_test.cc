// tests/cpp/table_build_test.cc -- the table build's rules on the CPU
// (dlsm_amd/csrc/table_build.h) against a writer that restates
// TableBuilder_BACS::Add (table/table_builder_bacs.cpp:186-226) and BlockBuilder
// (table/block_builder.cc:74-127) on its own.  Every key and value lives in an
// allocation of its own so that a sanitizer sees a read past its end.
// Prints "OK" on success; exits non-zero with a message otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../dlsm_amd/csrc/table_build.h"

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

static void varint(std::string& o, uint64_t v) {  // PutVarint64 (util/coding.cc:82-94)
  for (; v >= 128; v >>= 7) o.push_back(static_cast<char>(v | 128));
  o.push_back(static_cast<char>(v));
}
static void put32(std::string& o, uint32_t v) { o.append(reinterpret_cast<const char*>(&v), 4); }
static std::string entry(const std::string& key, uint64_t off, uint64_t size) {
  std::string h, o(1, 0);
  varint(h, off), varint(h, size);
  varint(o, key.size()), varint(o, h.size());
  return o + key + h;
}
static std::string bytes(size_t n, unsigned seed) {
  std::string s(n, 0);
  for (size_t i = 0; i < n; i++) s[i] = static_cast<char>(seed = seed * 1103515245u + 12345u) >> 3;
  return s;
}
static std::unique_ptr<uint8_t[]> own(const std::string& s) {  // exactly s.size() bytes
  std::unique_ptr<uint8_t[]> p(new uint8_t[s.size()]);
  memcpy(p.get(), s.data(), s.size());
  return p;
}

static void test_entries() {
  for (int sh : {7, 14, 21, 28, 35})
    for (int d = -1; d <= 1; d++)
      for (size_t ks : {8, 127, 128, 136})
        for (int which = 0; which < 2; which++) {
          const uint64_t v = (uint64_t(1) << sh) + d, off = which ? 5 : v, size = which ? (v & 0xffffffffull) : 44;
          const std::string key = bytes(ks, sh + ks), want = entry(key, off, size);
          CHECK(tb_entry_len(ks, off, size) == want.size(), "length at 2^%d%+d, key %zu", sh, d, ks);
          CHECK(tb_varint_len(v) == static_cast<uint32_t>(sh / 7 + (d >= 0)), "varint length");
          // whole, and clipped on either side by a tile that starts c bytes into the entry and holds len bytes
          for (int64_t c : {int64_t(0), int64_t(1), int64_t(3), int64_t(ks + 2), int64_t(want.size() - 2)})
            for (int64_t len : {int64_t(want.size()) - c, int64_t(1), int64_t(7)}) {
              if (len <= 0 || c + len > static_cast<int64_t>(want.size())) continue;
              std::unique_ptr<uint8_t[]> tile(new uint8_t[len]);
              memset(tile.get(), 0xEE, len);
              tb_entry_write(tile.get(), len, -c, ks, off, size);
              const int64_t k0 = tb_entry_head(ks) - c;
              for (int64_t b = 0; b < static_cast<int64_t>(ks); b++) tb_put(tile.get(), len, k0 + b, key[b]);
              CHECK(memcmp(tile.get(), want.data() + c, len) == 0, "entry bytes at 2^%d%+d, key %zu, clip %ld+%ld", sh, d,
                    ks, static_cast<long>(c), static_cast<long>(len));
            }
        }
}

// n pairs with key and value lengths from the two functions: the region and
// the index contents by the plain writer, then both units over every cap.
template <class KL, class VL>
static void test_units(size_t n, KL klen, VL vlen) {
  std::vector<std::unique_ptr<uint8_t[]>> keep;
  std::vector<uint64_t> off(n + 1), ksrc(n), vsrc(n), koff(n + 1, 0), voff(n + 1, 0);
  std::vector<uint32_t> kl(n), es(n + 2, 0);
  std::string region, entries, kpack, vpack;
  for (size_t i = 0; i < n; i++) {
    const std::string k = bytes(klen(i), 7 * i + 1), v = bytes(vlen(i), 11 * i + 2);
    off[i] = region.size();
    es[i] = entries.size();
    entries += entry(k, off[i], 8 + k.size() + v.size());
    put32(region, k.size());
    put32(region, v.size());
    region += k + v;
    keep.push_back(own(k));
    ksrc[i] = reinterpret_cast<uint64_t>(keep.back().get());
    keep.push_back(own(v));
    vsrc[i] = reinterpret_cast<uint64_t>(keep.back().get());
    kl[i] = k.size();
    kpack += k;
    vpack += v;
    koff[i + 1] = kpack.size();
    voff[i + 1] = vpack.size();
  }
  off[n] = region.size();
  es[n] = n;
  const auto kp = own(kpack), vp = own(vpack);
  const TbWindowView win{off.data(), ksrc.data(), vsrc.data(), kl.data()};
  const TbSource src{kp.get(), koff.data(), vp.get(), voff.data(), 0, 0, off.data()};
  const uint64_t total = region.size();
  for (uint64_t cap : {total, total - 1, total / 2 + 5, uint64_t(17), uint64_t(16)})
    for (int acc = 0; acc < 2; acc++) {
      if (cap > total) continue;
      std::vector<uint8_t> out((cap + 15) / 16 * 16 + 16, 0xEE);
      for (uint64_t u = 0; u < cap; u += 16)
        acc ? tb_region_unit(src, n, u, cap, out.data() + u) : tb_region_unit(win, n, u, cap, out.data() + u);
      CHECK(memcmp(out.data(), region.data(), cap) == 0, "region bytes, n %zu cap %llu", n, (unsigned long long)cap);
      for (size_t p = cap; p < out.size(); p++) CHECK(out[p] == 0xEE, "a write past the cap at %zu", p);
    }
  std::string contents = entries;
  for (size_t i = 0; i < n; i++) put32(contents, es[i]);
  put32(contents, n);
  const uint64_t E = entries.size(), ctot = contents.size();
  for (uint64_t q0 : {uint64_t(0), uint64_t(E / 32 * 16)}) {
    const auto tile = own(entries.substr(q0));  // content bytes [q0, E): nothing behind E is readable
    for (uint64_t cap : {ctot, ctot - 1, ctot - 5, E + 2, E, E > 20 ? E - 3 : E}) {
      std::vector<uint8_t> out((ctot + 15) / 16 * 16 + 16, 0xEE);
      for (uint64_t q = q0; q < cap; q += 16) tb_index_unit(tile.get(), q0, es.data(), E, ctot, q, cap, out.data() + q);
      CHECK(cap <= q0 || memcmp(out.data() + q0, contents.data() + q0, cap - q0) == 0, "index bytes, n %zu cap %llu E %llu",
            n, (unsigned long long)cap, (unsigned long long)E);
      for (size_t p = cap > q0 ? cap : q0; p < out.size(); p++) CHECK(out[p] == 0xEE, "a write past the cap at %zu", p);
    }
  }
}

static void test_chunks() {
  for (unsigned seed = 1; seed < 40; seed++) {
    const size_t n = 1 + seed * 5;
    std::vector<uint64_t> off(n + 1, 0);
    unsigned r = seed;
    for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + 16 + ((r = r * 1103515245u + 12345u) >> 8) % 300;
    for (uint64_t cb : {uint64_t(1), uint64_t(16), uint64_t(315), uint64_t(1000), off[n / 2], off[n / 2] - 1, off[n], ~uint64_t(0)})
      for (uint64_t a = 0; a < n; a++) {
        uint64_t j = a + 1;  // the greedy loop: pair j stays while the chunk's bytes with it are within cb
        while (j < n && off[j + 1] - off[a] <= cb) j++;
        bool over;
        CHECK(tb_chunk_next(off.data(), n, a, cb, &over) == j, "successor of %llu under %llu", (unsigned long long)a,
              (unsigned long long)cb);
        CHECK(over == (off[a + 1] - off[a] > cb), "oversize");
      }
  }
}

int main() {
  test_entries();
  // a key / value boundary and a pair boundary at every alignment within a unit; segments below and above 16 bytes
  for (size_t k0 = 8; k0 < 8 + 16; k0++) test_units(40, [&](size_t i) { return k0 + i % 3; }, [&](size_t i) { return (i * 5) % 23; });
  test_units(30, [](size_t i) { return 8 + (i * 29) % 140; }, [](size_t i) { return i % 4 ? (i * 67) % 90 : 0; });
  test_units(25, [](size_t) { return size_t(8); }, [](size_t) { return size_t(0); });
  test_units(12, [](size_t) { return size_t(28); }, [](size_t) { return size_t(400); });
  test_units(1, [](size_t) { return size_t(8); }, [](size_t) { return size_t(1); });
  test_chunks();
  printf("OK table build rules\n");
  return 0;
}
