// The adapter's sealed-block surface (include/dlsm_bloom_adapter.hpp) against
// the oracle (test infrastructure): FullFilterBlockBuilder::FinishBlock,
// host::ReadFilterBlock and FullFilterBlockReader::FromBlock.  Built and run
// by tests/test_adapter_block.py.
//
//   adapter_block_test cpu   builders with no context: every build falls back
//                            to the host loop, sealed on the host; too-small
//                            slots; ReadFilterBlock's codes in the reference's
//                            order (table/format.cc:389-441); FromBlock
//   adapter_block_test gpu   FinishBlock through every builder form
//                            (reference signature, staged keys,
//                            hash_in_addkey, batcher with DLSM_BATCH_SEALED)
//                            with no fallback counted; FromBlock + KeysMayMatch
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dlsm_bloom_adapter.hpp"

extern "C" {
int64_t orc_full_build(const uint8_t*, const uint64_t*, uint32_t, uint64_t, int, uint8_t*, uint64_t);
int orc_full_key_may_match(const uint8_t*, uint64_t, const uint8_t*, size_t);
void orc_dbbench_key(uint64_t v, int key_size, uint8_t* out);
uint32_t orc_crc32c_extend(uint32_t crc, const uint8_t* p, uint64_t n);
uint32_t orc_crc32c_mask(uint32_t crc);
}

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      return 1;                                               \
    }                                                         \
  } while (0)

using dlsm_adapter::FilterSlot;
using dlsm_adapter::FullFilterBlockBuilder;
using dlsm_adapter::FullFilterBlockReader;
using dlsm_adapter::Slice;

static std::string keys_of(int n, int seed) {
  std::string flat(static_cast<size_t>(n) * 20, '\0');
  for (int i = 0; i < n; i++)
    orc_dbbench_key(static_cast<uint64_t>(i) * 7 + 3 + seed, 20, reinterpret_cast<uint8_t*>(&flat[20 * i]));
  return flat;
}

// The oracle's sealed block of arbitrary contents.
static std::string seal(const std::string& contents) {
  std::string b = contents;
  b.push_back('\0');
  const uint32_t m = orc_crc32c_mask(orc_crc32c_extend(0, reinterpret_cast<const uint8_t*>(b.data()), b.size()));
  for (int i = 0; i < 4; i++) b.push_back(static_cast<char>(m >> (8 * i)));
  return b;
}

static std::string oracle_filter(const std::string& flat, int n, int bpk) {
  std::vector<uint8_t> out(static_cast<size_t>(n) * bpk / 8 + 256);
  const int64_t len = orc_full_build(reinterpret_cast<const uint8_t*>(flat.data()), nullptr, 20, n, bpk, out.data(),
                                     out.size());
  return len < 0 ? std::string() : std::string(reinterpret_cast<char*>(out.data()), static_cast<size_t>(len));
}

static std::string match_all(int bpk) {
  std::string f(64, '\xff');
  f.push_back(static_cast<char>(dlsm_bloom_full_num_probes(bpk)));
  f.append("\x01\0\0\0", 4);
  return f;
}

template <class B>
static void add_all(B& b, const std::string& flat, int n) {
  b.RestartBlock(0);
  for (int i = 0; i < n; i++) b.AddKey(Slice(flat.data() + 20 * i, 20));
}

static uint64_t process_fallbacks() {
  uint64_t n = 0;
  dlsm_fallback_stats(nullptr, nullptr, &n);
  return n;
}

static int cpu_part() {
  const int sizes[] = {0, 1, 7, 5000};
  for (int hash = 0; hash < 2; hash++) {
    dlsm_adapter::BuilderOptions opt;
    opt.hash_in_addkey = hash != 0;
    for (int n : sizes) {
      const std::string flat = keys_of(n, n);
      const std::string want = seal(oracle_filter(flat, n, 10));
      std::vector<char> slot(want.size() + 100, '\x11');
      FilterSlot mr{slot.data(), slot.size()};
      FullFilterBlockBuilder b(&mr, 10, nullptr, opt);  // no context: the host loop builds and seals
      add_all(b, flat, n);
      b.FinishBlock();
      CHECK(b.status() == DLSM_OK && b.fell_back());
      CHECK(b.result.size() == want.size() && std::memcmp(b.result.data(), want.data(), want.size()) == 0);
      CHECK(slot[want.size()] == '\x11');  // nothing past the block
      // Finish itself is unchanged: the bare filter
      add_all(b, flat, n);
      b.Finish();
      CHECK(b.status() == DLSM_OK && b.result.size() == want.size() - 5);
      CHECK(std::memcmp(b.result.data(), want.data(), want.size() - 5) == 0);
      // a slot too small by 1..5 bytes holds the filter but not its trailer:
      // the sealed match-everything filter (74 bytes) when that fits, else an
      // empty result, with DLSM_E_CAPACITY either way
      const std::string all = seal(match_all(10));
      CHECK(all.size() == 74);
      for (size_t d = 1; d <= 5; d++) {
        FilterSlot small{slot.data(), want.size() - d};
        FullFilterBlockBuilder s(&small, 10, nullptr, opt);
        add_all(s, flat, n);
        s.FinishBlock();
        CHECK(s.status() == DLSM_E_CAPACITY);
        if (small.length >= all.size()) {
          CHECK(s.result.size() == all.size() && std::memcmp(s.result.data(), all.data(), all.size()) == 0);
          Slice c;
          CHECK(dlsm_adapter::host::ReadFilterBlock(s.result, true, &c) == DLSM_BLOCK_OK);
          FullFilterBlockReader r(c, nullptr);
          CHECK(r.status() == DLSM_OK && r.KeyMayMatch(Slice("anything", 8)));
        } else {
          CHECK(s.result.size() == 0);
        }
      }
    }
  }
  // ReadFilterBlock: the reference's order of checks
  {
    const std::string flat = keys_of(5000, 1);
    const std::string filt = oracle_filter(flat, 5000, 10);
    const std::string blk = seal(filt);
    Slice c;
    for (size_t m = 0; m < 5; m++) {
      CHECK(dlsm_adapter::host::ReadFilterBlock(Slice(blk.data(), m), true, &c) == DLSM_BLOCK_SHORT);
      CHECK(dlsm_adapter::host::ReadFilterBlock(Slice(blk.data(), m), false, &c) == DLSM_BLOCK_SHORT);
    }
    CHECK(dlsm_adapter::host::ReadFilterBlock(Slice(blk), true, &c) == DLSM_BLOCK_OK);
    CHECK(c.data() == blk.data() && c.size() == filt.size());
    CHECK(dlsm_adapter::host::ReadFilterBlock(Slice(seal("")), true, &c) == DLSM_BLOCK_OK && c.size() == 0);
    const size_t n = filt.size();
    const size_t flips[] = {0, n / 2, n - 1, n + 1, n + 2, n + 3, n + 4};
    for (size_t i : flips) {
      std::string bad = blk;
      bad[i] ^= 0x40;
      CHECK(dlsm_adapter::host::ReadFilterBlock(Slice(bad), true, &c) == DLSM_BLOCK_CHECKSUM);
      CHECK(dlsm_adapter::host::ReadFilterBlock(Slice(bad), false, &c) == DLSM_BLOCK_OK);
    }
    std::string bad = blk;
    bad[n] = 1;  // the type byte alone: the checksum is checked first
    CHECK(dlsm_adapter::host::ReadFilterBlock(Slice(bad), true, &c) == DLSM_BLOCK_CHECKSUM);
    CHECK(dlsm_adapter::host::ReadFilterBlock(Slice(bad), false, &c) == DLSM_BLOCK_TYPE);
    // a compressed-type block with a correct crc over it
    std::string typed = filt;
    typed.push_back('\x01');
    const uint32_t m = orc_crc32c_mask(orc_crc32c_extend(0, reinterpret_cast<const uint8_t*>(typed.data()), typed.size()));
    for (int i = 0; i < 4; i++) typed.push_back(static_cast<char>(m >> (8 * i)));
    CHECK(dlsm_adapter::host::ReadFilterBlock(Slice(typed), true, &c) == DLSM_BLOCK_TYPE);
    // FromBlock: the checks, then the reader as today (single keys on the host)
    int st = -1;
    FullFilterBlockReader* r = FullFilterBlockReader::FromBlock(Slice(blk), true, nullptr, &st);
    CHECK(r && st == DLSM_BLOCK_OK && r->status() == DLSM_OK && r->filter_content.size() == filt.size());
    const std::string other = keys_of(3000, 999);
    for (int i = 0; i < 3000; i++) {
      CHECK(r->KeyMayMatch(Slice(flat.data() + 20 * i, 20)));
      const bool want = orc_full_key_may_match(reinterpret_cast<const uint8_t*>(filt.data()), filt.size(),
                                               reinterpret_cast<const uint8_t*>(other.data() + 20 * i), 20) != 0;
      CHECK(r->KeyMayMatch(Slice(other.data() + 20 * i, 20)) == want);
    }
    delete r;
    CHECK(FullFilterBlockReader::FromBlock(Slice(bad), true, nullptr, &st) == nullptr && st == DLSM_BLOCK_CHECKSUM);
    CHECK(FullFilterBlockReader::FromBlock(Slice(bad), false, nullptr, &st) == nullptr && st == DLSM_BLOCK_TYPE);
    CHECK(FullFilterBlockReader::FromBlock(Slice(blk.data(), 3), true, nullptr) == nullptr);
  }
  std::printf("OK adapter block cpu\n");
  return 0;
}

struct IbvMrShaped {  // <infiniband/verbs.h> struct ibv_mr's fields
  void* context;
  void* pd;
  void* addr;
  size_t length;
  uint32_t handle, lkey, rkey;
};

static int gpu_part() {
  dlsm_ctx* ctx = nullptr;
  CHECK(dlsm_thread_ctx(&ctx) == DLSM_OK && ctx);
  dlsm_batcher* batcher = nullptr;
  CHECK(dlsm_batcher_create(dlsm_ctx_device(ctx), 1, 0, 8, &batcher) == DLSM_OK);
  const uint64_t fallbacks0 = process_fallbacks();
  const int sizes[] = {0, 1, 7, 20000, 153846};
  for (int n : sizes) {
    const std::string flat = keys_of(n, n);
    const std::string filt = oracle_filter(flat, n, 10);
    const std::string want = seal(filt);
    std::vector<char> slot(want.size() + 64);
    // form 0: the reference's signature (hash_entries_, the thread's context);
    // 1: staged keys; 2: hash_in_addkey; 3, 4: the same two through a batcher
    for (int form = 0; form < 5; form++) {
      std::fill(slot.begin(), slot.end(), '\x11');
      FilterSlot mr{slot.data(), slot.size()};
      IbvMrShaped ibv{nullptr, nullptr, slot.data(), slot.size(), 0, 0, 0};
      dlsm_adapter::BuilderOptions opt;
      opt.hash_in_addkey = form == 2 || form == 4;
      opt.batcher = form >= 3 ? batcher : nullptr;
      FullFilterBlockBuilder* b = form == 0 ? new FullFilterBlockBuilder(&ibv, 10)
                                            : new FullFilterBlockBuilder(&mr, 10, ctx, opt);
      add_all(*b, flat, n);
      b->FinishBlock();
      CHECK(b->status() == DLSM_OK && b->device_status() == DLSM_OK && !b->fell_back());
      CHECK(b->result.size() == want.size() && std::memcmp(b->result.data(), want.data(), want.size()) == 0);
      CHECK(slot[want.size()] == '\x11');
      // one byte short of the sealed block: the sealed match-everything filter
      if (want.size() - 1 >= 74) {
        FilterSlot small{slot.data(), want.size() - 1};
        IbvMrShaped sibv{nullptr, nullptr, slot.data(), want.size() - 1, 0, 0, 0};
        FullFilterBlockBuilder* s = form == 0 ? new FullFilterBlockBuilder(&sibv, 10)
                                              : new FullFilterBlockBuilder(&small, 10, ctx, opt);
        add_all(*s, flat, n);
        s->FinishBlock();
        CHECK(s->status() == DLSM_E_CAPACITY && s->result.size() == 74);
        Slice c;
        CHECK(dlsm_adapter::host::ReadFilterBlock(s->result, true, &c) == DLSM_BLOCK_OK && c.size() == 69);
        delete s;
      }
      delete b;
    }
    if (n == 0) continue;  // the reader rejects the 0-key filter (no lines to probe)
    int st = -1;
    FullFilterBlockReader* r = FullFilterBlockReader::FromBlock(Slice(want), true, ctx, &st);
    CHECK(r && st == DLSM_BLOCK_OK && r->status() == DLSM_OK);
    const int nq = 4000;
    const std::string probe = keys_of(nq, n / 2 + 1);
    std::vector<Slice> qs;
    for (int i = 0; i < nq; i++) qs.push_back(Slice(probe.data() + 20 * i, 20));
    std::vector<uint8_t> got(nq, 9);
    CHECK(r->KeysMayMatch(qs.data(), qs.size(), got.data()) == DLSM_OK && r->last_device_status() == DLSM_OK);
    for (int i = 0; i < nq; i++)
      CHECK(got[i] == (orc_full_key_may_match(reinterpret_cast<const uint8_t*>(filt.data()), filt.size(),
                                              reinterpret_cast<const uint8_t*>(probe.data() + 20 * i), 20) != 0));
    delete r;
  }
  CHECK(process_fallbacks() == fallbacks0);
  uint64_t batches = 0, jobs = 0;
  CHECK(dlsm_batcher_stats(batcher, &batches, &jobs, nullptr) == DLSM_OK && jobs >= 10);
  dlsm_batcher_destroy(batcher);
  std::printf("OK adapter block gpu\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "gpu") == 0) return gpu_part();
  return cpu_part();
}
