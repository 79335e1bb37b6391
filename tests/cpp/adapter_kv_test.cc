// tests/cpp/adapter_kv_test.cc -- dlsm_adapter::TableData: ReadPair (the
// per-Get path) and ReadBatch against a walk over the pairs the regions were
// written from.  Without an argument: the all-host path (host::ReadBatch, and
// ReadBatch with whatever this machine has); with "gpu": ReadBatch on the
// device, then under an injected fault (the counted host fallback).  The
// writer restates TableBuilder_BACS::Add (table/table_builder_bacs.cpp:221-226).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "dlsm_bloom_adapter.hpp"

using dlsm_adapter::Slice;
using dlsm_adapter::TableData;

#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); \
      printf(__VA_ARGS__);                              \
      printf("\n");                                     \
      exit(1);                                          \
    }                                                   \
  } while (0)

struct Item {
  std::string user;
  uint8_t state_in, state_out;
  dlsm_kv_handle h;
  std::string value;  // the expected value (empty unless FOUND)
};

struct Fixture {
  std::vector<std::vector<std::string>> chunks;  // per file
  std::vector<std::vector<Slice>> slices;
  std::vector<Item> items;
  std::string kb;
  std::vector<uint64_t> offs;
  dlsm_keyset ks;
  std::vector<uint32_t> gets;
};

static std::string pair_of(const std::string& user, uint64_t seq, uint8_t type, const std::string& value) {
  std::string k = user;
  const uint64_t t = (seq << 8) | type;
  k.append(reinterpret_cast<const char*>(&t), 8);
  const uint32_t ks = static_cast<uint32_t>(k.size()), vs = static_cast<uint32_t>(value.size());
  std::string o(reinterpret_cast<const char*>(&ks), 4);
  o.append(reinterpret_cast<const char*>(&vs), 4);
  return o + k + value;
}

// Three files (the second without data); file 0 in chunks of at most 200
// bytes, file 2 in one chunk; FOUND items for every pair, then one item per way
// of going wrong and pass-through states with wild handles.
static void make_fixture(Fixture* F) {
  std::mt19937 rng(5);
  F->chunks.resize(3);
  for (uint32_t f : {0u, 2u}) {
    F->chunks[f].push_back(std::string());
    uint64_t done = 0;
    for (int j = 0; j < 120; j++) {
      char ub[32];
      snprintf(ub, sizeof ub, "user%u-%0*d", f, 1 + j % 9, j);
      std::string v(rng() % (j % 10 == 0 ? 500 : 60), '\0');
      for (char& c : v) c = static_cast<char>(rng());
      const uint8_t type = j % 13 == 5 ? 0 : 1;
      const std::string p = pair_of(ub, 10 + j, type, v);
      if (f == 0 && !F->chunks[f].back().empty() && F->chunks[f].back().size() + p.size() > 200) {
        done += F->chunks[f].back().size();
        F->chunks[f].push_back(std::string());
      }
      const dlsm_kv_handle h{done + F->chunks[f].back().size(), static_cast<uint32_t>(p.size()), f};
      F->chunks[f].back() += p;
      F->items.push_back(Item{ub, DLSM_GET_FOUND, static_cast<uint8_t>(type ? DLSM_GET_FOUND : DLSM_GET_DELETED), h,
                              type ? v : std::string()});
    }
  }
  CHECK(F->chunks[0].size() > 10, "file 0 is in many chunks");
  const Item good = F->items[3];
  auto bad = [&](dlsm_kv_handle h, const std::string& user) {
    F->items.push_back(Item{user, DLSM_GET_FOUND, DLSM_GET_CORRUPT, h, ""});
  };
  bad(dlsm_kv_handle{good.h.offset, good.h.size, 1}, good.user);               // no data held
  bad(dlsm_kv_handle{good.h.offset, good.h.size, 3}, good.user);               // file >= n_files
  bad(dlsm_kv_handle{uint64_t(1) << 40, good.h.size, 0}, good.user);           // past every chunk
  bad(dlsm_kv_handle{good.h.offset, good.h.size + 1, 0}, good.user);           // a length mismatch (or a straddle)
  bad(dlsm_kv_handle{good.h.offset, good.h.size - 1, 0}, good.user);
  bad(dlsm_kv_handle{good.h.offset, 15, 0}, good.user);                        // size < 16
  bad(dlsm_kv_handle{good.h.offset + 1, good.h.size - 1, 0}, good.user);       // not a pair's start
  bad(good.h, good.user + "x");                                                // user-key mismatch
  for (uint8_t s : {DLSM_GET_NOTFOUND, DLSM_GET_DELETED, DLSM_GET_CORRUPT})
    F->items.push_back(Item{"any", s, s, dlsm_kv_handle{~uint64_t(0) - 5, 0xfffffff0u, 0xffffffffu}, ""});
  std::shuffle(F->items.begin(), F->items.end(), rng);
  for (auto& f : F->chunks) {
    F->slices.push_back({});
    for (auto& c : f) F->slices.back().push_back(Slice(c));
  }
  F->slices[1].clear();
  F->offs.push_back(0);
  for (const Item& it : F->items) {
    F->kb += it.user;
    F->offs.push_back(F->kb.size());
  }
  F->ks = dlsm_keyset{reinterpret_cast<const uint8_t*>(F->kb.data()), F->offs.data(), 0, 0, F->items.size()};
}

struct Arrays {
  std::vector<uint8_t> state, values;
  std::vector<uint64_t> off;
  uint64_t bad = 77;
  bool operator==(const Arrays& o) const { return state == o.state && values == o.values && off == o.off && bad == o.bad; }
};

static Arrays fresh(const Fixture& F, uint64_t cap, uint64_t values_cap) {
  Arrays A;
  A.state.assign(cap + 8, 0xee);
  for (uint64_t i = 0; i < std::min<uint64_t>(cap, F.items.size()); i++) A.state[i] = F.items[i].state_in;
  A.off.assign(cap + 1 + 8, 0x5a5a5a5a5a5a5a5aull);
  A.values.assign(values_cap + 64, 0xcd);
  return A;
}

static std::vector<dlsm_kv_handle> handles(const Fixture& F) {
  std::vector<dlsm_kv_handle> h;
  for (const Item& it : F.items) h.push_back(it.h);
  return h;
}

// The walk's arrays.
static Arrays walk(const Fixture& F, uint64_t m, uint64_t cap, uint64_t values_cap) {
  Arrays A = fresh(F, cap, values_cap);
  std::string blob;
  A.bad = 0;
  for (uint64_t i = 0; i < m; i++) {
    A.off[i] = blob.size();
    A.state[i] = F.items[i].state_out;
    A.bad += F.items[i].state_in == DLSM_GET_FOUND && F.items[i].state_out == DLSM_GET_CORRUPT;
    blob += F.items[i].value;
  }
  A.off[m] = blob.size();
  memcpy(A.values.data(), blob.data(), std::min<uint64_t>(blob.size(), values_cap));
  return A;
}

static uint64_t total_of(const Fixture& F, uint64_t m) {
  uint64_t t = 0;
  for (uint64_t i = 0; i < m; i++) t += F.items[i].value.size();
  return t;
}

static void run_batch(TableData* td, dlsm_ctx* ctx, const Fixture& F, uint64_t cap, const uint64_t* count, uint64_t values_cap,
                      int fault, bool expect_device) {
  const uint64_t m = count ? std::min(*count, cap) : cap;
  Arrays got = fresh(F, cap, values_cap);
  const std::vector<dlsm_kv_handle> h = handles(F);
  uint64_t fb0 = 0, fb1 = 0;
  dlsm_fallback_stats(ctx, &fb0, nullptr);
  if (fault) CHECK(dlsm_ctx_set_option(ctx, DLSM_OPT_FAULT_INJECT, fault) == DLSM_OK, "inject");
  const int st = td->ReadBatch(F.ks, nullptr, count, cap, got.state.data(), h.data(), got.off.data(), got.values.data(),
                               values_cap, &got.bad);
  if (fault) CHECK(dlsm_ctx_set_option(ctx, DLSM_OPT_FAULT_INJECT, 0) == DLSM_OK, "inject off");
  CHECK(st == DLSM_OK, "ReadBatch: %d", st);
  if (expect_device) {
    CHECK(td->status() == (fault ? -fault : DLSM_OK), "device status %d", td->status());
    dlsm_fallback_stats(ctx, &fb1, nullptr);
    CHECK(fb1 - fb0 == (fault ? 1u : 0u), "fallbacks %llu", (unsigned long long)(fb1 - fb0));
  }
  CHECK(got == walk(F, m, cap, values_cap), "arrays differ from the walk (cap %llu, m %llu, values_cap %llu, fault %d)",
        (unsigned long long)cap, (unsigned long long)m, (unsigned long long)values_cap, fault);
}

static void test_host() {
  Fixture F;
  make_fixture(&F);
  const uint64_t n = F.items.size();
  TableData* td = TableData::FromChunks(F.slices);
  CHECK(td && td->n_files() == 3, "FromChunks");
  for (const Item& it : F.items) {  // ReadPair against the walk
    std::string v = "untouched";
    uint8_t st = it.state_in;
    CHECK(td->ReadPair(it.h, Slice(it.user), &v, &st) == DLSM_OK, "ReadPair");
    CHECK(st == it.state_out && v == (st == DLSM_GET_FOUND ? it.value : "untouched"), "ReadPair: state %d, walk %d", st,
          it.state_out);
  }
  CHECK(td->ReadPair(F.items[0].h, Slice("k", 1), nullptr, nullptr) == DLSM_E_ARG, "NULL state");
  const std::vector<dlsm_kv_handle> h = handles(F);
  // host::ReadBatch against the walk; the per-task form through gets
  std::vector<std::vector<dlsm_data_chunk>> files(3);
  for (size_t f = 0; f < 3; f++)
    for (const Slice& c : F.slices[f]) files[f].push_back(dlsm_data_chunk{reinterpret_cast<const uint8_t*>(c.data()), c.size()});
  const uint64_t total = total_of(F, n);
  const uint64_t below = 5, above = n + 9;
  for (uint64_t cap : {n, n - 1, uint64_t(1)})
    for (const uint64_t* count : {static_cast<const uint64_t*>(nullptr), &below, &above})
      for (uint64_t vc : {total, total - 1, total / 2, uint64_t(0)}) {
        const uint64_t m = count ? std::min(*count, cap) : cap;
        Arrays got = fresh(F, cap, vc);
        CHECK(dlsm_adapter::host::ReadBatch(files, F.ks, nullptr, count, cap, got.state.data(), h.data(), got.off.data(),
                                            got.values.data(), vc, &got.bad) == DLSM_OK,
              "host ReadBatch");
        CHECK(got == walk(F, m, cap, vc), "host ReadBatch differs from the walk");
        run_batch(td, nullptr, F, cap, count, vc, 0, false);  // the device, or (no device) the host: the walk's either way
      }
  {
    std::vector<uint32_t> ident(n);
    for (uint32_t i = 0; i < n; i++) ident[i] = i;
    ident[7] = static_cast<uint32_t>(n);  // a gets entry >= keys.n
    Arrays got = fresh(F, n, total), want = walk(F, n, n, total);
    CHECK(dlsm_adapter::host::ReadBatch(files, F.ks, ident.data(), nullptr, n, got.state.data(), h.data(), got.off.data(),
                                        got.values.data(), total, &got.bad) == DLSM_OK,
          "host ReadBatch with gets");
    if (F.items[7].state_in == DLSM_GET_FOUND) {
      CHECK(got.state[7] == DLSM_GET_CORRUPT && got.off[n] == want.off[n] - F.items[7].value.size(), "a key index past the batch");
    } else {
      CHECK(got == want, "pass-through");
    }
  }
  uint8_t st = DLSM_GET_FOUND;
  uint64_t off[2];
  CHECK(td->ReadBatch(F.ks, nullptr, nullptr, 1, &st, nullptr, off, nullptr, 0, nullptr) == DLSM_E_ARG, "bad arguments stay bad");
  delete td;
  // the C ABI's checks that need no device
  {
    dlsm_tabledata* t = reinterpret_cast<dlsm_tabledata*>(1);
    const uint32_t begin[2] = {0, 0};
    CHECK(dlsm_tabledata_create(nullptr, nullptr, begin, 1, 0, &t) == DLSM_E_ARG && t == nullptr, "NULL context");
    CHECK(dlsm_tabledata_destroy(nullptr) == DLSM_OK && dlsm_tabledata_size(nullptr, nullptr, nullptr, nullptr) == DLSM_E_ARG,
          "NULL data");
    CHECK(dlsm_kv_read_dev(nullptr, nullptr, &F.ks, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr) ==
              DLSM_E_ARG && dlsm_kv_read(nullptr, nullptr, &F.ks, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                                         0, nullptr) == DLSM_E_ARG,
          "read NULL");
    CHECK(dlsm_kv_pair_read(nullptr, 1, &h[0], nullptr, 0, &st, nullptr, nullptr) == DLSM_E_ARG, "chunks NULL");
    CHECK(dlsm_kv_read_stats(nullptr, nullptr, nullptr) == DLSM_E_ARG, "stats NULL");
    CHECK(dlsm_kv_read_chunk() >= 64 && dlsm_kv_read_span() % 16 == 0 && dlsm_kv_read_span() >= 16, "sizes");
  }
  printf("OK adapter kv host\n");
}

static void test_gpu() {
  dlsm_ctx* ctx = nullptr;
  CHECK(dlsm_ctx_create(0, &ctx) == DLSM_OK, "context");
  Fixture F;
  make_fixture(&F);
  const uint64_t n = F.items.size(), total = total_of(F, n);
  TableData* td = TableData::FromChunks(F.slices, ctx);
  CHECK(td != nullptr, "FromChunks");
  const uint64_t below = 5, above = n + 9;
  for (uint64_t cap : {n, n - 1, uint64_t(1)})
    for (const uint64_t* count : {static_cast<const uint64_t*>(nullptr), &below, &above})
      for (uint64_t vc : {total, total - 1, total / 2, uint64_t(0)}) run_batch(td, ctx, F, cap, count, vc, 0, true);
  run_batch(td, ctx, F, n, nullptr, total, 4, true);
  run_batch(td, ctx, F, n, nullptr, total, 0, true);  // the device path is back
  // a fault at the first call: the tables' upload itself is refused, the host still answers
  TableData* t2 = TableData::FromChunks(F.slices, ctx);
  run_batch(t2, ctx, F, n, nullptr, total - 3, 5, true);
  run_batch(t2, ctx, F, n, nullptr, total - 3, 0, true);
  uint64_t fb = 9;
  dlsm_fallback_stats(ctx, &fb, nullptr);
  CHECK(fb == 2, "only the injected faults fell back: %llu", (unsigned long long)fb);
  delete t2;
  delete td;
  dlsm_ctx_destroy(ctx);
  printf("OK adapter kv gpu\n");
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "gpu") == 0) test_gpu();
  else test_host();
  return 0;
}
