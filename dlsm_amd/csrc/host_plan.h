// dlsm_amd/csrc/host_plan.h -- the C ABI's host-side planning: what the
// kernels are handed (search orders, layouts, job tables, slice geometry),
// computed from plain arguments.  Pure host code: no device call, no
// environment, no context -- bloom_capi.hip fetches, allocates, uploads and
// launches around it, and tests/cpp/host_plan_test.cc runs it on the CPU.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/dlsm_bloom.h"
#include "bloom_internal.h"
#include "read_plan.h"

namespace dlsm {
namespace plan {

inline uint32_t ceil_div_u32(uint64_t a, uint64_t b) { return static_cast<uint32_t>((a + b - 1) / b); }

// A workspace laid out region by region, every region 256-byte aligned.
struct Layout {
  uint64_t at = 0;  // the bytes so far
  uint64_t take(uint64_t want) {
    const uint64_t off = at;
    at += (want + 255) & ~uint64_t(255);
    return off;
  }
  void region(uint64_t* off, uint64_t* bytes, uint64_t want) {
    *off = take(want);
    *bytes = want;
  }
};

inline KeyDesc to_desc(const dlsm_keyset& k) {
  KeyDesc d;
  d.bytes = k.bytes;
  d.offsets = k.offsets;
  d.n = k.n;
  d.key_len = k.key_len;
  d.suffix = k.suffix_len;
  return d;
}

// Slice width for the sliced build: the smallest 2^lgR (lgR in [9, 11]) that
// keeps every job at <= kMaxSlices slices, then narrower (down to 2^7 lines,
// 8 KiB) while the batch has fewer than two slice workgroups per CU -- a
// batch of dLSM-sized flush tables (153,846 keys, 3,005 lines) would
// otherwise leave most CUs idle.  Returns -1 if none fits.
inline int choose_build_lgR(const std::vector<uint32_t>& Ls) {
  auto slices = [&](int lg, uint64_t* total) {
    bool ok = true;
    *total = 0;
    for (uint32_t L : Ls) {
      const uint64_t n = (static_cast<uint64_t>(L) + (1u << lg) - 1) >> lg;
      ok = ok && n <= kMaxSlices;
      *total += std::max<uint64_t>(n, 1);
    }
    return ok;
  };
  uint64_t total = 0, t2 = 0;
  // the slice-workgroup count below which the slices narrow: two per CU
  constexpr uint64_t min_wgs = 2ull * kBuildSliceCUs;
  for (int lg = 9; lg <= 11; lg++) {  // widest-first search from 2^9 lines (32 KiB slices)
    if (!slices(lg, &total)) continue;
    while (lg > 7 && total < min_wgs && slices(lg - 1, &t2)) {
      lg--;
      total = t2;
    }
    return lg;
  }
  return -1;
}

// FullFilterBlockReader ctor checks (table/full_filter_block.cc:186-252) on the
// filter's 5-byte tail and total length.
inline int parse_tail(const uint8_t* tail, uint64_t len64, int* k_out, uint32_t* L_out, int* lg_out) {
  if (len64 < 5 || len64 > 0xffffffffull) return DLSM_E_CORRUPT;
  const int k = static_cast<int>(static_cast<int8_t>(tail[0]));
  if (k < 1) return DLSM_E_CORRUPT;  // the reference exit(1)s
  const uint32_t len = static_cast<uint32_t>(len64) - 5;
  const uint32_t L = uint32_t(tail[1]) | (uint32_t(tail[2]) << 8) | (uint32_t(tail[3]) << 16) |
                     (uint32_t(tail[4]) << 24);
  int lg;
  if (L * kCacheLineBytes == len) {
    // common case; L == 0 (empty filter) would make KeyMayMatch divide by 0,
    // and a wrapped product would index past the filter
    if (L == 0 || static_cast<uint64_t>(L) * kCacheLineBytes != len) return DLSM_E_CORRUPT;
    lg = 6;
  } else if (L == 0 || len % L != 0) {
    return DLSM_E_CORRUPT;  // the reference exit(1)s
  } else {
    lg = 0;  // log2_cache_line_size_ keeps its initialiser (full_filter_block.h:85)
  }
  *k_out = k;
  *L_out = L;
  *lg_out = lg;
  return DLSM_OK;
}

// ---- build job tables --------------------------------------------------------
// A host job table, the per-job chunk0s | slice0s (`starts`) and the totals
// the workspace is sized by.
template <typename Job>
struct JobTable {
  std::vector<Job> hj;
  std::vector<uint32_t> starts;
  uint64_t entry = 0, tabw = 0;
  uint32_t chunk = 0, slice = 0;
};

// The full-filter build's job table: Ls the speculative line counts, lgR the
// slice width (choose_build_lgR) when sliced_ok.
inline JobTable<FullJobDev> plan_full_jobs(const dlsm_build_job* jobs, int n_jobs, int bits_per_key,
                                           uint64_t* out_len_dev, const std::vector<uint32_t>& Ls, int lgR,
                                           bool sliced_ok, bool exact) {
  JobTable<FullJobDev> T;
  T.hj.resize(n_jobs);
  T.starts.resize(2 * n_jobs);
  const int k = full_num_probes(bits_per_key);
  for (int j = 0; j < n_jobs; j++) {
    const dlsm_build_job& b = jobs[j];
    FullJobDev& d = T.hj[j];
    d.keys = to_desc(b.keys);
    d.out = b.out;
    d.out_cap = b.out_cap;
    d.out_len = out_len_dev + j;
    d.entry0 = T.entry;
    d.n_chunks = ceil_div_u32(b.keys.n, kBuildChunk);
    d.chunk0 = T.chunk;
    d.L_spec = Ls[j];
    d.magic_spec = Ls[j] ? fastmod_magic(Ls[j]) : 0;
    d.n_slices = sliced_ok ? std::max<uint32_t>(1, ceil_div_u32(Ls[j], 1ull << lgR)) : 1;
    d.slice0 = T.slice;
    d.tab0 = T.tabw;
    d.k = k;
    d.bpk = bits_per_key;
    d.exact = exact ? 1 : 0;
    d.reserved = 0;
    T.starts[j] = T.chunk;
    T.starts[n_jobs + j] = T.slice;
    // chunk regions of kBuildRegion entries (buckets padded to 16-byte units)
    T.entry += static_cast<uint64_t>(d.n_chunks) * kBuildRegion;
    T.chunk += d.n_chunks;
    T.slice += d.n_slices;
    T.tabw += static_cast<uint64_t>(d.n_slices + 1) * d.n_chunks;
  }
  return T;
}

// At most G job groups of about equal chunk counts, as cut points into the
// jobs: cut[0] = 0 < ... < cut.back() = n_jobs (starts: the jobs' chunk0s).
inline std::vector<int> job_group_cuts(const std::vector<uint32_t>& starts, uint32_t chunk, int n_jobs, int G) {
  std::vector<int> cut(1, 0);
  for (int j = 1; j < n_jobs && static_cast<int>(cut.size()) < G; j++)
    if (static_cast<uint64_t>(starts[j]) * G >= static_cast<uint64_t>(chunk) * cut.size()) cut.push_back(j);
  cut.push_back(n_jobs);
  return cut;
}

// Tiles per legacy slice workgroup (log2): 16 (128 KiB of LDS, one workgroup
// per CU) unless the batch then has fewer slices than the chip has CUs.
// override_lg in [0, 4] (the caller's A/B knob) wins.
inline int choose_legacy_tps_lg(const std::vector<uint32_t>& n_tiles, int override_lg) {
  if (override_lg >= 0 && override_lg <= 4) return override_lg;
  int lg = 4;
  for (; lg > 0; lg--) {
    uint64_t total = 0;
    for (uint32_t t : n_tiles) total += (t + (1u << lg) - 1) >> lg;
    if (total >= kBuildSliceCUs) break;
  }
  return lg;
}

// The LDS-tiled legacy build's job table (tiles / regions: per job, as the
// caller's fit checks computed them).
inline JobTable<LegacyTileJobDev> plan_legacy_tile_jobs(const dlsm_build_job* jobs, int n_jobs, int bits_per_key,
                                                        uint64_t* out_len_dev, const std::vector<uint32_t>& tiles,
                                                        const std::vector<uint32_t>& regions, int tps_lg, int k) {
  JobTable<LegacyTileJobDev> T;
  T.hj.resize(n_jobs);
  T.starts.resize(2 * n_jobs);
  for (int j = 0; j < n_jobs; j++) {
    LegacyTileJobDev& d = T.hj[j];
    const uint64_t bits = legacy_bits(jobs[j].keys.n, bits_per_key);
    d.keys = to_desc(jobs[j].keys);
    d.out = jobs[j].out;
    d.out_len = out_len_dev + j;
    d.entry0 = T.entry;
    d.tab0 = T.tabw;
    d.bits = static_cast<uint32_t>(bits);
    d.magic = fastmod_magic(d.bits);
    d.n_tiles = tiles[j];
    d.region = regions[j];
    d.n_chunks = ceil_div_u32(jobs[j].keys.n, kLegacyChunk);
    d.chunk0 = T.chunk;
    d.n_slices = (tiles[j] + (1u << tps_lg) - 1) >> tps_lg;
    d.slice0 = T.slice;
    d.k = k;
    d.reserved = 0;
    T.starts[j] = T.chunk;
    T.starts[n_jobs + j] = T.slice;
    T.entry += static_cast<uint64_t>(d.n_chunks) * d.region;
    T.tabw += static_cast<uint64_t>(d.n_chunks) * (d.n_tiles + 1);
    T.chunk += d.n_chunks;
    T.slice += d.n_slices;
  }
  return T;
}

// ---- filter-set probe groups -------------------------------------------------
// A stacked image of the filters of one mask byte that share a line count
// and probe count (at most 8): filter f answers in bit f % 8 of byte f / 8.
// A group of 1, 2 or 3-4 filters gets a packed image instead (W = 1, 2 or 4
// bits per bit position, 64 * W bytes per line: 8 / 4 / 2 times the lines per
// LDS slice), so a large single filter -- the biggest file of a level -- still
// fits the sliced path, and small groups walk fewer, longer bucket runs.
struct ProbeGroup {
  uint64_t* stacked = nullptr;  // L * 8 * 2^lgw u64 words (device; the planner leaves it null)
  uint32_t L = 0, magic = 0;
  int k = 0;
  int mask_byte = 0;
  bool first_of_byte = false;  // writes its mask byte; later groups of the byte OR into it
  int lgw = 3;                  // log2 bits per bit position of the image (3: stacked bytes)
  uint32_t slotmap = 0;         // packed images: member m answers in bit (slotmap >> 4m) & 7
};

struct FilterGroupPlan {
  std::vector<ProbeGroup> groups;
  std::vector<std::vector<int>> members;  // per group, its filters
};

// Sliced-probe groups: within each mask byte, the filters with one (L, k)
// share a stacked image.  Every filter must have 64-byte lines (the
// reader's common case) for the sliced path; otherwise the set is probed
// directly (no groups).  packed == false: byte-wide images only (A/B knob).
inline FilterGroupPlan plan_filter_groups(const std::vector<FilterDev>& h, bool packed) {
  FilterGroupPlan P;
  const int n_filters = static_cast<int>(h.size());
  bool stack = true;
  for (int f = 0; f < n_filters; f++) stack = stack && h[f].lg == 6;
  if (!stack) return P;
  for (int b = 0; b * 8 < n_filters; b++) {
    bool first = true;
    std::vector<bool> done(8, false);
    for (int f = 8 * b; f < std::min(n_filters, 8 * b + 8); f++) {
      if (done[f - 8 * b]) continue;
      ProbeGroup g;
      g.L = h[f].L;
      g.magic = h[f].magic;
      g.k = h[f].k;
      g.mask_byte = b;
      g.first_of_byte = first;
      first = false;
      std::vector<int> m;
      for (int q = f; q < std::min(n_filters, 8 * b + 8); q++)
        if (!done[q - 8 * b] && h[q].L == g.L && h[q].k == g.k) {
          done[q - 8 * b] = true;
          m.push_back(q);
        }
      const int nm = static_cast<int>(m.size());
      g.lgw = nm == 1 ? 0 : nm == 2 ? 1 : nm <= 4 ? 2 : 3;
      if (!packed) g.lgw = 3;
      for (int j = 0; j < nm && g.lgw < 3; j++) g.slotmap |= static_cast<uint32_t>(m[j] % 8) << (4 * j);
      P.groups.push_back(g);
      P.members.push_back(m);
    }
  }
  return P;
}

// One image-width class of a one-pass multi-group probe: the global slices
// [s0, s0 + S) of the groups with image width lgw, walked by one slice launch
// of wgs workgroups (plan: S + 1 workgroup starts at plan_off of the plan).
struct MGClass {
  int lgw = 0, K = 0;  // K: 6 when every group of the class has k = 6, else 0 (run time k)
  uint32_t s0 = 0, S = 0;
  uint32_t plan_off = 0, wgs = 0;
};

struct MGLayout {
  bool ok = false;  // false: the set does not fit and keeps the per-group passes
  std::vector<MGroupDev> md;
  std::vector<uint32_t> plan;
  std::vector<MGClass> classes;
  uint32_t slices = 0;       // global slices
  uint32_t region = 0;       // entries per chunk region (every group's sub-region)
  uint32_t abytes = 0;       // answer bytes per chunk
  uint32_t stage_bytes = 0;  // the partition's largest staging area (LDS)
};

// The one-pass layout of a multi-group set (bloom_internal.h, MGroupDev): the
// groups ordered by image width (one slice launch per width), every group cut
// into full 128 KiB slices (2^(11 - lgw) lines), the slices numbered globally.
// Each width class gets a workgroup plan over the CUs (cu_budget): a slice's
// share of the workgroups is its share of the class's entries -- every lookup
// has one entry per group, so slice s of group j (nl_s of L_j lines) expects
// nl_s / L_j of them (a 3-slice group's slices get ~10x the workgroups of a
// 30-slice group's).  A set that does not fit (a group with more than 256
// slices, more than kMGMaxSlices in all, a group without an image) keeps the
// per-group passes.
inline MGLayout plan_mg_layout(const std::vector<ProbeGroup>& groups, uint32_t cu_budget) {
  MGLayout M;
  const int G = static_cast<int>(groups.size());
  std::vector<int> order(G);
  for (int j = 0; j < G; j++) order[j] = j;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return groups[a].lgw < groups[b].lgw; });
  std::vector<MGroupDev>& md = M.md;
  uint32_t sbase = 0;
  for (int j : order) {
    const ProbeGroup& g = groups[j];
    const uint32_t R = 1u << (11 - g.lgw);
    const uint32_t S = ceil_div_u32(g.L, R);
    if (S < 1 || S > static_cast<uint32_t>(kMaxSlices) || !g.stacked) return M;
    MGroupDev d{};
    d.image = reinterpret_cast<const uint8_t*>(g.stacked);
    d.L = g.L;
    d.magic = g.magic;
    d.R = R;
    d.rmagic = fastmod_magic(R);
    d.S = S;
    d.sbase = sbase;
    d.slotmap = g.slotmap;
    d.k = g.k;
    d.lgw = g.lgw;
    d.mask_byte = g.mask_byte;
    md.push_back(d);
    sbase += S;
  }
  if (sbase > kMGMaxSlices) return M;
  // every group's fixed sub-regions: entries, answers; its table columns
  constexpr uint32_t C = kMGChunk;
  uint32_t eoff = 0, aoff = 0;
  for (int j = 0; j < G; j++) {
    md[j].tcol = md[j].sbase + static_cast<uint32_t>(j);
    md[j].eoff = eoff;
    md[j].aoff = aoff;
    eoff += mg_sub_entries(C, md[j].S);
    aoff += mg_sub_abytes(C, md[j].S, md[j].lgw);
  }
  if (eoff > 65535u || aoff > 96u * 1024u) return M;  // u16 table offsets / the unpermute's LDS
  // the partition's staging LDS: the largest set of kMGSetSize groups
  constexpr int P = kMGSetSize;
  uint32_t stage = 0;
  for (int j0 = 0; j0 < G; j0 += P) {
    uint32_t st = 0;
    for (int j = j0; j < std::min(G, j0 + P); j++) st += mg_sub_entries(C, md[j].S) * 4u;
    stage = std::max(stage, st);
  }
  if (stage > 64u * 1024u) return M;
  const uint32_t budget = cu_budget;
  for (int j = 0; j < G;) {
    MGClass cl;
    cl.lgw = md[j].lgw;
    cl.s0 = md[j].sbase;
    cl.K = 6;
    std::vector<double> w;  // expected entry share per slice
    int q = j;
    for (; q < G && md[q].lgw == cl.lgw; q++) {
      if (md[q].k != 6) cl.K = 0;
      for (uint32_t t = 0; t < md[q].S; t++) {
        const uint32_t nl = std::min(md[q].R, md[q].L - t * md[q].R);
        w.push_back(static_cast<double>(nl) / md[q].L);
      }
    }
    cl.S = static_cast<uint32_t>(w.size());
    double W = 0;
    for (double x : w) W += x;
    std::vector<uint32_t> parts(cl.S);
    std::vector<std::pair<double, uint32_t>> rem;
    uint32_t used = 0;
    for (uint32_t t = 0; t < cl.S; t++) {
      const double want = budget * w[t] / W;
      parts[t] = std::max<uint32_t>(1u, static_cast<uint32_t>(want));
      used += parts[t];
      rem.push_back({want - parts[t], t});
    }
    std::sort(rem.begin(), rem.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    for (size_t r = 0; r < rem.size() && used < budget; r++, used++) parts[rem[r].second]++;
    cl.plan_off = static_cast<uint32_t>(M.plan.size());
    uint32_t acc = 0;
    for (uint32_t t = 0; t < cl.S; t++) {
      M.plan.push_back(acc);
      acc += parts[t];
    }
    M.plan.push_back(acc);
    cl.wgs = acc;
    M.classes.push_back(cl);
    j = q;
  }
  M.slices = sbase;
  M.region = eoff;
  M.abytes = aoff;
  M.stage_bytes = stage;
  M.ok = true;
  return M;
}

// ---- slice geometry and rounds of a probe -----------------------------------
// Slices of a group's image (line count L, image width lgw): the LDS holds up
// to 2^lgR lines (a byte-wide stacked table with more than kMaxSlices slices
// of 2^probe_lgr lines -- 64 KiB -- moves to 128 KiB, one workgroup per CU;
// packed images always use 128 KiB of 2^(11 - lgw) lines).  Balanced: the
// slice pass runs S x parts workgroups with parts = 256 / S0 (slice_parts, S0
// = the slice count at full width), so the slices are narrowed to R =
// ceil(L / floor(256 / parts)) lines to fill the 256 CUs exactly -- 8 x 1.6
// M-key filters (31,251 lines): 128 slices of 245 lines x 2 parts = 256
// workgroups instead of 123 x 2 = 246.
// Returns S, or 0 when the group cannot be sliced.
inline uint32_t group_slices(int probe_lgr, uint32_t L, int lgw, int* lgR, uint32_t* R_out) {
  if (lgw < 3) {
    *lgR = 11 - lgw;
  } else {
    *lgR = probe_lgr;
    if (ceil_div_u32(L, 1u << *lgR) > kMaxSlices && *lgR < 8) *lgR = 8;
  }
  const uint32_t Rmax = 1u << *lgR;
  const uint32_t S0 = ceil_div_u32(L, Rmax);
  if (S0 < 1 || S0 > kMaxSlices) return 0;
  uint32_t R = Rmax;
  const uint32_t per_cu = *lgR == 7 && lgw == 3 ? 2u : 1u;  // slice workgroups resident per CU
  const uint32_t slots = kBuildSliceCUs * per_cu;
  if (S0 < slots) {
    const uint32_t parts = std::max(1u, slots / S0);
    const uint32_t S_target = slots / parts;
    R = std::min(Rmax, ceil_div_u32(L, S_target));
  }
  *R_out = R;
  return ceil_div_u32(L, R);
}

// (slice, part) workgroups of the slice pass: about one resident wave of
// workgroups (256 CUs x 2 slices of 64 KiB or 1 of 128 KiB), each part at
// least one chunk per wave (a part's waves split its chunks into equal
// groups).
inline int slice_parts(uint32_t S, uint32_t nC, int lgR) {
  const uint32_t resident = 256u * (lgR == 7 ? 2u : 1u);
  int parts = static_cast<int>(std::max<uint32_t>(1, (resident + S / 2) / S));
  return std::min<int>(parts, static_cast<int>(std::max<uint32_t>(1, nC / 16)));
}

constexpr int kProbeBufs = 3;  // rotating intermediate buffers of a pipelined probe

// A probe of n keys cut into rounds of probe_round keys (0 or >= n: one
// round), whole chunks of C keys each; pipelined (round r's partition beside
// round r-1's slice pass, over nbuf rotating buffers) unless serial.
struct ProbeRounds {
  uint64_t round, n_rounds;
  bool pipe;
  int nbuf;
  uint64_t nCmax;  // chunks of the largest round
};
inline ProbeRounds probe_rounds(uint64_t n, uint64_t probe_round, bool serial, uint64_t C) {
  ProbeRounds r;
  r.round = n;
  if (probe_round && probe_round < n) r.round = std::max<uint64_t>(C, (probe_round / C) * C);
  r.n_rounds = (n + r.round - 1) / r.round;
  r.pipe = r.n_rounds > 1 && !serial;
  r.nbuf = r.pipe ? kProbeBufs : 1;
  r.nCmax = (std::min(r.round, n) + C - 1) / C;
  return r;
}

// The nr keys of kd from key r0 on (one round).
inline KeyDesc round_keys(const KeyDesc& kd, uint64_t r0, uint64_t nr) {
  KeyDesc kr = kd;
  kr.n = nr;
  if (kd.offsets) kr.offsets = kd.offsets + r0;
  else kr.bytes = kd.bytes + r0 * kd.key_len;
  return kr;
}

// ---- legacy block-based filter block (table/filter_block.cc) ----------------
constexpr uint64_t kFilterBaseLg = 11;  // filter_block.cc:15-16: a filter every 2 KiB

// FilterBlockBuilder's filter groups for the StartBlock / AddKey sequence of a
// TableBuilder: keys of data block b, then StartBlock(block_end_offset[b])
// (TableBuilder::Flush); GenerateFilter takes every pending key (first loop
// turn) or none (later turns); Finish generates one more if keys are pending.
struct FilterGroups {
  std::vector<uint64_t> begin, end;  // key range per filter (empty allowed)
  std::vector<uint32_t> off;         // filter_offsets_
  uint64_t array_offset = 0;
  uint64_t total = 0;  // block length
};

inline int filter_groups(const uint64_t* block_key_end, const uint64_t* block_end_offset, int n_blocks,
                         uint64_t n_keys, int bits_per_key, FilterGroups& G) {
  if (n_blocks < 0 || (n_blocks > 0 && (!block_key_end || !block_end_offset))) return DLSM_E_ARG;
  uint64_t pending = 0, prev_end = 0, result = 0;
  auto generate = [&](uint64_t upto) {
    G.off.push_back(static_cast<uint32_t>(result));
    G.begin.push_back(pending);
    G.end.push_back(upto);
    if (upto > pending) result += legacy_bits(upto - pending, bits_per_key) / 8 + 1;  // CreateFilter
    pending = upto;
  };
  for (int b = 0; b < n_blocks; b++) {
    const uint64_t ke = block_key_end[b];
    if (ke < prev_end || ke > n_keys) return DLSM_E_ARG;
    prev_end = ke;
    const uint64_t index = block_end_offset[b] / (uint64_t(1) << kFilterBaseLg);
    if (index < G.off.size()) return DLSM_E_ARG;  // assert(filter_index >= filter_offsets_.size())
    while (index > G.off.size()) generate(ke);     // later turns: no pending keys -> empty
  }
  if (n_keys > pending) generate(n_keys);  // Finish: start_ not empty
  G.array_offset = result;
  G.total = result + 4 * G.off.size() + 4 + 1;
  if (G.array_offset > 0xffffffffull) return DLSM_E_ARG;  // Fixed32 offsets
  return DLSM_OK;
}

// ---- version ------------------------------------------------------------------
// A level probed by the sliced version probe: its filters' lines back to
// back in one image (`image`, `lines` lines of 64 B, one probe count `k`).
struct VersionLevel {
  int level = 0;
  int k = 0;
  uint32_t lines = 0;
  const uint8_t* image = nullptr;  // device; the planner leaves it null (VersionPlan::image_off)
};

// Everything a version create computes before it allocates.  Per-file vectors
// are in search order (order[j]: the caller's index of file j); offsets are
// into the version's single allocation of `total` bytes:
// VFileDev[n] | prefixes | key blob | bounds | intervals | filters / level images | order.
struct VersionPlan {
  std::vector<int> order;
  int n_l0 = 0;
  uint32_t begin[kNumLevels] = {}, count[kNumLevels] = {};
  std::vector<VFileDev> h;
  std::vector<uint8_t> keys;
  std::vector<ulonglong2> pre, bnd;  // pre: n smallest | n largest
  std::vector<VIntervalDev> ivl;
  uint64_t files_bytes = 0, pre_bytes = 0, keys_bytes = 0, bnd_bytes = 0, ivl_bytes = 0;
  std::vector<uint64_t> foff, copy_len;  // per file: where its filter goes, and how much of it
  std::vector<VersionLevel> sliced;
  std::vector<uint64_t> image_off;  // per sliced level
  uint64_t order_off = 0, order_bytes = 0;  // order[] as u32 (the read plan's file mapping), after the filters
  int32_t lvl_sliced[kNumLevels] = {};
  uint64_t total = 0;
  int k_all = 0;
};

inline int check_version_files(const dlsm_version_file* files, int n_files) {
  if (n_files < 0 || (n_files > 0 && !files)) return DLSM_E_ARG;
  int n_l0 = 0;
  for (int f = 0; f < n_files; f++) {
    const dlsm_version_file& F = files[f];
    if (F.level < 0 || F.level >= kNumLevels) return DLSM_E_ARG;
    if ((F.smallest_len && !F.smallest_user_key) || (F.largest_len && !F.largest_user_key)) return DLSM_E_ARG;
    if (F.smallest_len > 0xffffffffull || F.largest_len > 0xffffffffull) return DLSM_E_ARG;
    if (F.level == 0) n_l0++;
  }
  if (n_l0 > 64 - (kNumLevels - 1)) return DLSM_E_ARG;
  return DLSM_OK;
}

// The probe count every filter of the version has, or 0 when they differ.
inline int version_k_all(const dlsm_version_file* files, const std::vector<int>& order,
                         const std::vector<VFileDev>& h) {
  int kc = 0;
  bool same = true;
  for (size_t j = 0; j < h.size(); j++) {
    if (!files[order[j]].filter) continue;
    same = same && (kc == 0 || h[j].f.k == kc);
    kc = h[j].f.k;
  }
  return same ? kc : 0;
}

// tails + 5 f: the last five bytes of files[f].filter (caller's order; unread for
// a file without filter or with filter_len < 5).  have_tails false (sealed
// blocks: the tails are known only after the device ingest): no filter is
// parsed and no level is sliced; the caller fills h[j].f and k_all afterwards.
// min_slice_bytes: a level >= 1 whose filters exceed it is sliced (0: none).
inline int plan_version(const dlsm_version_file* files, int n_files, const uint8_t* tails, bool have_tails,
                        uint64_t min_slice_bytes, VersionPlan& P) {
  if (int st = check_version_files(files, n_files)) return st;
  // search order: level 0 newest first (NewestFirst, version_set.cc:268-270),
  // then each level >= 1 in the caller's (key) order
  std::vector<int>& order = P.order;
  uint32_t* begin = P.begin;
  uint32_t* count = P.count;
  for (int f = 0; f < n_files; f++)
    if (files[f].level == 0) order.push_back(f);
  const int n_l0 = P.n_l0 = static_cast<int>(order.size());
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return files[a].number > files[b].number; });
  for (int lv = 1; lv < kNumLevels; lv++) {
    begin[lv] = static_cast<uint32_t>(order.size());
    for (int f = 0; f < n_files; f++)
      if (files[f].level == lv) order.push_back(f);
    count[lv] = static_cast<uint32_t>(order.size()) - begin[lv];
  }
  // layout: VFileDev[n] | key blob | filters (each 256-B aligned)
  std::vector<VFileDev>& h = P.h;
  std::vector<uint8_t>& keys = P.keys;
  h.resize(n_files);
  P.foff.assign(n_files, 0);
  P.files_bytes = (sizeof(VFileDev) * n_files + 255) & ~uint64_t(255);
  for (int j = 0; j < n_files; j++) {
    const dlsm_version_file& F = files[order[j]];
    VFileDev& d = h[j];
    d.smallest_off = keys.size();
    d.smallest_len = static_cast<uint32_t>(F.smallest_len);
    keys.insert(keys.end(), F.smallest_user_key, F.smallest_user_key + F.smallest_len);
    d.largest_off = keys.size();
    d.largest_len = static_cast<uint32_t>(F.largest_len);
    keys.insert(keys.end(), F.largest_user_key, F.largest_user_key + F.largest_len);
    d.largest_trailer = F.largest_trailer;
    d.f = FilterDev{};
  }
  // 16-byte big-endian key prefixes (VersionDev::pre_small / pre_large)
  std::vector<ulonglong2>& pre = P.pre;
  pre.resize(2 * static_cast<size_t>(n_files));
  auto be_prefix = [](const uint8_t* p, uint64_t n) {
    ulonglong2 r{0, 0};
    for (uint64_t i = 0; i < 16 && i < n; i++) {
      if (i < 8) r.x |= static_cast<uint64_t>(p[i]) << (56 - 8 * i);
      else r.y |= static_cast<uint64_t>(p[i]) << (56 - 8 * (i - 8));
    }
    return r;
  };
  for (int j = 0; j < n_files; j++) {
    pre[j] = be_prefix(keys.data() + h[j].smallest_off, h[j].smallest_len);
    pre[n_files + j] = be_prefix(keys.data() + h[j].largest_off, h[j].largest_len);
  }
  P.pre_bytes = (sizeof(ulonglong2) * pre.size() + 255) & ~uint64_t(255);
  P.keys_bytes = (keys.size() + 255) & ~uint64_t(255);
  // The interval index (VIntervalDev): the distinct bound prefixes in order,
  // and per open interval between two of them the level-0 files that hold
  // it and each level's FindFile pick.  For a lookup prefix strictly between
  // bnd[j-1] and bnd[j]: a bound with prefix index < j sorts below the lookup,
  // one with index >= j above it.
  auto pre_lt = [](const ulonglong2& a, const ulonglong2& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); };
  std::vector<ulonglong2>& bnd = P.bnd;
  bnd = pre;
  std::sort(bnd.begin(), bnd.end(), pre_lt);
  bnd.erase(std::unique(bnd.begin(), bnd.end(),
                        [](const ulonglong2& a, const ulonglong2& b) { return a.x == b.x && a.y == b.y; }),
            bnd.end());
  auto bidx = [&](const ulonglong2& p) {
    return static_cast<uint32_t>(std::lower_bound(bnd.begin(), bnd.end(), p, pre_lt) - bnd.begin());
  };
  std::vector<uint32_t> is(n_files), il(n_files);
  for (int j = 0; j < n_files; j++) {
    is[j] = bidx(pre[j]);
    il[j] = bidx(pre[n_files + j]);
  }
  const uint32_t n_bnd = static_cast<uint32_t>(bnd.size());
  std::vector<VIntervalDev>& ivl = P.ivl;
  ivl.resize(n_bnd + 1);
  // FindFile's pick per level as a two-pointer sweep: right(j) = the first
  // file r < count-1 whose largest has prefix index >= j (else count-1); the
  // set of such r only shrinks as j grows, so right(j) never decreases and
  // each level is walked once over all j (O(n_bnd + files), not O(n_bnd x
  // files): a 60,000-file level took seconds per version before).
  uint32_t rgt[kNumLevels] = {};
  for (uint32_t j = 0; j <= n_bnd; j++) {
    VIntervalDev& r = ivl[j];
    r.l0mask = 0;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    for (int f = 0; f < n_l0; f++)  // smallest <= lookup <= largest
      if (is[f] < j && il[f] >= j) r.l0mask |= 1ull << f;
    for (int lv = 1; lv < kNumLevels; lv++) {
      r.pick[lv - 1] = 0xffffu;
      if (!count[lv] || begin[lv] + count[lv] > 0xffffu) continue;  // (> 65,535 files: never read)
      // FindFile (version_set.cc:95-118): files [0, count-1) whose largest
      // sorts below the lookup come first; right starts at count-1
      uint32_t& right = rgt[lv];
      while (right < count[lv] - 1 && il[begin[lv] + right] < j) right++;
      if (is[begin[lv] + right] < j) r.pick[lv - 1] = static_cast<uint16_t>(begin[lv] + right);
    }
  }
  P.bnd_bytes = (sizeof(ulonglong2) * std::max<size_t>(1, bnd.size()) + 255) & ~uint64_t(255);
  P.ivl_bytes = (sizeof(VIntervalDev) * ivl.size() + 255) & ~uint64_t(255);
  uint64_t total = P.files_bytes + P.pre_bytes + P.keys_bytes + P.bnd_bytes + P.ivl_bytes;
  for (int j = 0; j < n_files && have_tails; j++) {
    const dlsm_version_file& F = files[order[j]];
    if (!F.filter) continue;
    if (F.filter_len < 5) return DLSM_E_CORRUPT;
    int k, lg;
    uint32_t L;
    if (int st = parse_tail(tails + 5 * order[j], F.filter_len, &k, &L, &lg)) return st;
    h[j].f.L = L;
    h[j].f.magic = fastmod_magic(L);
    h[j].f.k = k;
    h[j].f.lg = lg;
  }
  // Levels for the sliced probe; their filters' lines are laid out back to
  // back (line0 per file), the other filters one by one, 256-byte aligned.
  std::vector<VersionLevel>& sliced = P.sliced;
  std::vector<uint64_t>& copy_len = P.copy_len;
  copy_len.assign(n_files, 0);
  for (int lv = 0; lv < kNumLevels; lv++) P.lvl_sliced[lv] = -1;
  // (from sealed blocks the line counts are not known before the layout: no level is sliced)
  const uint64_t min_bytes = have_tails ? min_slice_bytes : 0;
  for (int lv = 1; lv < kNumLevels && min_bytes; lv++) {
    uint64_t lines = 0;
    int k = 0;
    bool ok = true;
    for (uint32_t j = begin[lv]; j < begin[lv] + count[lv]; j++) {
      if (!files[order[j]].filter) continue;
      ok = ok && h[j].f.lg == 6 && (k == 0 || h[j].f.k == k);
      k = h[j].f.k;
      lines += h[j].f.L;
    }
    if (!ok || lines * 64 <= min_bytes || lines >= kVNoLine) continue;
    P.lvl_sliced[lv] = static_cast<int32_t>(sliced.size());
    VersionLevel vl;
    vl.level = lv;
    vl.k = k;
    vl.lines = static_cast<uint32_t>(lines);
    sliced.push_back(vl);
  }
  P.image_off.assign(sliced.size(), 0);
  for (size_t q = 0; q < sliced.size(); q++) {
    const int lv = sliced[q].level;
    P.image_off[q] = total;
    uint32_t line0 = 0;
    for (uint32_t j = begin[lv]; j < begin[lv] + count[lv]; j++) {
      if (!files[order[j]].filter) continue;
      h[j].line0 = line0;
      P.foff[j] = total + static_cast<uint64_t>(line0) * 64;
      copy_len[j] = static_cast<uint64_t>(h[j].f.L) * 64;  // the lines; the trailer was parsed above
      line0 += h[j].f.L;
    }
    total += (static_cast<uint64_t>(sliced[q].lines) * 64 + 255) & ~uint64_t(255);
  }
  for (int j = 0; j < n_files; j++) {
    const dlsm_version_file& F = files[order[j]];
    if (!F.filter || copy_len[j]) continue;
    P.foff[j] = total;
    copy_len[j] = F.filter_len;
    total += (F.filter_len + 255) & ~uint64_t(255);
  }
  P.order_off = total;
  P.order_bytes = (sizeof(uint32_t) * static_cast<uint64_t>(n_files) + 255) & ~uint64_t(255);
  total += P.order_bytes;
  P.total = total;
  P.k_all = version_k_all(files, order, h);
  return DLSM_OK;
}

// ---- read plan (read_plan.hip) ---------------------------------------------------
// One digit pass of the plan's counting sort: its items (pass 0: the n Gets;
// later passes: the tasks, of which the host knows only the bound items_max --
// the kernels clip to the device-side total) on sort_grid's grid of kPlanChunk
// chunks.
struct ReadPlanPass : SortGrid {
  uint64_t items_max = 0;
  uint32_t shift = 0;  // the digit's first bit
};

// Everything dlsm_version_read_plan_dev computes before it launches: the
// passes, and the workspace layout (byte offsets, every region 256-byte
// aligned).  Buffer b of the key / Get-index pairs is written by pass p with
// p % 2 == b; in DLSM_PLAN_FIRST mode the histogram of pass 0 leaves one file
// id per Get in keys[1] for its scatter to read (4 B instead of mask + pick).
struct ReadPlan {
  int passes = 1;
  uint32_t gets_per_chunk = kPlanChunk;  // C of the tests: Gets per workgroup-chunk of pass 0
  uint64_t tasks_max = 0;                // bound on the tasks: n (FIRST) or n x tasks_per_get (ALL)
  ReadPlanPass pass[kPlanMaxPasses];
  uint32_t table_wgs = 1;    // workgroup rows of the tables: max nwg over the passes
  uint64_t table_entries = 0;  // kSortBins x table_wgs
  uint64_t pair_items = 0;   // items of each keys / vals buffer in use
  uint64_t cnt_off = 0, cnt_bytes = 0;    // u32[table_entries]: per (bin, workgroup) counts
  uint64_t off_off = 0, off_bytes = 0;    // u64[table_entries]: their exclusive prefix sums
  uint64_t drop_off = 0, drop_bytes = 0;  // u64[table_wgs]: per workgroup dropped tasks
  uint64_t total_off = 0, total_bytes = 0;  // u64[1]: the task total
  uint64_t keys_off[2] = {}, keys_bytes[2] = {};  // u32[pair_items] or unused (0 bytes)
  uint64_t vals_off[2] = {}, vals_bytes[2] = {};
  uint64_t bytes = 0;
};

// Digit passes that cover file ids 0 .. n_files-1.
inline int read_plan_passes(uint64_t n_files) {
  int bits = 0;
  while (n_files > 1 && ((n_files - 1) >> bits) != 0) bits++;
  return std::max(1, (bits + kSortBinLg - 1) / kSortBinLg);
}

inline ReadPlanPass read_plan_pass(uint64_t items_max, uint32_t shift) {
  ReadPlanPass p;
  p.items_max = items_max;
  p.shift = shift;
  static_cast<SortGrid&>(p) = sort_grid(items_max, kPlanChunk, kSortMaxWgs);
  return p;
}

// n Gets (<= UINT32_MAX) against a version of n_files files; tasks_per_get: the
// most tasks one Get can have (FIRST: 1; ALL: level-0 files + non-empty levels).
inline int plan_read(uint64_t n, uint64_t n_files, uint32_t tasks_per_get, int mode, ReadPlan& R) {
  if (n > 0xffffffffull || n_files > 0x7fffffffull || (mode != DLSM_PLAN_FIRST && mode != DLSM_PLAN_ALL))
    return DLSM_E_ARG;
  if (tasks_per_get > 64) return DLSM_E_ARG;
  R = ReadPlan();
  R.passes = read_plan_passes(n_files);
  R.tasks_max = mode == DLSM_PLAN_FIRST ? n : n * tasks_per_get;
  R.pass[0] = read_plan_pass(n, 0);
  for (int p = 1; p < R.passes; p++) R.pass[p] = read_plan_pass(R.tasks_max, static_cast<uint32_t>(p) * kSortBinLg);
  for (int p = 0; p < R.passes; p++) R.table_wgs = std::max(R.table_wgs, R.pass[p].nwg);
  R.table_entries = static_cast<uint64_t>(kSortBins) * R.table_wgs;
  Layout ws;
  ws.region(&R.cnt_off, &R.cnt_bytes, sizeof(uint32_t) * R.table_entries);
  ws.region(&R.off_off, &R.off_bytes, sizeof(uint64_t) * R.table_entries);
  ws.region(&R.drop_off, &R.drop_bytes, sizeof(uint64_t) * R.table_wgs);
  ws.region(&R.total_off, &R.total_bytes, sizeof(uint64_t));
  // keys[1]: FIRST's per-Get file ids, and pass 1's output; the rest only for
  // several passes (vals[1]: written by pass 1 when a pass 2 reads it)
  const bool multi = R.passes > 1;
  R.pair_items = R.tasks_max;
  const uint64_t pb = sizeof(uint32_t) * R.pair_items;
  ws.region(&R.keys_off[0], &R.keys_bytes[0], multi ? pb : 0);
  ws.region(&R.vals_off[0], &R.vals_bytes[0], multi ? pb : 0);
  ws.region(&R.keys_off[1], &R.keys_bytes[1], (multi || mode == DLSM_PLAN_FIRST) ? pb : 0);
  ws.region(&R.vals_off[1], &R.vals_bytes[1], R.passes > 2 ? pb : 0);
  R.bytes = ws.at;
  return DLSM_OK;
}

// The decoder's view of a version (levels 1..5 of begin / count).
inline PlanShape plan_shape(uint32_t n_l0, const uint32_t* begin, const uint32_t* count) {
  PlanShape s{};
  s.n_l0 = n_l0;
  s.n_slots = n_l0 + kPlanLevels;
  for (int lv = 1; lv < kNumLevels; lv++) {
    s.lvl_begin[lv - 1] = begin[lv];
    s.lvl_count[lv - 1] = count[lv];
  }
  return s;
}

// The most tasks one Get can have in DLSM_PLAN_ALL mode.
inline uint32_t plan_tasks_per_get(const PlanShape& s) {
  uint32_t t = s.n_l0;
  for (int lv = 0; lv < kPlanLevels; lv++) t += s.lvl_count[lv] ? 1u : 0u;
  return t;
}

// ---- shard route (shard_route.hip) -----------------------------------------------
// The route's one counting-sort pass: the n Gets on sort_grid's grid of
// kRouteChunk chunks and at most max_wgs (the ABI: kSortMaxWgs) workgroups, and
// the workspace layout (byte offsets, every region 256-byte aligned).
struct ShardRoute : SortGrid {
  uint32_t bins = 0;     // n_shards + 1: the shards and the "no shard" bin
  uint64_t table_entries = 0;               // bins x nwg
  uint64_t ids_off = 0, ids_bytes = 0;      // u16[n]: every Get's bin (the count pass writes them)
  uint64_t cnt_off = 0, cnt_bytes = 0;      // u32[table_entries]: per (bin, workgroup) counts
  uint64_t off_off = 0, off_bytes = 0;      // u64[table_entries]: the first output position of each
  uint64_t bytes = 0;
};

// dlsm_shard_route_cap: every bin's run starts at a multiple of kRouteAlign, so
// each of the n_shards + 1 bins wastes at most kRouteAlign - 1 slots.
inline uint64_t shard_route_cap(uint64_t n, int n_shards) {
  const uint64_t c = n + static_cast<uint64_t>(kRouteAlign - 1) * (static_cast<uint64_t>(n_shards) + 1);
  return (c + kRouteAlign - 1) & ~static_cast<uint64_t>(kRouteAlign - 1);
}

// The padded-offset arithmetic of the scan kernel: off[s] = the previous bin's
// end rounded up to kRouteAlign.  Returns the last bin's end rounded up.
inline uint64_t shard_route_offsets(const uint64_t* cnt, uint32_t bins, uint64_t* off) {
  uint64_t at = 0;
  for (uint32_t s = 0; s < bins; s++) {
    off[s] = at;
    at = (at + cnt[s] + kRouteAlign - 1) & ~static_cast<uint64_t>(kRouteAlign - 1);
  }
  return at;
}

inline int plan_shard_route(uint64_t n, int n_shards, uint32_t max_wgs, ShardRoute& R) {
  if (n > 0xffffffffull || n_shards < 1 || n_shards > static_cast<int>(kSortBins) - 1 || max_wgs == 0)
    return DLSM_E_ARG;
  R = ShardRoute();
  R.bins = static_cast<uint32_t>(n_shards) + 1;
  static_cast<SortGrid&>(R) = sort_grid(n, kRouteChunk, max_wgs);
  R.table_entries = static_cast<uint64_t>(R.bins) * R.nwg;
  Layout ws;
  ws.region(&R.ids_off, &R.ids_bytes, sizeof(uint16_t) * n);
  ws.region(&R.cnt_off, &R.cnt_bytes, sizeof(uint32_t) * R.table_entries);
  ws.region(&R.off_off, &R.off_bytes, sizeof(uint64_t) * R.table_entries);
  R.bytes = ws.at;
  return DLSM_OK;
}

// dlsm_shardmap_create's checks and the map's device image: the bounds'
// prefixes, their byte offsets and their bytes.  DLSM_E_ARG unless the bounds
// are strictly ascending under Slice::compare.
struct ShardMapImage {
  std::vector<RoutePrefix> pre;
  std::vector<uint64_t> off;   // n + 1
  std::vector<uint8_t> bytes;
  uint64_t pre_off = 0, off_off = 0, bytes_off = 0, total = 0;  // 256-byte aligned regions
};

inline int plan_shardmap(const uint8_t* const* bounds, const uint64_t* lens, int n_shards, ShardMapImage& M) {
  if (!bounds || !lens || n_shards < 1 || n_shards > static_cast<int>(kSortBins) - 1) return DLSM_E_ARG;
  M = ShardMapImage();
  M.off.assign(1, 0);
  for (int i = 0; i < n_shards; i++) {
    if (lens[i] && !bounds[i]) return DLSM_E_ARG;
    if (i > 0 && route_compare(bounds[i - 1], lens[i - 1], bounds[i], lens[i]) >= 0) return DLSM_E_ARG;
    M.pre.push_back(route_prefix(bounds[i], lens[i]));
    if (lens[i]) M.bytes.insert(M.bytes.end(), bounds[i], bounds[i] + lens[i]);
    M.off.push_back(M.bytes.size());
  }
  Layout img;
  M.pre_off = img.take(sizeof(RoutePrefix) * M.pre.size());
  M.off_off = img.take(sizeof(uint64_t) * M.off.size());
  M.bytes_off = img.take(std::max<size_t>(1, M.bytes.size()));
  M.total = img.at;
  return DLSM_OK;
}

// ---- table index (index_seek.hip) ----------------------------------------------
// dlsm_tableindex_create_blocks from the blocks' lengths alone: each held
// file's slot in the arena (256-byte aligned, the whole sealed block: host
// blocks are verified in place), its entry slots (the most entries len content
// bytes can hold) and its fences (one per S slots).  present[f] == 0: no index
// is held for file f.
struct IndexOpen {
  std::vector<uint64_t> arena_off;  // per file
  std::vector<uint64_t> fence0;     // per file
  std::vector<uint64_t> slot0;      // n_files + 1
  std::vector<uint32_t> rec;        // per file: its position among the held files
  uint32_t held = 0;
  uint64_t arena_bytes = 0, fences = 0, slots = 0;
};

inline int plan_index_open(const uint64_t* lens, const uint8_t* present, int n_files, uint32_t S, IndexOpen& P) {
  if (n_files < 0 || S == 0 || (n_files > 0 && (!lens || !present))) return DLSM_E_ARG;
  P = IndexOpen();
  P.arena_off.assign(n_files, 0);
  P.fence0.assign(n_files, 0);
  P.rec.assign(n_files, 0);
  P.slot0.assign(static_cast<size_t>(n_files) + 1, 0);
  for (int f = 0; f < n_files; f++) {
    P.slot0[f] = P.slots;
    if (!present[f]) continue;
    if (lens[f] > 0xffffffffull) return DLSM_E_ARG;  // Block's offsets are 32 bits
    const uint64_t content = lens[f] >= 5 ? lens[f] - 5 : 0;
    const uint64_t most = content >= 4 ? (content - 4) / kIndexEntryMinBytes : 0;
    P.arena_off[f] = P.arena_bytes;
    P.arena_bytes += (lens[f] + 255) & ~uint64_t(255);
    P.fence0[f] = P.fences;
    P.fences += (most + S - 1) / S;
    P.slots += most;
    P.rec[f] = P.held++;
  }
  P.slot0[n_files] = P.slots;
  return DLSM_OK;
}

// The seek's grid: a workgroup per kIndexSeekBlock tasks of the capacity, at
// most max_wgs; the kernel splits the true total (read on the device) evenly.
inline uint32_t plan_index_seek_wgs(uint64_t cap, uint32_t max_wgs) {
  const uint64_t w = (cap + kIndexSeekBlock - 1) / kIndexSeekBlock;
  return static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(w, 1), max_wgs));
}

// ---- value read (kv_read.hip) ---------------------------------------------------
// dlsm_kv_read_dev from the capacity alone (the item count is read on the
// device): the size and offset passes on sort_grid's grid of kKvChunk items, so
// at most max_wgs (the ABI: kSortMaxWgs) workgroups share the partial-sum table,
// the copy's persistent grid, and the workspace layout (byte offsets, every
// region 256-byte aligned): 12 bytes per item plus the partial sums.
struct KvReadPlan : SortGrid {
  uint32_t copy_wgs = 0;
  uint64_t len_off = 0, len_bytes = 0;  // u32[cap]
  uint64_t src_off = 0, src_bytes = 0;  // u64[cap]
  uint64_t sum_off = 0, sum_bytes = 0;  // u64[nwg]
  uint64_t bad_off = 0, bad_bytes = 0;  // u64[nwg]
  uint64_t bytes = 0;
};

// The copy's grid on a device of `cus` compute units.
inline uint32_t plan_kv_copy_wgs(uint32_t cus) { return std::max<uint32_t>(cus, 1) * kKvCopyWgsPerCu; }

inline int plan_kv_read(uint64_t cap, uint32_t max_wgs, uint32_t copy_wgs, KvReadPlan& P) {
  if (cap > 0xffffffffull || max_wgs == 0 || copy_wgs == 0) return DLSM_E_ARG;
  P = KvReadPlan();
  static_cast<SortGrid&>(P) = sort_grid(cap, kKvChunk, max_wgs);
  P.copy_wgs = copy_wgs;
  Layout ws;
  ws.region(&P.len_off, &P.len_bytes, sizeof(uint32_t) * cap);
  ws.region(&P.src_off, &P.src_bytes, sizeof(uint64_t) * cap);
  ws.region(&P.sum_off, &P.sum_bytes, sizeof(uint64_t) * P.nwg);
  ws.region(&P.bad_off, &P.bad_bytes, sizeof(uint64_t) * P.nwg);
  P.bytes = ws.at;
  return DLSM_OK;
}

// dlsm_tabledata_create from the chunk table alone: the running ends of every
// file's chunks (end[c] within its file), and, for host chunks, each chunk's
// place in the arena (16-byte aligned).
struct TableDataPlan {
  std::vector<uint64_t> end;        // per chunk
  std::vector<uint64_t> arena_off;  // per chunk
  uint64_t arena_bytes = 0, data_bytes = 0;
};

inline int plan_tabledata(const dlsm_data_chunk* chunks, const uint32_t* chunk_begin, int n_files, TableDataPlan& P) {
  if (n_files < 0 || !chunk_begin || chunk_begin[0] != 0) return DLSM_E_ARG;
  P = TableDataPlan();
  const uint32_t nc = chunk_begin[n_files];
  if (nc > 0 && !chunks) return DLSM_E_ARG;
  P.end.assign(nc, 0);
  P.arena_off.assign(nc, 0);
  for (int f = 0; f < n_files; f++) {
    if (chunk_begin[f + 1] < chunk_begin[f] || chunk_begin[f + 1] > nc) return DLSM_E_ARG;
    uint64_t at = 0;
    for (uint32_t c = chunk_begin[f]; c < chunk_begin[f + 1]; c++) {
      if (chunks[c].len && !chunks[c].base) return DLSM_E_ARG;
      if (at + chunks[c].len < at) return DLSM_E_ARG;
      at += chunks[c].len;
      P.end[c] = at;
      P.arena_off[c] = P.arena_bytes;
      P.arena_bytes += (chunks[c].len + 15) & ~uint64_t(15);
      P.data_bytes += chunks[c].len;
    }
  }
  return DLSM_OK;
}

}  // namespace plan
}  // namespace dlsm
