// dlsm_amd/csrc/read_plan.h -- the read plan's constants and its task decoder,
// shared by the kernels (read_plan.hip), the planner (host_plan.h) and the CPU
// test (tests/cpp/read_plan_test.cc).  Plain integer code: no device call.
#pragma once
#include <stdint.h>

#include "bloom_math.h"
#include "sort_pass.h"

namespace dlsm {

// The plan is a stable counting sort of (Get, file) tasks by file id, one digit
// of kSortBinLg bits per pass (sort_pass.h), least significant first: one pass
// up to kSortBins files.
constexpr int kPlanChunkLg = 15;
constexpr uint32_t kPlanChunk = 1u << kPlanChunkLg;  // items (Gets or tasks) per workgroup-chunk
constexpr uint32_t kPlanWaveItems = kPlanChunk / kSortWaves;  // a wave's contiguous share of a chunk
constexpr int kPlanMaxPasses = 4;           // 4 x 9 bits >= the 31 bits of an int file count
constexpr uint32_t kPlanNoFile = 0xffffffffu;  // decoder: the task is dropped; a Get without a task
constexpr int kPlanLevels = 5;              // levels 1 .. kNumLevels-1: one search slot each

static_assert(kPlanWaveItems % 128 == 0, "a wave walks its share 128 Gets (one 16-byte load per lane) at a time");
static_assert(kSortBinLg * kPlanMaxPasses >= 31, "the passes cover every file count an int holds");

// What the decoder needs of a version: its search slots and, per level 1..5,
// where the level's files start in search order and how many there are.
struct PlanShape {
  uint32_t n_l0;
  uint32_t n_slots;  // n_l0 + kPlanLevels (<= 64)
  uint32_t lvl_begin[kPlanLevels];
  uint32_t lvl_count[kPlanLevels];
};

// Task (slot, pick) -> the file's index in search order, or kPlanNoFile when
// the task is malformed and must be dropped: a slot the version does not have,
// or a level pick past the level's files (UINT32_MAX included; an empty level
// drops every pick).  pick is read for slots >= n_l0 only.
DLSM_HD uint32_t plan_task_file(const PlanShape& v, uint32_t slot, uint32_t pick) {
  if (slot >= v.n_slots) return kPlanNoFile;
  if (slot < v.n_l0) return slot;
  const uint32_t lv = slot - v.n_l0;  // level - 1
  if (lv >= static_cast<uint32_t>(kPlanLevels) || pick >= v.lvl_count[lv]) return kPlanNoFile;
  return v.lvl_begin[lv] + pick;
}

// The digit of file id f that pass p sorts by.
DLSM_HD uint32_t plan_digit(uint32_t f, uint32_t shift) { return (f >> shift) & (kSortBins - 1u); }

}  // namespace dlsm
