// esl_init_group.hpp — the host side of esl_init_quadrics' input: a stable counting sort of the observation list by object, the checks
// of its indices, and the launch order.  Plain C++, no HIP: tests/init_group_main.cpp compiles it with an ordinary compiler.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace esl {

// one object of the launch: its observations are idx[first .. first + n), its plane matrix lives at row 4 * spill of the global slab
// when spill >= 0 (more than `tile` observations), in LDS otherwise
struct InitObj { int32_t obj, first, n, spill; };

enum { INIT_GROUP_OK = 0, INIT_GROUP_BAD_CAM = 1, INIT_GROUP_BAD_OBJ = 2 };

// Entries with obs_obj < 0 are skipped (an esl_associate_boxes assoc_out is an obs_obj).  offsets: N + 1, idx: the kept entries'
// positions in the list, grouped by object, list order inside a group.  A kept entry with obs_cam outside [0, F) or obs_obj >= N
// fails the call; *bad is its position.
inline int init_group(int64_t n_obs, int32_t N, int32_t F, const int32_t* obs_cam, const int32_t* obs_obj, std::vector<int32_t>& offsets,
                      std::vector<int32_t>& idx, int64_t* bad) {
  offsets.assign((size_t)N + 1, 0);
  int64_t kept = 0;
  for (int64_t i = 0; i < n_obs; ++i) {
    const int32_t o = obs_obj[i];
    if (o < 0) continue;
    if (o >= N) { if (bad) *bad = i; return INIT_GROUP_BAD_OBJ; }
    if (obs_cam[i] < 0 || obs_cam[i] >= F) { if (bad) *bad = i; return INIT_GROUP_BAD_CAM; }
    ++offsets[(size_t)o + 1];
    ++kept;
  }
  for (int32_t o = 0; o < N; ++o) offsets[(size_t)o + 1] += offsets[o];
  idx.resize((size_t)kept);
  std::vector<int32_t> at(offsets.begin(), offsets.end() - 1);
  for (int64_t i = 0; i < n_obs; ++i) {
    const int32_t o = obs_obj[i];
    if (o >= 0) idx[(size_t)at[o]++] = (int32_t)i;
  }
  return INIT_GROUP_OK;
}

// The launch list: objects by falling observation count (ties by rising index), so the long ones start first and the short ones fill
// the tail.  An object with at least min_observations observations and more than `tile` of them gets rows of the slab; returns the
// slab's size in observations.
inline int64_t init_order(int32_t N, const std::vector<int32_t>& offsets, int32_t tile, int32_t min_observations, std::vector<InitObj>& order) {
  order.resize((size_t)N);
  for (int32_t o = 0; o < N; ++o) order[o] = InitObj{o, offsets[o], offsets[(size_t)o + 1] - offsets[o], -1};
  std::stable_sort(order.begin(), order.end(), [](const InitObj& a, const InitObj& b) { return a.n > b.n; });
  int64_t slab = 0;
  for (InitObj& e : order)
    if (e.n > tile && e.n >= min_observations) {
      if (slab + e.n > INT32_MAX) return -1;
      e.spill = (int32_t)slab;
      slab += e.n;
    }
  return slab;
}

}  // namespace esl
