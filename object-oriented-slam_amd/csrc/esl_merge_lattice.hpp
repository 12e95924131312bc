// esl_merge_lattice.hpp — the integer side of esl_map_overlaps / esl_map_merge (include/esl.h, "map maintenance"): the lattice of the unit
// ball (step 2), the walk a lane takes through the lattice's cube, and the ordered key that settles a conflict of the rewritten edge
// list (step 7).  Plain C++ for host and device, no HIP include: tests/merge_lattice_main.cpp compiles it with an ordinary compiler.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ESL_MERGE_HD __host__ __device__
#else
#define ESL_MERGE_HD
#endif

namespace esl {

constexpr int kMergeLatticeMin = 4, kMergeLatticeMax = 32;
constexpr int kMergeMaxObjects = 65536;

// The cube of the lattice has n^3 cells t = (px n + py) n + pz, so ascending t is the (px, py, pz) lexicographic order.  Cell p stands
// for the odd integer triple k = 2 p + 1 - n; it belongs to the ball iff |k|^2 <= n^2 (never equal: |k|^2 = 3 mod 8 for even n, n^2 is
// 0 or 4 mod 8; for odd n every k is even, |k|^2 = 0 mod 4, n^2 = 1 mod 4).
struct MergeCell { int px, py, pz; };

ESL_MERGE_HD inline int merge_lattice_cells(int n) { return n * n * n; }

ESL_MERGE_HD inline MergeCell merge_cell_of(int n, int t) {
  MergeCell c;
  c.pz = t % n; t /= n;
  c.py = t % n; c.px = t / n;
  return c;
}

// the stride of a wavefront through the cube, 64 = a n^2 + b n + c with b, c < n, and one step of a lane by it: no division in the loop
struct MergeStep { int a, b, c; };
ESL_MERGE_HD inline MergeStep merge_step_of(int n, int stride) {
  MergeStep s;
  s.c = stride % n; stride /= n;
  s.b = stride % n; s.a = stride / n;
  return s;
}
ESL_MERGE_HD inline void merge_cell_advance(int n, const MergeStep& s, MergeCell& c) {
  c.pz += s.c;
  if (c.pz >= n) { c.pz -= n; ++c.py; }
  c.py += s.b;
  if (c.py >= n) { c.py -= n; ++c.px; }
  c.px += s.a;   // px >= n: the lane has left the cube
}

ESL_MERGE_HD inline void merge_cell_k(int n, const MergeCell& c, int k[3]) {
  k[0] = 2 * c.px + 1 - n; k[1] = 2 * c.py + 1 - n; k[2] = 2 * c.pz + 1 - n;
}
ESL_MERGE_HD inline bool merge_cell_in_ball(int n, const MergeCell& c) {
  int k[3];
  merge_cell_k(n, c, k);
  return c.px < n && k[0] * k[0] + k[1] * k[1] + k[2] * k[2] <= n * n;
}

// N_ball(n): 32, 280, 2176, 17256 for n = 4, 8, 16, 32
ESL_MERGE_HD inline int merge_lattice_count(int n) {
  int cnt = 0;
  for (int t = 0; t < n * n * n; ++t) cnt += merge_cell_in_ball(n, merge_cell_of(n, t)) ? 1 : 0;
  return cnt;
}

// Step 7: of the list entries that land on one (frame, merged object) the one with the SMALLEST key survives -- larger weight of the
// original object first, then the lower original index.  weight in [0, 2^31), index in [0, 65536).  Entries of the winning object are
// then ordered by their list position.
ESL_MERGE_HD inline uint64_t merge_conflict_key(int32_t weight, int32_t index) {
  return ((uint64_t)(uint32_t)(0x7fffffff - weight) << 32) | (uint64_t)(uint32_t)index;
}
ESL_MERGE_HD inline int32_t merge_conflict_key_index(uint64_t key) { return (int32_t)(uint32_t)(key & 0xffffffffull); }

// the group's representative is the member with the LARGEST of these: larger weight, then the lower index
ESL_MERGE_HD inline uint64_t merge_rep_key(int32_t weight, int32_t index) {
  return ((uint64_t)(uint32_t)weight << 32) | (uint64_t)(uint32_t)(0x7fffffff - index);
}
ESL_MERGE_HD inline int32_t merge_rep_key_index(uint64_t key) { return 0x7fffffff - (int32_t)(uint32_t)(key & 0xffffffffull); }

// the hash table's key of (frame, merged object): frame < 2^31, group < 2^17; never all ones (the empty slot)
ESL_MERGE_HD inline uint64_t merge_slot_key(int32_t cam, int32_t group) { return ((uint64_t)(uint32_t)cam << 17) | (uint64_t)(uint32_t)group; }
ESL_MERGE_HD inline uint64_t merge_slot_hash(uint64_t z) {   // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace esl
