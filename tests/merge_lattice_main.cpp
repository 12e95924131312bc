// Stand-alone driver of csrc/esl_merge_lattice.hpp (the integer side of esl_map_overlaps / esl_map_merge) for
// tests/test_map_merge_ref.py, which compiles it with and without -fsanitize=address,undefined and compares its output exactly with the
// Python statement.
//   stdin:  count, then `count` values of n; then pairs, then `pairs` lines "weight index"
//   stdout: per n  "count n N_ball", one line "cell n t px py pz kx ky kz in" per cube cell t, and, for every lane 0..63, the walk the
//           overlap kernel takes -- "walk n lane t0 t1 ..." where each t is rebuilt from the advanced cell, -1 once the cell has left
//           the cube; then per pair "key weight index conflict_key rep_key conflict_index rep_index"
#include <cstdio>
#include <vector>

#include "../object-oriented-slam_amd/csrc/esl_merge_lattice.hpp"

int main() {
  int count;
  if (std::scanf("%d", &count) != 1 || count < 0) return 2;
  for (int c = 0; c < count; ++c) {
    int n;
    if (std::scanf("%d", &n) != 1 || n < esl::kMergeLatticeMin || n > esl::kMergeLatticeMax) return 2;
    const int cells = esl::merge_lattice_cells(n);
    std::printf("count %d %d\n", n, esl::merge_lattice_count(n));
    std::vector<int> seen((size_t)cells, 0);   // exactly n^3 entries: a walk that leaves the cube unnoticed writes past them
    for (int t = 0; t < cells; ++t) {
      const esl::MergeCell cell = esl::merge_cell_of(n, t);
      int k[3];
      esl::merge_cell_k(n, cell, k);
      std::printf("cell %d %d %d %d %d %d %d %d %d\n", n, t, cell.px, cell.py, cell.pz, k[0], k[1], k[2], esl::merge_cell_in_ball(n, cell) ? 1 : 0);
    }
    const esl::MergeStep step = esl::merge_step_of(n, 64);
    const int rounds = (cells + 63) / 64;
    for (int lane = 0; lane < 64; ++lane) {
      esl::MergeCell cell = esl::merge_cell_of(n, lane);
      std::printf("walk %d %d", n, lane);
      for (int it = 0; it < rounds; ++it) {
        int t = -1;
        if (cell.px < n) {
          t = (cell.px * n + cell.py) * n + cell.pz;
          if (cell.py < 0 || cell.py >= n || cell.pz < 0 || cell.pz >= n) return 3;
          ++seen[(size_t)t];
        }
        std::printf(" %d", t);
        esl::merge_cell_advance(n, step, cell);
      }
      std::printf("\n");
    }
    for (int t = 0; t < cells; ++t)
      if (seen[(size_t)t] != 1) return 4;   // every cell exactly once
  }
  int pairs;
  if (std::scanf("%d", &pairs) != 1 || pairs < 0) return 2;
  for (int p = 0; p < pairs; ++p) {
    long long w, i;
    if (std::scanf("%lld %lld", &w, &i) != 2 || w < 0 || w > 0x7fffffffll || i < 0 || i >= esl::kMergeMaxObjects) return 2;
    const uint64_t ck = esl::merge_conflict_key((int32_t)w, (int32_t)i), rk = esl::merge_rep_key((int32_t)w, (int32_t)i);
    std::printf("key %lld %lld %llu %llu %d %d\n", w, i, (unsigned long long)ck, (unsigned long long)rk, esl::merge_conflict_key_index(ck),
                esl::merge_rep_key_index(rk));
  }
  return 0;
}
