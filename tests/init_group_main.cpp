// Stand-alone driver of csrc/esl_init_group.hpp (the host side of esl_init_quadrics' input) for tests/test_init_batch_ref.py, which
// compiles it with -fsanitize=address,undefined and compares its output with the numpy grouping.
//   stdin:  N F tile min_observations n_obs, then n_obs pairs "cam obj"
//   stdout: "rc <code> <bad entry>", then on success "offsets ...", "idx ...", "slab <observations>", "order obj first n spill" per object
#include <cstdio>
#include <vector>

#include "../object-oriented-slam_amd/csrc/esl_init_group.hpp"

int main() {
  int N, F, tile, min_obs;
  long long n_obs;
  if (std::scanf("%d %d %d %d %lld", &N, &F, &tile, &min_obs, &n_obs) != 5) return 2;
  std::vector<int32_t> cam((size_t)n_obs), obj((size_t)n_obs);
  for (long long i = 0; i < n_obs; ++i)
    if (std::scanf("%d %d", &cam[(size_t)i], &obj[(size_t)i]) != 2) return 2;
  std::vector<int32_t> offsets, idx;
  std::vector<esl::InitObj> order;
  int64_t bad = -1;
  // empty vectors hand out null pointers: what a caller with n_obs = 0 passes
  const int rc = esl::init_group(n_obs, N, F, cam.data(), obj.data(), offsets, idx, &bad);
  std::printf("rc %d %lld\n", rc, (long long)bad);
  if (rc) return 0;
  std::printf("offsets");
  for (int32_t v : offsets) std::printf(" %d", v);
  std::printf("\nidx");
  for (int32_t v : idx) std::printf(" %d", v);
  const int64_t slab = esl::init_order(N, offsets, tile, min_obs, order);
  std::printf("\nslab %lld\n", (long long)slab);
  for (const esl::InitObj& e : order) std::printf("order %d %d %d %d\n", e.obj, e.first, e.n, e.spill);
  return 0;
}
