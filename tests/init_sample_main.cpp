// Stand-alone driver of csrc/esl_init_sample.hpp (the view subsets of esl_init_quadrics_robust) for tests/test_init_robust_ref.py, which
// compiles it with and without -fsanitize=address,undefined and compares its output exactly with the Python sampler.
//   stdin:  seed sample_size n_hypotheses count, then `count` values of n
//   stdout: per n and hypothesis "n h s i0 i1 ..." (the hypotheses init_sample_count says the object has), and per n a line
//           "mix n <mix(seed, n, 0)>" so that the 64-bit stream itself is compared too
#include <cstdio>
#include <vector>

#include "../object-oriented-slam_amd/csrc/esl_init_sample.hpp"

int main() {
  unsigned long long seed;
  int sample_size, H, count;
  if (std::scanf("%llu %d %d %d", &seed, &sample_size, &H, &count) != 4) return 2;
  if (sample_size < 1 || sample_size > esl::kInitSampleMax || H < 1 || count < 0) return 2;
  for (int c = 0; c < count; ++c) {
    int n;
    if (std::scanf("%d", &n) != 1 || n < 0) return 2;
    std::vector<int32_t> out((size_t)esl::init_sample_views(n, sample_size));   // exactly s entries: a write past them is an error
    const int nh = esl::init_sample_count(n, sample_size, H);
    for (int h = 0; h < nh; ++h) {
      const int s = esl::init_sample((uint64_t)seed, h, n, sample_size, out.data());
      std::printf("%d %d %d", n, h, s);
      for (int k = 0; k < s; ++k) std::printf(" %d", out[(size_t)k]);
      std::printf("\n");
    }
    std::printf("mix %d %llu\n", n, (unsigned long long)esl::init_sample_mix((uint64_t)seed, (uint32_t)n, 0));
  }
  return 0;
}
