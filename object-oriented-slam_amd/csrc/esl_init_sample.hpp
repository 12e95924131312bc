// esl_init_sample.hpp — the view subsets of esl_init_quadrics_robust's hypotheses (include/esl.h, step 2): Floyd's sampling of s distinct
// indices out of n, driven by a splitmix64 finaliser of (seed, h, k).  Plain C++ for host and device, no HIP include:
// tests/init_sample_main.cpp compiles it with an ordinary compiler.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ESL_SAMPLE_HD __host__ __device__
#else
#define ESL_SAMPLE_HD
#endif

namespace esl {

constexpr int kInitSampleMax = 16;   // the largest sample_size

// splitmix64's finaliser of seed ^ (golden ratio * counter), everything mod 2^64 (esl_dense_planes.hpp counts differently)
ESL_SAMPLE_HD inline uint64_t init_sample_finalise(uint64_t seed, uint64_t counter) {
  uint64_t z = seed ^ (0x9E3779B97F4A7C15ull * counter);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// ... on the counter 32 h + k + 1
ESL_SAMPLE_HD inline uint64_t init_sample_mix(uint64_t seed, uint32_t h, uint32_t k) {
  return init_sample_finalise(seed, (uint64_t)(32ull * h + k + 1ull));
}

// how many hypotheses an object of n entries has, and how many entries each uses
ESL_SAMPLE_HD inline int init_sample_count(int n, int sample_size, int n_hypotheses) { return n <= sample_size ? 1 : n_hypotheses; }
ESL_SAMPLE_HD inline int init_sample_views(int n, int sample_size) { return n < sample_size ? n : sample_size; }

// out[0 .. s): the local indices of hypothesis h, ascending; s = min(sample_size, n) <= kInitSampleMax.  With n <= sample_size the
// sample is 0 .. n-1 whatever h is.  Returns s.
ESL_SAMPLE_HD inline int init_sample(uint64_t seed, int h, int n, int sample_size, int32_t* out) {
  const int s = init_sample_views(n, sample_size);
  if (n <= sample_size) {
    for (int k = 0; k < s; ++k) out[k] = k;
    return s;
  }
  for (int k = 0; k < s; ++k) {
    const int j = n - s + k;
    int t = (int)((init_sample_mix(seed, (uint32_t)h, (uint32_t)k) >> 11) % (uint64_t)(j + 1));
    for (int i = 0; i < k; ++i)
      if (out[i] == t) { t = j; break; }   // j itself cannot have been taken: every earlier pick is < j
    out[k] = t;
  }
  for (int k = 1; k < s; ++k) {   // ascending (insertion sort: s <= 16)
    const int32_t v = out[k];
    int i = k - 1;
    for (; i >= 0 && out[i] > v; --i) out[i + 1] = out[i];
    out[i + 1] = v;
  }
  return s;
}

}  // namespace esl
