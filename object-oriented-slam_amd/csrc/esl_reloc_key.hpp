// esl_reloc_key.hpp — the two pieces of esl_relocalize (esl_reloc.hip) that are plain integer / comparison logic: the decode of a pair
// index into its candidate pair and the total order that picks the winning hypothesis.  No HIP in here: tests/reloc_key_main.cpp
// compiles this header with a plain C++ compiler (and its sanitizers) and walks the boundaries.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define ESL_RELOC_HD __host__ __device__
#else
#define ESL_RELOC_HD
#endif

namespace esl {

// Pairs i < j of P candidates, numbered t = j (j - 1) / 2 + i (t < P (P - 1) / 2 <= 2^39 at the largest P the interface admits).
// The square root only proposes j; the two loops make the result exact whatever its rounding.
ESL_RELOC_HD inline void reloc_pair_decode(uint64_t t, uint64_t& i, uint64_t& j) {
  uint64_t jj = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)t)) * 0.5);
  if (jj < 1) jj = 1;
  while (jj * (jj - 1) / 2 > t) --jj;
  while ((jj + 1) * jj / 2 <= t) ++jj;
  j = jj;
  i = t - jj * (jj - 1) / 2;
}
ESL_RELOC_HD inline uint64_t reloc_pair_count(uint64_t P) { return P < 2 ? 0 : P * (P - 1) / 2; }

// A scored hypothesis: inlier count, sum of squared inlier distances, key = i P + j.  key < 0: none.
struct RelocBest {
  int64_t key;
  double cost;
  int32_t n;
  int32_t pad;
};
// total order: more inliers, then lower cost, then lower key; anything beats "none".  Keys are unique, so two different hypotheses
// never compare equal and the winner does not depend on the order they are met in.
ESL_RELOC_HD inline bool reloc_better(int32_t na, double ca, int64_t ka, int32_t nb, double cb, int64_t kb) {
  if (ka < 0) return false;
  if (kb < 0) return true;
  if (na != nb) return na > nb;
  if (ca != cb) return ca < cb;
  return ka < kb;
}

}  // namespace esl
