// esl_dense_covis.hpp — the arithmetic of esl_dense_covis_frames (include/esl.h, "covisibility of the dense map"; the steps' numbers
// below are the header's) beyond the observation itself, which is dcv_observe of esl_dense_carve.hpp word for word (step V2): the
// redundancy predicate (step V5), the order of two cull candidates (step V6) and the pair count of two rows of the bit matrix (step V4).
// Plain C++ for host and device, no HIP include: tests/dense_covis_main.cpp compiles it with an ordinary compiler.  Every translation
// unit that includes it is built with -ffp-contract=off, as esl_dense_carve.hpp asks.
#pragma once
#include "esl_dense_carve.hpp"

namespace esl {

constexpr int kDcoChunk = 32;           // frames per chunk of k_dco_observe
constexpr int kDcoTile = 32;            // the edge of k_dco_pairs' tile of frame pairs, in frames
constexpr int kDcoSlab = 64;            // the words of a row that k_dco_pairs stages in LDS at a time
constexpr int kDcoMaxFrames = 4096;     // F: pair_out holds F x F int32, at most 64 MiB
constexpr int kDcoMaxCoverDen = 1 << 20;

// step V5: frame f with seen_f voxels, covered_f of them covered without it; both products as 64-bit integers
ESL_DENSE_HD bool dco_redundant(int seen, int covered, int cover_num, int cover_den) {
  return seen >= 1 && (long long)covered * (long long)cover_den >= (long long)cover_num * (long long)seen;
}

// step V6: does candidate a (frame fa with unc_a = seen - covered voxels that only it keeps covered) leave before candidate b
ESL_DENSE_HD bool dco_before(int unc_a, int fa, int unc_b, int fb) { return unc_a < unc_b || (unc_a == unc_b && fa < fb); }

ESL_DENSE_HD int dco_popc(unsigned long long w) { return __builtin_popcountll(w); }   // the compiler's builtin on host and device

// step V4: the voxels that two frames both see, from their rows of W words (bit i % 64 of word i / 64 = the frame sees voxel i)
ESL_DENSE_HD long long dco_pair_count(const unsigned long long* a, const unsigned long long* b, long long W) {
  long long s = 0;
  for (long long w = 0; w < W; ++w) s += dco_popc(a[w] & b[w]);   // at most W words
  return s;
}

}  // namespace esl
