// esl_dense_key.hpp — the per-sample arithmetic of esl_dense_* (include/esl.h, "the dense map"; the steps' numbers below are the
// header's): the depth sample and its camera point (step 1), the pose and the world point (step 2), the voxel key, its packing and the
// range test (step 3), the fixed-point term of the centroid sums (step 4) and the rounding of a mean colour (step 7).  Plain C++ for
// host and device, no HIP include: tests/dense_key_main.cpp compiles it with an ordinary compiler.  Every translation unit that
// includes it is built with -ffp-contract=off: the keys are floors of computed doubles and are compared exactly.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ESL_DENSE_HD __host__ __device__ inline
#else
#define ESL_DENSE_HD inline
#endif

namespace esl {

constexpr int kDenseMaxDim = 16384;                           // rows, cols
constexpr int kDenseKeyOff = 1 << 20;                         // a key component is stored as k + 2^20 in 21 bits
constexpr int kDenseKeyMax = (1 << 20) - 1;                   // |k| above this: the sample is dropped (n_key_out)
constexpr unsigned long long kDenseEmpty = ~0ull;             // no packed key has bit 63 set
constexpr double kDenseFix = 1073741824.0;                    // 2^30 fixed-point units per metre
constexpr int kDensePose = 12;                                // R row-major (9), t (3)

enum { DENSE_USED = 0, DENSE_ZERO = 1, DENSE_DEPTH_OUT = 2, DENSE_KEY_OUT = 3 };

// step 2: the frame's R (q_to_R's matrix of the quaternion divided by its norm) and t.  false: a non-finite number, or a norm that is
// 0 or not finite.  Runs on the host only (the poses of a call are a few numbers), so one compiler decides every bit of R.
inline bool dense_pose(const double cam[7], double P[kDensePose]) {
  bool ok = true;
  for (int k = 0; k < 7; ++k) ok = ok && std::isfinite(cam[k]);
  const double nrm = std::sqrt(cam[3] * cam[3] + cam[4] * cam[4] + cam[5] * cam[5] + cam[6] * cam[6]);
  if (!ok || !std::isfinite(nrm) || !(nrm > 0)) return false;
  const double x = cam[3] / nrm, y = cam[4] / nrm, z = cam[5] / nrm, w = cam[6] / nrm;
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  P[0] = 1 - (tyy + tzz); P[1] = txy - twz;       P[2] = txz + twy;
  P[3] = txy + twz;       P[4] = 1 - (txx + tzz); P[5] = tyz - twx;
  P[6] = txz - twy;       P[7] = tyz + twx;       P[8] = 1 - (txx + tyy);
  P[9] = cam[0]; P[10] = cam[1]; P[11] = cam[2];
  return true;
}

// step 1: DENSE_ZERO / DENSE_DEPTH_OUT, or DENSE_USED with the camera point (multiply, then divide)
ESL_DENSE_HD int dense_sample(unsigned raw, int col, int row, const double K[4], double depth_scale, double depth_min, double depth_max,
                              double pc[3]) {
  if (raw == 0) return DENSE_ZERO;
  const double z = (double)raw / depth_scale;
  if (z < depth_min || z > depth_max) return DENSE_DEPTH_OUT;
  pc[0] = ((double)col - K[2]) * z / K[0];
  pc[1] = ((double)row - K[3]) * z / K[1];
  pc[2] = z;
  return DENSE_USED;
}

// step 2: p_w = R^T (p_c - t), every component summed left to right
ESL_DENSE_HD void dense_world(const double P[kDensePose], const double pc[3], double pw[3]) {
  const double d0 = pc[0] - P[9], d1 = pc[1] - P[10], d2 = pc[2] - P[11];
  pw[0] = (P[0] * d0 + P[3] * d1) + P[6] * d2;
  pw[1] = (P[1] * d0 + P[4] * d1) + P[7] * d2;
  pw[2] = (P[2] * d0 + P[5] * d1) + P[8] * d2;
}

// step 3: k = floor(p_w / leaf); false when a component is out of range (a NaN or an infinity included)
ESL_DENSE_HD bool dense_key(const double pw[3], double leaf, int k[3]) {
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    const double f = std::floor(pw[a] / leaf);
    const bool in = std::fabs(f) <= (double)kDenseKeyMax;
    k[a] = in ? (int)f : 0;
    ok = ok && in;
  }
  return ok;
}
ESL_DENSE_HD bool dense_key_in_range(int kx, int ky, int kz) {
  return kx >= -kDenseKeyMax && kx <= kDenseKeyMax && ky >= -kDenseKeyMax && ky <= kDenseKeyMax && kz >= -kDenseKeyMax && kz <= kDenseKeyMax;
}
// the unsigned order of the packed key is the lexicographic order of (kx, ky, kz)
ESL_DENSE_HD unsigned long long dense_pack(int kx, int ky, int kz) {
  return ((unsigned long long)(kx + kDenseKeyOff) << 42) | ((unsigned long long)(ky + kDenseKeyOff) << 21) |
         (unsigned long long)(kz + kDenseKeyOff);
}
ESL_DENSE_HD void dense_unpack(unsigned long long key, int k[3]) {
  k[0] = (int)((key >> 42) & 0x1FFFFFull) - kDenseKeyOff;
  k[1] = (int)((key >> 21) & 0x1FFFFFull) - kDenseKeyOff;
  k[2] = (int)(key & 0x1FFFFFull) - kDenseKeyOff;
}

// The sample as k_dense_insert forms it: esl_dense_align_frames and esl_dense_carve_frames find the voxels that insertion made only
// while k_dense_insert, k_dal_accum and k_dcv_mark form it bit for bit alike.
// sample i of a frame, consecutive i on consecutive sampled columns: row < rows and col < cols for i < srows scols.  By value: with
// two output pointers the three kernels' listings change
struct DensePixel { int row, col; };
ESL_DENSE_HD DensePixel dense_sample_pixel(long long i, int stride, int scols) {
  const int sr = (int)(i / scols);
  return {sr * stride, (int)(i - (long long)sr * scols) * stride};
}
// steps 1 to 3 of one raw depth at (col, row): the category with DENSE_KEY_OUT folded in; pc, pw and k are set when it is DENSE_USED.
// k_dal_accum calls it; k_dense_insert and k_dcv_mark keep the three calls written out (tests/dense_key_main.cpp holds the two equal)
ESL_DENSE_HD int dense_sample_key(unsigned raw, int col, int row, const double K[4], double depth_scale, double depth_min, double depth_max,
                                  const double P[kDensePose], double leaf, double pc[3], double pw[3], int k[3]) {
  int cat = dense_sample(raw, col, row, K, depth_scale, depth_min, depth_max, pc);
  if (cat == DENSE_USED) {
    dense_world(P, pc, pw);
    if (!dense_key(pw, leaf, k)) cat = DENSE_KEY_OUT;
  }
  return cat;
}

// step 4: a coordinate's term of S_a (round to nearest, ties to even; the product with 2^30 is exact)
ESL_DENSE_HD long long dense_fix(double v) { return (long long)std::llrint(v * kDenseFix); }
// step 7: the centroid and the mean colour of a voxel
ESL_DENSE_HD double dense_mean(long long S, long long count) { return (double)S / kDenseFix / (double)count; }
ESL_DENSE_HD unsigned dense_color(unsigned long long sum, unsigned long long count) { return (unsigned)((2 * sum + count) / (2 * count)); }

}  // namespace esl
