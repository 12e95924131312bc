// esl_dense_proj.hpp — the per-(voxel, frame) arithmetic of esl_dense_render (include/esl.h, "viewing the dense map"; the steps' numbers
// below are the header's): the camera point and the depth gate (step 2), the six image coordinates, their range test and the footprint's
// pixel bounds (step 3), the quantised depth and the pixel's candidate word (step 4), the comparison class (step 6).  Plain C++ for host
// and device, no HIP include: tests/dense_render_main.cpp compiles it with an ordinary compiler.  Every translation unit that includes it
// is built with -ffp-contract=off: one fused multiply-add moves a pixel.
#pragma once
#include <cmath>
#include <cstdint>

#include "esl_dense_key.hpp"
#include "esl_render_ray.hpp"   // render_compare: step 6 is esl_render_map's, stated once

namespace esl {

constexpr double kDrnCoordMax = 1073741824.0;         // 2^30: an image coordinate beyond it (or not finite) puts the voxel outside
constexpr double kDrnZFix = 1048576.0;                // 2^20 units of zq per metre
constexpr double kDrnDepthMax = 4095.0;               // depth_max above this could take zq to 2^32
constexpr int kDrnMaxRadius = 64;                     // max_radius: 0 .. 64
constexpr unsigned long long kDrnEmpty = ~0ull;       // a pixel without a candidate; no candidate has zq = 2^32 - 1

enum { DRN_DRAWN = 0, DRN_DEPTH_OUT = 1, DRN_OUTSIDE = 2 };

// step 2: p_c = R p + t of a world point, every component summed left to right
ESL_DENSE_HD void drn_cam(const double P[kDensePose], const double p[3], double pc[3]) {
  pc[0] = ((P[0] * p[0] + P[1] * p[1]) + P[2] * p[2]) + P[9];
  pc[1] = ((P[3] * p[0] + P[4] * p[1]) + P[5] * p[2]) + P[10];
  pc[2] = ((P[6] * p[0] + P[7] * p[1]) + P[8] * p[2]) + P[11];
}
// the z of step 2 alone: what the resolve pass recomputes for the winner (the same operations, the same bits)
ESL_DENSE_HD double drn_cam_z(const double P[kDensePose], const double p[3]) { return ((P[6] * p[0] + P[7] * p[1]) + P[8] * p[2]) + P[11]; }
ESL_DENSE_HD bool drn_depth_in(double z, double depth_min, double depth_max) { return z >= depth_min && z <= depth_max; }   // a NaN fails

ESL_DENSE_HD bool drn_coord_ok(double v) { return std::fabs(v) <= kDrnCoordMax; }   // a NaN or an infinity fails

// step 3 along one axis: f, c = the focal length and the principal point, x = the camera point's coordinate, n = the image's size.
// false: a coordinate out of range, or no pixel.  Otherwise lo <= hi are the inclusive pixel bounds.  Multiply, then divide, then add;
// the bounds stay doubles (exact integers below 2^30 + 65) until the clip has brought them into the image.
ESL_DENSE_HD bool drn_axis(double f, double c, double x, double z, double e, int max_radius, int n, int* lo, int* hi) {
  const double u = (f * x) / z + c, u0 = (f * (x - e)) / z + c, u1 = (f * (x + e)) / z + c;
  if (!drn_coord_ok(u) || !drn_coord_ok(u0) || !drn_coord_ok(u1)) return false;
  const double col = std::floor(u + 0.5);
  double c0 = std::fmin(col, std::ceil(u0)), c1 = std::fmax(col, std::floor(u1));
  c0 = std::fmax(c0, col - (double)max_radius); c1 = std::fmin(c1, col + (double)max_radius);
  c0 = std::fmax(c0, 0.0); c1 = std::fmin(c1, (double)(n - 1));
  if (c0 > c1) return false;
  *lo = (int)c0; *hi = (int)c1;
  return true;
}

// steps 2 and 3 of one voxel in one frame: its class, its z and (DRN_DRAWN) the inclusive bounds box = {c0, c1, r0, r1}
ESL_DENSE_HD int drn_project(const double P[kDensePose], const double K[4], const double p[3], double e, int max_radius, int rows, int cols,
                             double depth_min, double depth_max, double* z_out, int box[4]) {
  double pc[3];
  drn_cam(P, p, pc);
  *z_out = pc[2];
  if (!drn_depth_in(pc[2], depth_min, depth_max)) return DRN_DEPTH_OUT;
  const bool okx = drn_axis(K[0], K[2], pc[0], pc[2], e, max_radius, cols, &box[0], &box[1]);
  const bool oky = drn_axis(K[1], K[3], pc[1], pc[2], e, max_radius, rows, &box[2], &box[3]);
  return okx && oky ? DRN_DRAWN : DRN_OUTSIDE;
}

// step 4: the pixel's candidate.  0 <= z <= 4095, so zq < 2^32; the smallest word is the nearest voxel, ties to the lowest index
ESL_DENSE_HD unsigned long long drn_zq(double z) { return (unsigned long long)std::llrint(z * kDrnZFix); }
ESL_DENSE_HD unsigned long long drn_word(double z, unsigned i) { return drn_zq(z) << 32 | (unsigned long long)i; }
ESL_DENSE_HD unsigned drn_word_index(unsigned long long w) { return (unsigned)(w & 0xFFFFFFFFull); }

// step 6: 0 agree, 1 nearer, 2 farther, 3 no data
ESL_DENSE_HD int drn_compare(unsigned raw, double z, double depth_scale, double depth_min, double depth_max, double depth_tol) {
  return render_compare(raw, z, depth_scale, depth_min, depth_max, depth_tol);
}

}  // namespace esl
