// esl_dense_carve.hpp — the per-(voxel, frame) arithmetic of esl_dense_carve_frames (include/esl.h, "carving the dense map"; the steps'
// numbers below are the header's): the observation of a voxel in an observer frame (step C2) and the verdict on a voxel's counts (step
// C4).  Built on esl_dense_proj.hpp's camera point, depth gate, coordinate test and comparison class, none of which is restated here.
// Plain C++ for host and device, no HIP include: tests/dense_carve_main.cpp compiles it with an ordinary compiler.  Every translation
// unit that includes it is built with -ffp-contract=off: one fused multiply-add moves the centre pixel.
#pragma once
#include "esl_dense_proj.hpp"

namespace esl {

constexpr int kDcvMaxWindow = 4;        // window: 0 .. 4, so a window holds at most 9 x 9 pixels
constexpr int kDcvChunk = 32;           // observer frames per chunk of k_dcv_observe
constexpr int kDcvMaxObs = 65535;       // F_obs: a voxel's four counts live in 16 bits each and sum to at most F_obs

// the class of one observation; the first four are vox_out's columns
enum { DCV_AGREE = 0, DCV_NEARER = 1, DCV_THROUGH = 2, DCV_NODATA = 3, DCV_DEPTH_OUT = 4, DCV_OUTSIDE = 5 };

// step C2: voxel p seen from the frame with pose P and the measured depth image `depth` (rows x cols raw values)
ESL_DENSE_HD int dcv_observe(const double P[kDensePose], const double K[4], const double p[3], const unsigned short* depth, int rows, int cols,
                             int window, double depth_scale, double depth_min, double depth_max, double depth_tol) {
  double pc[3];
  drn_cam(P, p, pc);
  const double z = pc[2];
  if (!drn_depth_in(z, depth_min, depth_max)) return DCV_DEPTH_OUT;
  const double u = (K[0] * pc[0]) / z + K[2], v = (K[1] * pc[1]) / z + K[3];   // multiply, then divide, then add
  if (!drn_coord_ok(u) || !drn_coord_ok(v)) return DCV_OUTSIDE;
  const double col = std::floor(u + 0.5), row = std::floor(v + 0.5);   // compared as doubles: exact integers below 2^30 + 1
  if (!(col >= 0.0 && col <= (double)(cols - 1) && row >= 0.0 && row <= (double)(rows - 1))) return DCV_OUTSIDE;
  const int c = (int)col, r = (int)row;
  const int c0 = c - window < 0 ? 0 : c - window, c1 = c + window > cols - 1 ? cols - 1 : c + window;
  const int r0 = r - window < 0 ? 0 : r - window, r1 = r + window > rows - 1 ? rows - 1 : r + window;
  bool nearer = false, through = false;
  // at most (2 window + 1)^2 <= 81 pixels, all inside the image
  for (int y = r0; y <= r1; ++y) {
    const unsigned short* line = depth + (size_t)y * cols;
    for (int x = c0; x <= c1; ++x) {
      const int cat = render_compare(line[x], z, depth_scale, depth_min, depth_max, depth_tol);
      if (cat == 0) return DCV_AGREE;   // agree wins over every other pixel of the window
      nearer = nearer || cat == 1;
      through = through || cat == 2;
    }
  }
  return nearer ? DCV_NEARER : through ? DCV_THROUGH : DCV_NODATA;
}

// step C4: the product as a 64-bit integer
ESL_DENSE_HD bool dcv_verdict(int agree, int through, int min_through, int through_per_agree) {
  return through >= min_through && (long long)through >= (long long)through_per_agree * (long long)agree;
}

// a voxel's four counts as one 64-bit word, 16 bits each in DCV_AGREE .. DCV_NODATA's order
ESL_DENSE_HD unsigned long long dcv_pack_one(int cls) { return 1ull << (16 * cls); }
ESL_DENSE_HD int dcv_unpack(unsigned long long w, int cls) { return (int)((w >> (16 * cls)) & 0xFFFFull); }

}  // namespace esl
