// esl_render_ray.hpp — the per-ray arithmetic of esl_render_map (include/esl.h, "rendering the map"; the steps' numbers below are the
// header's): validity of a map row (step 1), the camera-frame body A, g, c0 from the columns of [Rco | tco] (step 2), the ray of a pixel
// and its nearest hit (step 3), and the pixel bounds the tile kernel culls with.  Plain C++ for host and device, no HIP include:
// tests/render_ray_main.cpp compiles it with an ordinary compiler.  Rco / tco and the outline's box are NOT formed here: the kernel takes
// them from box_geom and box_from_conic (esl_math.hpp), the stand-alone program reads them.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ESL_RENDER_HD __host__ __device__ inline
#else
#define ESL_RENDER_HD inline
#endif

namespace esl {

constexpr int kRenderMaxDim = 16384;   // rows, cols
enum { RENDER_DRAWN = 1, RENDER_INVALID = 2, RENDER_INSIDE = 4, RENDER_BOUNDED = 8 };   // flags_out

// what a ray needs of one (frame, object): A packed (00 01 02 11 12 22), g, c0
constexpr int kRenderBody = 10;
struct RenderRec {
  double b[kRenderBody];
  int x0, x1, y0, y1;   // inclusive pixel bounds; x1 < x0: no pixel
};

// step 1.  q = the normalised quaternion (x y z w), s = |half-axes|
ESL_RENDER_HD bool render_valid(const double v[10], double q[4], double s[3]) {
  bool ok = true;
  for (int k = 0; k < 10; ++k) ok = ok && std::isfinite(v[k]);
  const double nrm = std::sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6]);
  s[0] = std::fabs(v[7]); s[1] = std::fabs(v[8]); s[2] = std::fabs(v[9]);
  ok = ok && std::isfinite(nrm) && nrm > 0 && s[0] > 0 && s[1] > 0 && s[2] > 0;
  if (!ok) return false;
  q[0] = v[3] / nrm; q[1] = v[4] / nrm; q[2] = v[5] / nrm; q[3] = v[6] / nrm;
  return true;
}

// step 2.  n[k] = column k of Rco (k < 3), n[3] = tco: BoxGeom::n.  A = Rco diag(1 / s^2) Rco^T, g = A tco, c0 = tco^T A tco - 1
ESL_RENDER_HD void render_body(const double n[4][3], const double s[3], double b[kRenderBody]) {
  const double w0 = 1.0 / (s[0] * s[0]), w1 = 1.0 / (s[1] * s[1]), w2 = 1.0 / (s[2] * s[2]);
  const double* t = n[3];
#define ESL_AIJ(i, j) (w0 * n[0][i] * n[0][j] + w1 * n[1][i] * n[1][j] + w2 * n[2][i] * n[2][j])
  b[0] = ESL_AIJ(0, 0); b[1] = ESL_AIJ(0, 1); b[2] = ESL_AIJ(0, 2);
  b[3] = ESL_AIJ(1, 1); b[4] = ESL_AIJ(1, 2); b[5] = ESL_AIJ(2, 2);
#undef ESL_AIJ
  b[6] = b[0] * t[0] + b[1] * t[1] + b[2] * t[2];
  b[7] = b[1] * t[0] + b[3] * t[1] + b[4] * t[2];
  b[8] = b[2] * t[0] + b[4] * t[1] + b[5] * t[2];
  b[9] = (b[6] * t[0] + b[7] * t[1] + b[8] * t[2]) - 1.0;
}

// step 3: the ray of pixel (col, row), d = ((col - cx) / fx, (row - cy) / fy, 1), integer pixels, as the monomials of d that the
// quadratic form takes: what does not depend on the body is formed once per pixel, and a test is eleven multiply-adds
struct RenderRay { double x, y, xx, xy2, x2, yy, y2; };
ESL_RENDER_HD RenderRay render_ray(const double K[4], int col, int row) {
  RenderRay d;
  d.x = ((double)col - K[2]) / K[0];
  d.y = ((double)row - K[3]) / K[1];
  d.xx = d.x * d.x; d.xy2 = 2.0 * d.x * d.y; d.x2 = 2.0 * d.x; d.yy = d.y * d.y; d.y2 = 2.0 * d.y;
  return d;
}

// step 3: hit iff beta > 0 and Delta > 0, both strict
ESL_RENDER_HD bool render_hit_terms(const double b[kRenderBody], const RenderRay& d, double& beta, double& delta) {
  const double alpha = b[0] * d.xx + b[1] * d.xy2 + b[2] * d.x2 + b[3] * d.yy + b[4] * d.y2 + b[5];
  beta = b[6] * d.x + b[7] * d.y + b[8];
  delta = beta * beta - alpha * b[9];
  return beta > 0 && delta > 0;
}
// the depth of a hit: z = c0 / (beta + sqrt(Delta))
ESL_RENDER_HD double render_depth(double c0, double beta, double delta) { return c0 / (beta + std::sqrt(delta)); }

ESL_RENDER_HD bool render_hit(const double b[kRenderBody], const RenderRay& d, double& z) {
  double beta, delta;
  if (!render_hit_terms(b, d, beta, delta)) return false;
  z = render_depth(b[9], beta, delta);
  return true;
}

// A hit that cannot win against the pixel's running minimum `best`, decided without the square root and the division (an FP64 root and
// quotient cost more than the whole test).  Delta <= beta^2 gives sqrt(Delta) <= beta up to an ulp, so beta + sqrt(Delta) <= 2 beta and
// render_depth(...) >= c0 / (2 beta) up to a few ulp; the factor's excess over 2 (1e-7) is a million times those ulps.  So true here
// implies render_depth(...) > best: leaving the hit out of the minimum changes no bit of any result.  best = +inf: never true.
// (A bound tight to 1e-6, from a single-precision root, was measured too: it rejects more hits but only a wave whose 64 lanes all
// reject saves anything, and its own instructions cost more than that gained -- DESIGN 4.24.)
ESL_RENDER_HD bool render_behind(double c0, double beta, double delta, double best) {
  return delta <= beta * beta && c0 > best * (2.0000002 * beta);
}

// The flags of a valid body and its pixel bounds.  bb = box_from_conic's box (NaN when the outline is no ellipse), C22 = the dual conic's
// last entry, tz = tco_z.  c0 <= 0: the camera centre is inside or on the body, nothing drawn.  C22 < 0 says the body does not meet the
// principal plane: with tz < 0 it lies wholly behind (no pixel, no flag), with tz > 0 wholly in front, every hit pixel lies inside the
// outline and the bounds are its box widened by a pixel and clipped.  Otherwise the whole image.  The bounds only cull.
ESL_RENDER_HD int render_bounds(const double bb[4], double C22, double tz, double c0, int rows, int cols, int& x0, int& x1, int& y0,
                                int& y1) {
  x0 = 0; x1 = -1; y0 = 0; y1 = -1;
  if (!(c0 > 0)) return RENDER_INSIDE;
  if (C22 < 0 && tz < 0) return 0;
  const bool fin = std::isfinite(bb[0]) && std::isfinite(bb[1]) && std::isfinite(bb[2]) && std::isfinite(bb[3]);
  if (C22 < 0 && tz > 0 && fin) {
    // clamped as doubles first: the box of a body far outside the image does not fit an int
    const double fx0 = std::fmax(std::floor(bb[0]) - 1.0, 0.0), fx1 = std::fmin(std::ceil(bb[2]) + 1.0, (double)(cols - 1));
    const double fy0 = std::fmax(std::floor(bb[1]) - 1.0, 0.0), fy1 = std::fmin(std::ceil(bb[3]) + 1.0, (double)(rows - 1));
    if (fx0 <= fx1 && fy0 <= fy1) { x0 = (int)fx0; x1 = (int)fx1; y0 = (int)fy0; y1 = (int)fy1; }
    return RENDER_DRAWN | RENDER_BOUNDED;
  }
  x0 = 0; x1 = cols - 1; y0 = 0; y1 = rows - 1;
  return RENDER_DRAWN;
}

// step 6: 0 agree, 1 nearer, 2 farther, 3 no data
ESL_RENDER_HD int render_compare(unsigned raw, double z, double depth_scale, double depth_min, double depth_max, double depth_tol) {
  const double zm = (double)raw / depth_scale;
  if (raw == 0 || !(zm >= depth_min) || !(zm <= depth_max)) return 3;
  if (std::fabs(zm - z) <= depth_tol) return 0;
  return zm < z - depth_tol ? 1 : 2;
}

}  // namespace esl
