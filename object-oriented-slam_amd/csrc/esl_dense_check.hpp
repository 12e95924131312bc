// esl_dense_check.hpp — what the entries that read the dense map refuse for a parameter's value alone, stated once: the image geometry
// (esl_dense_add / _remove / _move_frames, esl_dense_render, esl_dense_align_frames, esl_dense_carve_frames, esl_dense_covis_frames), the
// depth gate (render, carve and covis) and one function per parameter struct.  Every function gives the text of the first refusal in the order the entry keeps, or
// nullptr; the entry does  if (const char* m = ...) return dense_fail(ESL_ERR_INVALID, who, m);  What needs the context, the map's state
// or the caller's pointers stays in the entry.  Plain C++ for the host, no HIP include: tests/dense_*_main.cpp run these functions
// with an ordinary compiler (mode "check").
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/esl.h"
#include "esl_dense_align.hpp"
#include "esl_dense_carve.hpp"
#include "esl_dense_covis.hpp"
#include "esl_dense_key.hpp"
#include "esl_dense_proj.hpp"

namespace esl {

inline bool dense_nonneg(double v) { return std::isfinite(v) && v >= 0; }

// K and the image's size; cx and cy are free here (esl_dense_align_frames asks them to be finite, directly after)
inline const char* dense_image_check(const double K[4], int32_t rows, int32_t cols) {
  if (!K) return "null K";
  if (rows < 1 || rows > kDenseMaxDim) return "rows < 1 or > 16384";
  if (cols < 1 || cols > kDenseMaxDim) return "cols < 1 or > 16384";
  if (!std::isfinite(K[0]) || !(K[0] > 0)) return "fx not finite or <= 0";
  if (!std::isfinite(K[1]) || !(K[1] > 0)) return "fy not finite or <= 0";
  return nullptr;
}

// the gate on a measured depth: esl_dense_render's depth_meas, esl_dense_carve_frames' depth_obs
inline const char* dense_gate_check(double depth_scale, double depth_min, double depth_max, double depth_tol) {
  if (!std::isfinite(depth_scale) || !(depth_scale > 0)) return "depth_scale not finite or <= 0";
  if (!dense_nonneg(depth_min)) return "depth_min not finite or negative";
  if (!dense_nonneg(depth_max)) return "depth_max not finite or negative";
  if (!dense_nonneg(depth_tol)) return "depth_tol not finite or negative";
  if (depth_min > depth_max) return "depth_min > depth_max";
  if (depth_max > kDrnDepthMax) return "depth_max > 4095";
  return nullptr;
}

// npix = rows cols of an image that dense_image_check has passed
inline const char* drn_params_check(const esl_dense_render_params& p, size_t npix) {
  if (const char* m = dense_gate_check(p.depth_scale, p.depth_min, p.depth_max, p.depth_tol)) return m;
  if (!dense_nonneg(p.footprint)) return "footprint not finite or negative";
  if (p.max_radius < 0 || p.max_radius > kDrnMaxRadius) return "max_radius outside 0 .. 64";
  if (p.min_count < 1) return "min_count < 1";
  if (p.zbuf_bytes < (int64_t)(8 * npix)) return "zbuf_bytes < 8 rows cols";
  return nullptr;
}

inline const char* dcv_params_check(const esl_dense_carve_params& p) {
  if (const char* m = dense_gate_check(p.depth_scale, p.depth_min, p.depth_max, p.depth_tol)) return m;
  if (p.window < 0 || p.window > kDcvMaxWindow) return "window outside 0 .. 4";
  if (p.min_through < 1) return "min_through < 1";
  if (p.through_per_agree < 0) return "negative through_per_agree";
  if (p.apply != 0 && p.apply != 1) return "apply not 0 or 1";
  return nullptr;
}

inline const char* dco_params_check(const esl_dense_covis_params& p) {
  if (const char* m = dense_gate_check(p.depth_scale, p.depth_min, p.depth_max, p.depth_tol)) return m;
  if (p.window < 0 || p.window > kDcvMaxWindow) return "window outside 0 .. 4";
  if (p.min_others < 1) return "min_others < 1";
  if (p.cover_den < 1 || p.cover_den > kDcoMaxCoverDen) return "cover_den outside 1 .. 2^20";
  if (p.cover_num < 0 || p.cover_num > p.cover_den) return "cover_num outside 0 .. cover_den";
  if (p.max_cull < 0) return "negative max_cull";
  if (p.reserved != 0) return "reserved not 0";
  return nullptr;
}

inline const char* dnr_params_check(const esl_dense_normal_params& p) {
  if (!dense_nonneg(p.max_curvature)) return "max_curvature not finite or negative";
  if (p.radius < 1 || p.radius > kDnrMaxRadius) return "radius outside 1 .. 2";
  if (p.min_count < 1) return "min_count < 1";
  if (p.min_neighbors < 1) return "min_neighbors < 1";
  return nullptr;
}

inline const char* dal_params_check(const esl_dense_align_params& p) {
  if (!dense_nonneg(p.max_dist)) return "max_dist not finite or negative";
  if (!dense_nonneg(p.damping)) return "damping not finite or negative";
  if (!dense_nonneg(p.min_pivot_ratio)) return "min_pivot_ratio not finite or negative";
  if (!dense_nonneg(p.tol_t)) return "tol_t not finite or negative";
  if (!dense_nonneg(p.tol_r)) return "tol_r not finite or negative";
  if (p.iters < 0 || p.iters > kDalMaxIters) return "iters outside 0 .. 64";
  if (p.stride < 1) return "stride < 1";
  if (p.reach < 0 || p.reach > kDalMaxReach) return "reach outside 0 .. 2";
  if (p.min_inliers < 1) return "min_inliers < 1";
  return dnr_params_check(p.normals);
}

}  // namespace esl
