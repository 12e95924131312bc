// esl_dense_align.hpp — the per-voxel and per-sample arithmetic of esl_dense_normals and esl_dense_align_frames (include/esl.h, "normals of
// the dense map" steps N1 to N5 and "aligning frames to the dense map" steps a to e) and the host's Gauss-Newton step: the moments of a
// voxel's neighbourhood and its normal, the match's squared distance, the 28 fixed-point terms of a sample, the 6 x 6 solve and the pose
// update.  Plain C++ for host and device, no HIP include: tests/dense_align_main.cpp compiles it with an ordinary compiler.  Every
// translation unit that includes it is built with -ffp-contract=off: every output is compared with the numpy statement bit for bit.
// What is `inline` only runs on the host: one compiler decides every bit of a pose.
#pragma once
#include <cmath>
#include <cstdint>

#include "esl_dense_key.hpp"
#include "esl_dense_planes.hpp"   // dpl_jacobi_min: the project's one cyclic Jacobi

namespace esl {

constexpr int kDalSums = 28;      // 21 products J_a J_b (a <= b, row after row), 6 products J_a e, e^2: each llrint(x 2^30)
constexpr int kDalFold = 29;      // ... and the inlier count that is folded with them
constexpr int kDalRow = 37;       // a frame's row of one pass: the 29, then the eight counts
enum { DAL_FOLD_N = 28, DAL_SAMPLED = 29, DAL_ZERO, DAL_DEPTH_OUT, DAL_KEY_OUT, DAL_USED, DAL_NOMATCH, DAL_FAR, DAL_INLIER };
enum { DAL_MAX_ITERS = 0, DAL_CONVERGED = 1, DAL_TOO_FEW = 2, DAL_DEGENERATE = 3 };   // esl_dense_align_frame::status
enum { DAL_CLASS_NONE = -1, DAL_CLASS_NOMATCH = 0, DAL_CLASS_FAR = 1, DAL_CLASS_INLIER = 2 };
constexpr int kDalMaxIters = 64, kDalMaxReach = 2, kDnrMaxRadius = 2;

// step N3: one neighbour's terms, one product and one add at a time; M = {xx, xy, xz, yy, yz, zz}
ESL_DENSE_HD void dnr_add(const double ci[3], const double cj[3], int* m, double s[3], double M[6]) {
  const double d0 = cj[0] - ci[0], d1 = cj[1] - ci[1], d2 = cj[2] - ci[2];
  s[0] = s[0] + d0; s[1] = s[1] + d1; s[2] = s[2] + d2;
  M[0] = M[0] + d0 * d0; M[1] = M[1] + d0 * d1; M[2] = M[2] + d0 * d2;
  M[3] = M[3] + d1 * d1; M[4] = M[4] + d1 * d2; M[5] = M[5] + d2 * d2;
  *m += 1;
}

// steps N3 to N5: C, the normal, the curvature and the validity of a voxel with m >= 1 neighbours.  An invalid voxel: n = 0, curv = NaN
ESL_DENSE_HD bool dnr_finish(int m, const double s[3], const double M[6], int min_neighbors, double max_curvature, double n[3], double* curv) {
  n[0] = n[1] = n[2] = 0;
  *curv = std::nan("");
  if (m < 1 || m < min_neighbors) return false;
  const double dm = (double)m;
  const double u0 = s[0] / dm, u1 = s[1] / dm, u2 = s[2] / dm;
  const double C[6] = {M[0] / dm - u0 * u0, M[1] / dm - u0 * u1, M[2] / dm - u0 * u2, M[3] / dm - u1 * u1, M[4] / dm - u1 * u2, M[5] / dm - u2 * u2};
  const double trace = (C[0] + C[3]) + C[5];
  if (!(trace > 0)) return false;
  double w[3];
  dpl_jacobi_min(C, w);
  bool flip = false;   // the first non-zero component positive
  if (w[0] != 0) flip = w[0] < 0;
  else if (w[1] != 0) flip = w[1] < 0;
  else flip = w[2] < 0;
  if (flip) { w[0] = -w[0]; w[1] = -w[1]; w[2] = -w[2]; }
  const double c0 = (C[0] * w[0] + C[1] * w[1]) + C[2] * w[2];
  const double c1 = (C[1] * w[0] + C[3] * w[1]) + C[4] * w[2];
  const double c2 = (C[2] * w[0] + C[4] * w[1]) + C[5] * w[2];
  const double lam = (w[0] * c0 + w[1] * c1) + w[2] * c2;
  const double cv = lam / trace;
  if (!(cv <= max_curvature)) return false;
  n[0] = w[0]; n[1] = w[1]; n[2] = w[2];
  *curv = cv;
  return true;
}

// step b: the squared distance of a sample to a centroid, summed left to right.  The match is the candidate with the smallest one;
// candidates are visited in ascending packed-key order and replace the best only when strictly nearer: ties go to the smallest key
ESL_DENSE_HD double dal_dist2(const double pw[3], const double c[3]) {
  const double r0 = pw[0] - c[0], r1 = pw[1] - c[1], r2 = pw[2] - c[2];
  return (r0 * r0 + r1 * r1) + r2 * r2;
}
ESL_DENSE_HD int dal_class(bool matched, double d2, double max_dist2) {
  if (!matched) return DAL_CLASS_NOMATCH;
  return d2 > max_dist2 ? DAL_CLASS_FAR : DAL_CLASS_INLIER;
}
// step b: max_dist = 0 means (reach + 1) leaf; the gate is the square of that, one double computed on the host
inline double dal_max_dist2(double max_dist, int reach, double leaf) {
  const double d = max_dist > 0 ? max_dist : (double)(reach + 1) * leaf;
  return d * d;
}

// step c: the camera centre o = R^T (0 - t), dense_world of p_c = 0
ESL_DENSE_HD void dal_centre(const double P[kDensePose], double o[3]) {
  const double z[3] = {0, 0, 0};
  dense_world(P, z, o);
}

// step c: the 28 terms of an inlier with the world point pw, the match's centroid c and normal n
ESL_DENSE_HD void dal_terms(const double pw[3], const double o[3], const double c[3], const double n[3], long long T[kDalSums]) {
  const double q0 = pw[0] - o[0], q1 = pw[1] - o[1], q2 = pw[2] - o[2];
  const double r0 = pw[0] - c[0], r1 = pw[1] - c[1], r2 = pw[2] - c[2];
  const double e = (n[0] * r0 + n[1] * r1) + n[2] * r2;
  const double J[6] = {n[0], n[1], n[2], q1 * n[2] - q2 * n[1], q2 * n[0] - q0 * n[2], q0 * n[1] - q1 * n[0]};
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) T[k++] = dense_fix(J[a] * J[b]);
  for (int a = 0; a < 6; ++a) T[21 + a] = dense_fix(J[a] * e);
  T[27] = dense_fix(e * e);
}

// step c: Q, the bound on |q| = |p_c| of a used sample and on every |J_a| and |e|: the farthest pixel corner at depth_max, no less than 1
// (|n| = 1) and than sqrt(max_dist2) (|e| <= the match's distance), widened by 2^-20 for R's rounding
inline double dal_bound(const double K[4], int rows, int cols, double depth_max, double max_dist2) {
  const double x = std::fmax(std::fabs(0.0 - K[2]), std::fabs((double)(cols - 1) - K[2])) / K[0];
  const double y = std::fmax(std::fabs(0.0 - K[3]), std::fabs((double)(rows - 1) - K[3])) / K[1];
  const double far = std::fabs(depth_max) * std::sqrt((1.0 + x * x) + y * y);
  return std::fmax(std::fmax(1.0, far), std::sqrt(max_dist2)) * (1.0 + 1.0 / 1048576.0);
}
// false: the sums of a frame with n_sampled pixels could reach 2^62 (a NaN bound fails too)
inline bool dal_sums_fit(long long n_sampled, double Q) {
  return (double)n_sampled * (Q * Q * kDenseFix + 1.0) < 4611686018427387904.0;
}

// step d: H (6 x 6, row-major, symmetric) and g from the sums
inline void dal_system(const long long T[kDalSums], double H[36], double g[6]) {
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      const double v = (double)T[k++] / kDenseFix;
      H[a * 6 + b] = v; H[b * 6 + a] = v;
    }
  for (int a = 0; a < 6; ++a) g[a] = (double)T[21 + a] / kDenseFix;
}

// step d: (H + damping diag H) delta = -g by a Cholesky factorisation, every sum taken term after term.  DAL_TOO_FEW / DAL_DEGENERATE,
// or 0 with delta = (v, omega)
inline int dal_solve(const double H[36], const double g[6], long long n_inlier, int min_inliers, double damping, double min_pivot_ratio,
                     double delta[6]) {
  for (int a = 0; a < 6; ++a) delta[a] = 0;
  if (n_inlier < (long long)min_inliers) return DAL_TOO_FEW;
  double A[36], L[36];
  for (int a = 0; a < 36; ++a) { A[a] = H[a]; L[a] = 0; }
  double dmax = 0;
  for (int a = 0; a < 6; ++a) {
    A[a * 6 + a] = H[a * 6 + a] + damping * H[a * 6 + a];
    if (a == 0 || A[a * 6 + a] > dmax) dmax = A[a * 6 + a];
  }
  const double floor_ = min_pivot_ratio * dmax;
  for (int j = 0; j < 6; ++j) {
    double piv = A[j * 6 + j];
    for (int k = 0; k < j; ++k) piv = piv - L[j * 6 + k] * L[j * 6 + k];
    if (!(piv > 0) || !(piv >= floor_)) return DAL_DEGENERATE;
    const double ljj = std::sqrt(piv);
    L[j * 6 + j] = ljj;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i * 6 + j];
      for (int k = 0; k < j; ++k) v = v - L[i * 6 + k] * L[j * 6 + k];
      L[i * 6 + j] = v / ljj;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double v = -g[i];
    for (int k = 0; k < i; ++k) v = v - L[i * 6 + k] * y[k];
    y[i] = v / L[i * 6 + i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v = v - L[k * 6 + i] * delta[k];
    delta[i] = v / L[i * 6 + i];
  }
  for (int a = 0; a < 6; ++a) if (!std::isfinite(delta[a])) return DAL_DEGENERATE;
  return 0;
}

inline double dal_norm3(const double v[3]) { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// step d: the pose after delta = (v, omega).  q is divided by its norm as dense_pose divides it; dq = (omega / 2, 1) / its norm;
// q_new = q (x) conj(dq) (Hamilton, (x, y, z, w)); o_new = o + v; t_new = -(R_new o_new).  No sine or cosine.  false: the new pose is
// not a valid one (the frame is reported as degenerate and keeps its pose)
inline bool dal_update(const double cam[7], const double delta[6], double out[7]) {
  double P[kDensePose], o[3];
  for (int a = 0; a < 7; ++a) out[a] = cam[a];
  if (!dense_pose(cam, P)) return false;
  dal_centre(P, o);
  const double nrm = std::sqrt(cam[3] * cam[3] + cam[4] * cam[4] + cam[5] * cam[5] + cam[6] * cam[6]);
  const double ax = cam[3] / nrm, ay = cam[4] / nrm, az = cam[5] / nrm, aw = cam[6] / nrm;
  const double hx = delta[3] / 2, hy = delta[4] / 2, hz = delta[5] / 2;
  const double dn = std::sqrt(((hx * hx + hy * hy) + hz * hz) + 1.0);
  const double bx = -(hx / dn), by = -(hy / dn), bz = -(hz / dn), bw = 1.0 / dn;   // conj(dq)
  double c[7];
  c[3] = ((aw * bx + ax * bw) + ay * bz) - az * by;
  c[4] = ((aw * by - ax * bz) + ay * bw) + az * bx;
  c[5] = ((aw * bz + ax * by) - ay * bx) + az * bw;
  c[6] = ((aw * bw - ax * bx) - ay * by) - az * bz;
  c[0] = c[1] = c[2] = 0;
  double Pn[kDensePose];
  if (!dense_pose(c, Pn)) return false;
  const double o0 = o[0] + delta[0], o1 = o[1] + delta[1], o2 = o[2] + delta[2];
  c[0] = -((Pn[0] * o0 + Pn[1] * o1) + Pn[2] * o2);
  c[1] = -((Pn[3] * o0 + Pn[4] * o1) + Pn[5] * o2);
  c[2] = -((Pn[6] * o0 + Pn[7] * o1) + Pn[8] * o2);
  for (int a = 0; a < 7; ++a) if (!std::isfinite(c[a])) return false;
  for (int a = 0; a < 7; ++a) out[a] = c[a];
  return true;
}

// step d: the frame stops early when |v| <= tol_t and |omega| <= tol_r
inline bool dal_converged(const double delta[6], double tol_t, double tol_r) {
  return dal_norm3(delta) <= tol_t && dal_norm3(delta + 3) <= tol_r;
}

}  // namespace esl
