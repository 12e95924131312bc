// esl_math.hpp — fp64 device arithmetic of the EllipsoidSLAM hot path for gfx950.
//
// Everything here is per-lane scalar fp64 (the path is small-matrix algebra per edge; MFMA is
// reserved for the dense reduced-camera solve).  Functions name the reference routine whose
// result they reproduce (paths relative to the reference tree):
//   SE3 exp/log/product        Thirdparty/g2o/g2o/types/se3quat.h:110-134, 229-322
//   ellipsoid retraction       src/core/Ellipsoid.cpp:38-47
//   bbox of projected quadric  src/core/Ellipsoid.cpp:209-307 — evaluated here with the closed-form
//                              tangent lines of the dual conic C* = P Q* P^T (no 3x3 inverse, no atan2):
//                              x = (C02 -/+ sqrt(C02^2 - C00 C22)) / C22, y likewise with index 1
//   9-DoF log error, 4 yaws    src/core/Ellipsoid.cpp:63-117
//   gravity prior              src/core/BasicEllipsoidEdges.cpp:129-152
//   odometry                   Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:90-99
#pragma once
#include <hip/hip_runtime.h>

#define ESL_HD __host__ __device__ __forceinline__

namespace esl {

struct Quat { double x, y, z, w; };
struct SE3 { Quat r; double t[3]; };
struct Ell { SE3 pose; double s[3]; };
struct Mat3 { double m[9]; };  // row-major

ESL_HD Quat q_mul(const Quat& a, const Quat& b) {
  Quat r;
  r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
  r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
  return r;
}
ESL_HD Quat q_conj(const Quat& a) { return Quat{-a.x, -a.y, -a.z, a.w}; }

ESL_HD void q_rot(const Quat& q, const double v[3], double out[3]) {
  double ux = q.y * v[2] - q.z * v[1], uy = q.z * v[0] - q.x * v[2], uz = q.x * v[1] - q.y * v[0];
  ux += ux; uy += uy; uz += uz;
  out[0] = v[0] + q.w * ux + (q.y * uz - q.z * uy);
  out[1] = v[1] + q.w * uy + (q.z * ux - q.x * uz);
  out[2] = v[2] + q.w * uz + (q.x * uy - q.y * ux);
}

ESL_HD Mat3 q_to_R(const Quat& q) {
  Mat3 R;
  double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  R.m[0] = 1 - (tyy + tzz); R.m[1] = txy - twz;       R.m[2] = txz + twy;
  R.m[3] = txy + twz;       R.m[4] = 1 - (txx + tzz); R.m[5] = tyz - twx;
  R.m[6] = txz - twy;       R.m[7] = tyz + twx;       R.m[8] = 1 - (txx + tyy);
  return R;
}

// rotation matrix -> quaternion; branch on the largest diagonal combination
ESL_HD Quat q_from_R(const Mat3& Rm) {
  const double* R = Rm.m;
  Quat q;
  double t = R[0] + R[4] + R[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q.w = 0.5 * t;
    t = 0.5 / t;
    q.x = (R[7] - R[5]) * t; q.y = (R[2] - R[6]) * t; q.z = (R[3] - R[1]) * t;
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    t = sqrt(R[0] - R[4] - R[8] + 1.0);
    q.x = 0.5 * t; t = 0.5 / t;
    q.w = (R[7] - R[5]) * t; q.y = (R[3] + R[1]) * t; q.z = (R[6] + R[2]) * t;
  } else if (R[4] >= R[8]) {
    t = sqrt(R[4] - R[8] - R[0] + 1.0);
    q.y = 0.5 * t; t = 0.5 / t;
    q.w = (R[2] - R[6]) * t; q.z = (R[7] + R[5]) * t; q.x = (R[1] + R[3]) * t;
  } else {
    t = sqrt(R[8] - R[0] - R[4] + 1.0);
    q.z = 0.5 * t; t = 0.5 / t;
    q.w = (R[3] - R[1]) * t; q.x = (R[2] + R[6]) * t; q.y = (R[5] + R[7]) * t;
  }
  return q;
}

// SE3Quat::normalizeRotation: w >= 0, unit norm
ESL_HD Quat q_normalize_pos(Quat q) {
  if (q.w < 0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
  const double inv = 1.0 / sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);  // one reciprocal, not four divisions
  q.x *= inv; q.y *= inv; q.z *= inv; q.w *= inv;
  return q;
}

ESL_HD SE3 se3_load(const double* v) {
  SE3 T;
  T.t[0] = v[0]; T.t[1] = v[1]; T.t[2] = v[2];
  T.r.x = v[3]; T.r.y = v[4]; T.r.z = v[5]; T.r.w = v[6];
  return T;
}
ESL_HD void se3_store(const SE3& T, double* v) {
  v[0] = T.t[0]; v[1] = T.t[1]; v[2] = T.t[2];
  v[3] = T.r.x; v[4] = T.r.y; v[5] = T.r.z; v[6] = T.r.w;
}
ESL_HD Ell ell_load(const double* v) {
  Ell e;
  e.pose = se3_load(v);
  e.s[0] = v[7]; e.s[1] = v[8]; e.s[2] = v[9];
  return e;
}
ESL_HD void ell_store(const Ell& e, double* v) {
  se3_store(e.pose, v);
  v[7] = e.s[0]; v[8] = e.s[1]; v[9] = e.s[2];
}

ESL_HD SE3 se3_mul(const SE3& A, const SE3& B) {
  SE3 R;
  double rt[3];
  q_rot(A.r, B.t, rt);
  R.t[0] = A.t[0] + rt[0]; R.t[1] = A.t[1] + rt[1]; R.t[2] = A.t[2] + rt[2];
  R.r = q_normalize_pos(q_mul(A.r, B.r));
  return R;
}
ESL_HD SE3 se3_inv(const SE3& A) {
  SE3 R;
  R.r = q_conj(A.r);
  double nt[3] = {-A.t[0], -A.t[1], -A.t[2]};
  q_rot(R.r, nt, R.t);
  return R;
}

ESL_HD Mat3 skew(const double v[3]) {
  Mat3 m;
  m.m[0] = 0;     m.m[1] = -v[2]; m.m[2] = v[1];
  m.m[3] = v[2];  m.m[4] = 0;     m.m[5] = -v[0];
  m.m[6] = -v[1]; m.m[7] = v[0];  m.m[8] = 0;
  return m;
}
ESL_HD Mat3 m3_mul(const Mat3& a, const Mat3& b) {
  Mat3 c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      c.m[i * 3 + j] = a.m[i * 3] * b.m[j] + a.m[i * 3 + 1] * b.m[3 + j] + a.m[i * 3 + 2] * b.m[6 + j];
  return c;
}
ESL_HD void m3_vec(const Mat3& a, const double v[3], double o[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = a.m[i * 3] * v[0] + a.m[i * 3 + 1] * v[1] + a.m[i * 3 + 2] * v[2];
}

// SE3Quat::exp including g2o's small-angle branch (R = I + W + W^2, V = R)
ESL_HD SE3 se3_exp(const double u[6]) {
  const double w[3] = {u[0], u[1], u[2]}, ups[3] = {u[3], u[4], u[5]};
  const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const Mat3 Om = skew(w);
  const Mat3 Om2 = m3_mul(Om, Om);
  double a, b, c, bv;
  if (theta < 0.00001) { a = 1.0; b = 1.0; bv = 1.0; c = 1.0; }
  else {
    const double st = sin(theta), ct = cos(theta);
    a = st / theta; b = (1 - ct) / (theta * theta); bv = b; c = (theta - st) / (theta * theta * theta);
  }
  Mat3 R, V;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double id = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
    R.m[i] = id + a * Om.m[i] + b * Om2.m[i];
    V.m[i] = (theta < 0.00001) ? R.m[i] : (id + bv * Om.m[i] + c * Om2.m[i]);
  }
  SE3 T;
  T.r = q_normalize_pos(q_from_R(R));
  m3_vec(V, ups, T.t);
  return T;
}

// Coefficients of SE3Quat::log (se3quat.h:205-240) from d = (trace R - 1) / 2:
//   omega = f * vee(R - R^T),  f = theta / (2 sin theta);   V^-1 = I - Omega/2 + c Omega^2,
//   c = (1 - theta / (2 tan(theta/2))) / theta^2.   tan(theta/2) = sin theta / (1 + cos theta) turns the reference's
// tan() into quantities already at hand (same value to rounding; FP64 tan costs ~200 instructions on gfx950).
struct LogAux { double d, theta, st, f, c; bool small; };
ESL_HD void so3_log_coeffs(double d, LogAux& a) {
  const bool small = d > 0.99999;   // the reference's small-angle branch
  double theta = 0, st = 0, f = 0.5, c = 1. / 12.;
  if (!small) {   // (locals, not the struct, inside the branch: the struct form was lowered to indexed scratch stores)
    theta = acos(d);
    st = sqrt(1 - d * d);
    const double inv2st = 0.5 / st;
    f = theta * inv2st;
    c = (1 - theta * (1 + d) * inv2st) / (theta * theta);
  }
  a.d = d; a.small = small; a.theta = theta; a.st = st; a.f = f; a.c = c;
}
ESL_HD void vcross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
// log of (R, t) given as a matrix: out = [omega, V^-1 t];  V^-1 t = t - (w x t)/2 + c w x (w x t)
ESL_HD void se3_log_R(const Mat3& R, const double t[3], double out[6], LogAux& a) {
  so3_log_coeffs(0.5 * (R.m[0] + R.m[4] + R.m[8] - 1), a);
  const double w[3] = {a.f * (R.m[7] - R.m[5]), a.f * (R.m[2] - R.m[6]), a.f * (R.m[3] - R.m[1])};
  double wt[3], wwt[3];
  vcross3(w, t, wt);
  vcross3(w, wt, wwt);
  out[0] = w[0]; out[1] = w[1]; out[2] = w[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) out[3 + i] = t[i] - 0.5 * wt[i] + a.c * wwt[i];
}
// SE3Quat::log
ESL_HD void se3_log(const SE3& T, double out[6]) {
  LogAux a;
  se3_log_R(q_to_R(T.r), T.t, out, a);
}

ESL_HD Ell ell_oplus(const Ell& e, const double u[9]) {  // ellipsoid::exp_update
  Ell r;
  r.pose = se3_mul(e.pose, se3_exp(u));
  r.s[0] = e.s[0] + u[6]; r.s[1] = e.s[1] + u[7]; r.s[2] = e.s[2] + u[8];
  return r;
}
ESL_HD SE3 cam_oplus(const SE3& T, const double u[6]) { return se3_mul(se3_exp(u), T); }  // VertexSE3Expmap::oplusImpl

// ------------------------------------------------------------------------------------------------
// bbox edge.  M = K [Rcw|tcw] T_wo  (3x4, columns m0 m1 m2 m3);  C* = sum_k s_k^2 m_k m_k^T - m3 m3^T
// ------------------------------------------------------------------------------------------------
struct BoxGeom {
  double m[4][3];   // columns of M
  double n[4][3];   // columns of N = [Rco | tco] (camera-frame object pose), needed for camera Jacobians
  double C00, C01, C02, C11, C12, C22;
};

ESL_HD void box_geom(const SE3& Tcw, const Ell& e, const double K[4], BoxGeom& g) {
  const Mat3 Rc = q_to_R(Tcw.r);
  const Mat3 Ro = q_to_R(e.pose.r);
  const Mat3 Rco = m3_mul(Rc, Ro);
  double tco[3];
  m3_vec(Rc, e.pose.t, tco);
  tco[0] += Tcw.t[0]; tco[1] += Tcw.t[1]; tco[2] += Tcw.t[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) { g.n[k][0] = Rco.m[k]; g.n[k][1] = Rco.m[3 + k]; g.n[k][2] = Rco.m[6 + k]; }
  g.n[3][0] = tco[0]; g.n[3][1] = tco[1]; g.n[3][2] = tco[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    g.m[k][0] = K[0] * g.n[k][0] + K[2] * g.n[k][2];
    g.m[k][1] = K[1] * g.n[k][1] + K[3] * g.n[k][2];
    g.m[k][2] = g.n[k][2];
  }
  const double d0 = e.s[0] * e.s[0], d1 = e.s[1] * e.s[1], d2 = e.s[2] * e.s[2];
#define ESL_CIJ(i, j) (d0 * g.m[0][i] * g.m[0][j] + d1 * g.m[1][i] * g.m[1][j] + d2 * g.m[2][i] * g.m[2][j] - g.m[3][i] * g.m[3][j])
  g.C00 = ESL_CIJ(0, 0); g.C01 = ESL_CIJ(0, 1); g.C02 = ESL_CIJ(0, 2);
  g.C11 = ESL_CIJ(1, 1); g.C12 = ESL_CIJ(1, 2); g.C22 = ESL_CIJ(2, 2);
#undef ESL_CIJ
}

// bbox (x1,y1,x2,y2) from the dual conic; NaN when the outline is not a real ellipse (C22 >= 0:
// the ellipsoid meets the camera's principal plane / camera inside) — the cases where the
// reference's A^2 / B^2 go negative (Ellipsoid.cpp:240-243).
ESL_HD void box_from_conic(const BoxGeom& g, double bb[4], double sq[2]) {
  const double du = g.C02 * g.C02 - g.C00 * g.C22;
  const double dv = g.C12 * g.C12 - g.C11 * g.C22;
  if (!(g.C22 < 0) || !(du >= 0) || !(dv >= 0)) {
    const double qnan = __builtin_nan("");
    bb[0] = bb[1] = bb[2] = bb[3] = qnan; sq[0] = sq[1] = qnan;
    return;
  }
  const double su = sqrt(du), sv = sqrt(dv);
  const double inv = 1.0 / g.C22;
  bb[0] = (g.C02 + su) * inv; bb[2] = (g.C02 - su) * inv;   // C22 < 0: "+" root is the smaller one
  bb[1] = (g.C12 + sv) * inv; bb[3] = (g.C12 - sv) * inv;
  sq[0] = su; sq[1] = sv;
}

ESL_HD void res_bbox(const SE3& Tcw, const Ell& e, const double K[4], const double meas[4], double r[4]) {
  BoxGeom g;
  box_geom(Tcw, e, K, g);
  double bb[4], sq[2];
  box_from_conic(g, bb, sq);
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = (meas[i] >= 5) ? bb[i] - meas[i] : 0.0;
}

// derivative of the 4 bbox coordinates given (dC00, dC02, dC22, dC11, dC12)
// sq[2], sq[3] carry 1/(2 sqrt(du)), 1/(2 sqrt(dv)); sq[4] = 1/C22 (hoisted: this runs 9-15 times per edge)
ESL_HD void box_dcoords(const BoxGeom& g, const double bb[4], const double sq[5], double dC00, double dC02,
                        double dC22, double dC11, double dC12, double out[4]) {
  const double inv = sq[4];
  const double ddu = (2 * g.C02 * dC02 - dC00 * g.C22 - g.C00 * dC22) * sq[2];
  const double ddv = (2 * g.C12 * dC12 - dC11 * g.C22 - g.C11 * dC22) * sq[3];
  out[0] = (dC02 + ddu - bb[0] * dC22) * inv;
  out[2] = (dC02 - ddu - bb[2] * dC22) * inv;
  out[1] = (dC12 + ddv - bb[1] * dC22) * inv;
  out[3] = (dC12 - ddv - bb[3] * dC22) * inv;
}

// Analytic Jacobians of the bbox residual.  Jo: 4x9 row-major wrt the ellipsoid retraction
// (pose * exp([w,v]), s + ds); Jc: 4x6 wrt the camera retraction exp([w,v]) * Tcw (may be null).
// (template flags instead of null-pointer tests: a pointer comparison on Jo/Jc keeps the arrays from being
// promoted to registers — the kernel then streams its Jacobian through scratch, i.e. through HBM)
template <bool WITH_JO, bool WITH_JC>
ESL_HD void jac_bbox_t(const SE3& Tcw, const Ell& e, const double K[4], const double meas[4], double r[4],
                       double* Jo, double* Jc) {
  BoxGeom g;
  box_geom(Tcw, e, K, g);
  double bb[4], sq[5];
  box_from_conic(g, bb, sq);
  sq[2] = 1.0 / (2 * sq[0]); sq[3] = 1.0 / (2 * sq[1]); sq[4] = 1.0 / g.C22;
  bool mask[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { mask[i] = meas[i] >= 5; r[i] = mask[i] ? bb[i] - meas[i] : 0.0; }
  const double d[3] = {e.s[0] * e.s[0], e.s[1] * e.s[1], e.s[2] * e.s[2]};
  double col[4];
  (void)Jo; (void)Jc;
  // symmetric outer-sum helper: entries (0,0),(0,2),(2,2),(1,1),(1,2) of a b^T + b a^T
#define ESL_SYM5(a, b, f, o00, o02, o22, o11, o12)                                    \
  o00 = (f) * 2 * a[0] * b[0]; o02 = (f) * (a[0] * b[2] + a[2] * b[0]); o22 = (f) * 2 * a[2] * b[2]; \
  o11 = (f) * 2 * a[1] * b[1]; o12 = (f) * (a[1] * b[2] + a[2] * b[1]);
  if constexpr (WITH_JO) {
    double c00, c02, c22, c11, c12;
    // rotations: dC/dwx = (d1-d2)(m1 m2^T + m2 m1^T), dwy = (d2-d0)(m0 m2^T+..), dwz = (d0-d1)(m0 m1^T+..)
    ESL_SYM5(g.m[1], g.m[2], (d[1] - d[2]), c00, c02, c22, c11, c12)
    box_dcoords(g, bb, sq, c00, c02, c22, c11, c12, col);
#pragma unroll
    for (int i = 0; i < 4; ++i) Jo[i * 9 + 0] = mask[i] ? col[i] : 0.0;
    ESL_SYM5(g.m[0], g.m[2], (d[2] - d[0]), c00, c02, c22, c11, c12)
    box_dcoords(g, bb, sq, c00, c02, c22, c11, c12, col);
#pragma unroll
    for (int i = 0; i < 4; ++i) Jo[i * 9 + 1] = mask[i] ? col[i] : 0.0;
    ESL_SYM5(g.m[0], g.m[1], (d[0] - d[1]), c00, c02, c22, c11, c12)
    box_dcoords(g, bb, sq, c00, c02, c22, c11, c12, col);
#pragma unroll
    for (int i = 0; i < 4; ++i) Jo[i * 9 + 2] = mask[i] ? col[i] : 0.0;
    // translations: dC/dv_j = -(m_j m3^T + m3 m_j^T)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      ESL_SYM5(g.m[j], g.m[3], -1.0, c00, c02, c22, c11, c12)
      box_dcoords(g, bb, sq, c00, c02, c22, c11, c12, col);
#pragma unroll
      for (int i = 0; i < 4; ++i) Jo[i * 9 + 3 + j] = mask[i] ? col[i] : 0.0;
    }
    // scales: dC/ds_k = 2 s_k m_k m_k^T
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double f = 2 * e.s[k];
      c00 = f * g.m[k][0] * g.m[k][0]; c02 = f * g.m[k][0] * g.m[k][2]; c22 = f * g.m[k][2] * g.m[k][2];
      c11 = f * g.m[k][1] * g.m[k][1]; c12 = f * g.m[k][1] * g.m[k][2];
      box_dcoords(g, bb, sq, c00, c02, c22, c11, c12, col);
#pragma unroll
      for (int i = 0; i < 4; ++i) Jo[i * 9 + 6 + k] = mask[i] ? col[i] : 0.0;
    }
  }
  if constexpr (WITH_JC) {
    // B = N D M^T (3x3): B[a][b] = sum_k d_k n_k[a] m_k[b] - n3[a] m3[b]
    double B[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        B[a][b] = d[0] * g.n[0][a] * g.m[0][b] + d[1] * g.n[1][a] * g.m[1][b] + d[2] * g.n[2][a] * g.m[2][b] - g.n[3][a] * g.m[3][b];
    // dC = X + X^T, X = K [e_j]x B.  rows of [e_j]x B: (e_j x B_col) per column
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double Y[3][3];  // [e_j]x B
      const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
#pragma unroll
      for (int b = 0; b < 3; ++b) { Y[j][b] = 0; Y[j1][b] = -B[j2][b]; Y[j2][b] = B[j1][b]; }
      double X[3][3];
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        X[0][b] = K[0] * Y[0][b] + K[2] * Y[2][b];
        X[1][b] = K[1] * Y[1][b] + K[3] * Y[2][b];
        X[2][b] = Y[2][b];
      }
      box_dcoords(g, bb, sq, 2 * X[0][0], X[0][2] + X[2][0], 2 * X[2][2], 2 * X[1][1], X[1][2] + X[2][1], col);
#pragma unroll
      for (int i = 0; i < 4; ++i) Jc[i * 6 + j] = mask[i] ? col[i] : 0.0;
    }
    // translation of the camera: dM = K e_j e4^T -> X = -(K e_j) m3^T
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double ke[3] = {0, 0, 0};
      if (j == 0) { ke[0] = K[0]; }
      else if (j == 1) { ke[1] = K[1]; }
      else { ke[0] = K[2]; ke[1] = K[3]; ke[2] = 1.0; }
      double c00, c02, c22, c11, c12;
      ESL_SYM5(ke, g.m[3], -1.0, c00, c02, c22, c11, c12)
      box_dcoords(g, bb, sq, c00, c02, c22, c11, c12, col);
#pragma unroll
      for (int i = 0; i < 4; ++i) Jc[i * 6 + 3 + j] = mask[i] ? col[i] : 0.0;
    }
  }
#undef ESL_SYM5
}

// checkVisibility (src/core/Optimizer.cpp:35-81): ellipsoid centre in front of the camera, camera centre outside the
// ellipsoid, and the projected centre -- or the top-left / bottom-right corner of the projected box -- inside the image
ESL_HD bool bbox_edge_visible(const SE3& Tcw, const Ell& e, const double K[4], int rows, int cols) {
  const Mat3 Rc = q_to_R(Tcw.r);
  double pc[3];
  m3_vec(Rc, e.pose.t, pc);
  pc[0] += Tcw.t[0]; pc[1] += Tcw.t[1]; pc[2] += Tcw.t[2];
  if (pc[2] < 0) return false;
  // camera centre in the world: -Rc^T tc; in the object frame: Ro^T (X - to)
  double xw[3], d[3], xo[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) xw[k] = -(Rc.m[k] * Tcw.t[0] + Rc.m[3 + k] * Tcw.t[1] + Rc.m[6 + k] * Tcw.t[2]);
  const Mat3 Ro = q_to_R(e.pose.r);
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = xw[k] - e.pose.t[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) xo[k] = (Ro.m[k] * d[0] + Ro.m[3 + k] * d[1] + Ro.m[6 + k] * d[2]) / e.s[k];
  if (xo[0] * xo[0] + xo[1] * xo[1] + xo[2] * xo[2] - 1.0 < 0) return false;
  const double u = (K[0] * pc[0] + K[2] * pc[2]) / pc[2], v = (K[1] * pc[1] + K[3] * pc[2]) / pc[2];
  if (u > 0 && u < cols && v > 0 && v < rows) return true;
  BoxGeom g;
  box_geom(Tcw, e, K, g);
  double bb[4], sq[2];
  box_from_conic(g, bb, sq);
  if (bb[0] > 0 && bb[0] < cols && bb[1] > 0 && bb[1] < rows) return true;
  if (bb[2] > 0 && bb[2] < cols && bb[3] > 0 && bb[3] < rows) return true;
  return false;
}

// ------------------------------------------------------------------------------------------------
// Plane-tangency residual (esl_lm_params::bbox_residual = ESL_BBOX_TANGENCY; NOT a reference edge type: the reference
// uses the constraint pi^T Q* pi = 0 only in its SVD initialiser, src/core/Initializer.cpp:147-164, 271-284).
// Row k of a bbox observation is the plane through the camera centre and the image line l_k (l_0: x = x1, l_1: y = y1,
// l_2: x = x2, l_3: y = y2; Initializer.cpp:115-142), pi = P^T l with the normal scaled to unit length; the residual is
// pi^T Q* pi, evaluated in the camera frame:  r_k = sum_j s_j^2 (Rco_j . n)^2 - (tco . n)^2  (m^2; 0 = tangent).
// Entries whose measurement is < 5 are skipped like in the reprojection residual (BasicEllipsoidEdges.cpp:109).
// ------------------------------------------------------------------------------------------------
ESL_HD void tangency_normal(const double K[4], const double meas[4], int k, double n[3]) {
  // K^T l_k : l = (1, 0, -x) for k even, (0, 1, -y) for k odd
  if ((k & 1) == 0) { n[0] = K[0]; n[1] = 0; n[2] = K[2] - meas[k]; }
  else { n[0] = 0; n[1] = K[1]; n[2] = K[3] - meas[k]; }
  const double inv = 1.0 / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  n[0] *= inv; n[1] *= inv; n[2] *= inv;
}
template <bool WITH_JO, bool WITH_JC>
ESL_HD void jac_tangency_t(const SE3& Tcw, const Ell& e, const double K[4], const double meas[4], double r[4], double* Jo, double* Jc) {
  BoxGeom g;
  box_geom(Tcw, e, K, g);   // g.n[j] = column j of R_co (j < 3), g.n[3] = t_co
  (void)Jo; (void)Jc;
  const double d[3] = {e.s[0] * e.s[0], e.s[1] * e.s[1], e.s[2] * e.s[2]};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool on = meas[k] >= 5;
    double n[3];
    tangency_normal(K, meas, k, n);
    double m[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) m[j] = g.n[j][0] * n[0] + g.n[j][1] * n[1] + g.n[j][2] * n[2];
    const double q = g.n[3][0] * n[0] + g.n[3][1] * n[1] + g.n[3][2] * n[2];
    r[k] = on ? d[0] * m[0] * m[0] + d[1] * m[1] * m[1] + d[2] * m[2] * m[2] - q * q : 0.0;
    if constexpr (WITH_JO) {   // pose * exp([w, v]), s + ds
      double* J = Jo + 9 * k;
      J[0] = on ? 2 * m[1] * m[2] * (d[1] - d[2]) : 0.0;
      J[1] = on ? 2 * m[0] * m[2] * (d[2] - d[0]) : 0.0;
      J[2] = on ? 2 * m[0] * m[1] * (d[0] - d[1]) : 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) { J[3 + j] = on ? -2 * q * m[j] : 0.0; J[6 + j] = on ? 2 * e.s[j] * m[j] * m[j] : 0.0; }
    }
    if constexpr (WITH_JC) {   // exp([w, v]) * Tcw
      double* J = Jc + 6 * k;
      double a[3] = {0, 0, 0};
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double f = 2 * d[j] * m[j];
        a[0] += f * (g.n[j][1] * n[2] - g.n[j][2] * n[1]);
        a[1] += f * (g.n[j][2] * n[0] - g.n[j][0] * n[2]);
        a[2] += f * (g.n[j][0] * n[1] - g.n[j][1] * n[0]);
      }
      a[0] -= 2 * q * (g.n[3][1] * n[2] - g.n[3][2] * n[1]);
      a[1] -= 2 * q * (g.n[3][2] * n[0] - g.n[3][0] * n[2]);
      a[2] -= 2 * q * (g.n[3][0] * n[1] - g.n[3][1] * n[0]);
#pragma unroll
      for (int j = 0; j < 3; ++j) { J[j] = on ? a[j] : 0.0; J[3 + j] = on ? -2 * q * n[j] : 0.0; }
    }
  }
}
ESL_HD void res_tangency(const SE3& Tcw, const Ell& e, const double K[4], const double meas[4], double r[4]) {
  jac_tangency_t<false, false>(Tcw, e, K, meas, r, nullptr, nullptr);
}
// the residual of a bbox observation in the mode the run asks for (0 = reprojection, the reference's edge; 1 = tangency)
ESL_HD void res_box_edge(int mode, const SE3& Tcw, const Ell& e, const double K[4], const double meas[4], double r[4]) {
  if (mode) res_tangency(Tcw, e, K, meas, r);
  else res_bbox(Tcw, e, K, meas, r);
}

// runtime-pointer front end (either Jacobian may be null)
ESL_HD void jac_bbox(const SE3& Tcw, const Ell& e, const double K[4], const double meas[4], double r[4],
                     double* Jo, double* Jc) {
  if (Jo && Jc) jac_bbox_t<true, true>(Tcw, e, K, meas, r, Jo, Jc);
  else if (Jo) jac_bbox_t<true, false>(Tcw, e, K, meas, r, Jo, nullptr);
  else if (Jc) jac_bbox_t<false, true>(Tcw, e, K, meas, r, nullptr, Jc);
  else res_bbox(Tcw, e, K, meas, r);
}
// both Jacobians, no null tests on the arrays (`if (Jo && Jc)` on two private arrays is not folded by the compiler -- null is a valid
// private address -- and an array whose address is compared stays in scratch memory: 496 B per lane in k_slam_linearize_chunks, round 6)
ESL_HD void jac_box_edge_both(int mode, const SE3& Tcw, const Ell& e, const double K[4], const double meas[4], double r[4], double* Jo, double* Jc) {
  if (!mode) jac_bbox_t<true, true>(Tcw, e, K, meas, r, Jo, Jc);
  else jac_tangency_t<true, true>(Tcw, e, K, meas, r, Jo, Jc);
}
ESL_HD void jac_box_edge(int mode, const SE3& Tcw, const Ell& e, const double K[4], const double meas[4], double r[4], double* Jo, double* Jc) {
  if (!mode) { jac_bbox(Tcw, e, K, meas, r, Jo, Jc); return; }
  if (Jo && Jc) jac_tangency_t<true, true>(Tcw, e, K, meas, r, Jo, Jc);
  else if (Jo) jac_tangency_t<true, false>(Tcw, e, K, meas, r, Jo, nullptr);
  else if (Jc) jac_tangency_t<false, true>(Tcw, e, K, meas, r, nullptr, Jc);
  else res_tangency(Tcw, e, K, meas, r);
}

// ------------------------------------------------------------------------------------------------
// 9-DoF 3-D edge
// ------------------------------------------------------------------------------------------------
// sin/cos of yaw/2 for yaw = k*pi/2, k = -1,0,1,2, and the entries of the yaw rotation matrix Rz built from the
// NORMALISED quaternion (0,0,s,c) exactly as q_to_R would: cy = 1 - 2 z^2, sy = 2 z w.  Filled once on the host.
struct YawTable { double s[4], c[4], cy[4], sy[4]; int as_written; /* esl_lm_params::e3d_half_turn of the current run */ };
ESL_HD void yaw_table_fill(YawTable& yt, const double half_sin[4], const double half_cos[4]) {
  yt.as_written = 0;
  for (int k = 0; k < 4; ++k) {
    const Quat q = q_normalize_pos(Quat{0, 0, half_sin[k], half_cos[k]});
    yt.s[k] = half_sin[k]; yt.c[k] = half_cos[k];
    yt.cy[k] = 1 - 2 * q.z * q.z;
    yt.sy[k] = 2 * q.z * q.w;
  }
}

// Relative pose of one yaw hypothesis:  E_k = (T_wc T_meas Rz_k)^-1 T_est = Rz_k^T E_0  with  E_0 = (T_wc T_meas)^-1 T_est
// (EdgeSE3EllipsoidProj-free 3-D edge, Edge.cpp: the measured ellipsoid is tried at 4 yaws and the smallest
// 9-norm of the error wins).  The reference multiplies everything out per hypothesis; E_0 is shared here and the
// hypothesis only mixes its first two rows / translation components.
struct E3dHyp { Mat3 R; double t[3]; LogAux a; };
ESL_HD void e3d_hypothesis(const Mat3& R0, const double t0[3], double cy, double sy, E3dHyp& h) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    h.R.m[c] = cy * R0.m[c] + sy * R0.m[3 + c];
    h.R.m[3 + c] = cy * R0.m[3 + c] - sy * R0.m[c];
    h.R.m[6 + c] = R0.m[6 + c];
  }
  h.t[0] = cy * t0[0] + sy * t0[1];
  h.t[1] = cy * t0[1] - sy * t0[0];
  h.t[2] = t0[2];
}

// residual of the 3-D edge; `best` (optional) receives the chosen hypothesis' relative pose and log coefficients
// hypothesis-independent part of the 3-D edge: E_0 = (T_wc T_meas)^-1 T_est
ESL_HD SE3 e3d_E0(const SE3& Tcw, const Ell& est, const Ell& meas) {
  const SE3 Twc = se3_inv(Tcw);
  const SE3 mw = se3_mul(Twc, meas.pose);
  return se3_mul(se3_inv(mw), est.pose);
}
ESL_HD void res_e3d_from_E0(const SE3& E0, const double est_s[3], const double meas_s[3], const YawTable& yt, double r[9],
                            E3dHyp* best_out = nullptr);
ESL_HD void res_e3d(const SE3& Tcw, const Ell& est, const Ell& meas, const YawTable& yt, double r[9], E3dHyp* best_out = nullptr) {
  res_e3d_from_E0(e3d_E0(Tcw, est, meas), est.s, meas.s, yt, r, best_out);
}
ESL_HD void res_e3d_from_E0(const SE3& E0, const double est_s[3], const double meas_s[3], const YawTable& yt, double r[9],
                            E3dHyp* best_out) {
  const Mat3 R0 = q_to_R(E0.r);
  // (round 5) the half-turn exclusion below must leave something to take: when E_0 itself is a half turn about a
  // HORIZONTAL axis (the estimate upside-down relative to the measurement) every Rz_k^T E_0 is one too -- then all four stay
  // eligible and the first minimum as written wins, which is what the reference and the checker compute there
  bool all_half = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double tr = (yt.cy[k] * R0.m[0] + yt.sy[k] * R0.m[3]) + (yt.cy[k] * R0.m[4] - yt.sy[k] * R0.m[1]) + R0.m[8];
    all_half = all_half && !(0.5 * (tr - 1.0) > -1.0 + 1e-12);
  }
  double best = 0, b_cy = 1, b_sy = 0;
  LogAux b_a;
  b_a.d = 1; b_a.theta = 0; b_a.st = 0; b_a.f = 0.5; b_a.c = 1. / 12.; b_a.small = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    E3dHyp h;
    e3d_hypothesis(R0, E0.t, yt.cy[k], yt.sy[k], h);
    double e[9];
    se3_log_R(h.R, h.t, e, h.a);
    const bool swap = (k == 0 || k == 2);  // yaw = -90 or +90 degrees: a/b swapped
    e[6] = est_s[0] - (swap ? meas_s[1] : meas_s[0]);
    e[7] = est_s[1] - (swap ? meas_s[0] : meas_s[1]);
    e[8] = est_s[2] - meas_s[2];
    double n2 = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) n2 += e[i] * e[i];
    // A hypothesis within ~1.4e-6 rad of a HALF TURN is not eligible (round 4).  The reference's log has no branch for theta -> pi
    // (se3quat.h:229-266): omega = theta / (2 sqrt(1 - d^2)) vee(R - R^T) with d = cos(theta) rounded to the nearest double is
    // pi delta / sqrt(1 - d^2) in size at theta = pi - delta -- anything between 0 and inf for delta below 1e-8, decided by the last
    // bit of the trace.  The configuration is reached in practice: an ellipsoid held by ONE 3-D edge and the gravity prior converges
    // to the measurement's yaw exactly and keeps a tilt residual eps, and Rz(pi) R_tilt(eps) is a half turn for ANY eps.  Its true
    // norm is pi (never the minimum over the four yaws); measured on the streaming sequence, frame 11: this code took it at 7e-13
    // where the checker's (and the numpy restatement's) arithmetic lands on the other side and keeps the true minimum 1.88e-2.
    const double nn = (yt.as_written || all_half || h.a.d > -1.0 + 1e-12) ? sqrt(n2) : 1.7976931348623157e308;   // (as_written: esl_lm_params::e3d_half_turn = 1, the reference's minCoeff)
    const bool take = (k == 0) || (nn < best);
    best = take ? nn : best;
#pragma unroll
    for (int i = 0; i < 9; ++i) r[i] = take ? e[i] : r[i];
    // remember the winner by its scalars only (a conditional copy of the whole hypothesis went through scratch)
    b_cy = take ? yt.cy[k] : b_cy; b_sy = take ? yt.sy[k] : b_sy;
    b_a.d = take ? h.a.d : b_a.d; b_a.theta = take ? h.a.theta : b_a.theta; b_a.st = take ? h.a.st : b_a.st;
    b_a.f = take ? h.a.f : b_a.f; b_a.c = take ? h.a.c : b_a.c; b_a.small = take ? h.a.small : b_a.small;
  }
  if (best_out) {
    e3d_hypothesis(R0, E0.t, b_cy, b_sy, *best_out);
    best_out->a = b_a;
  }
}

// d log(E exp(delta)) / d delta at 0 (6x6, row-major; rows/cols ordered [omega, upsilon]) for E = (R, t) whose log
// coefficients `a` are already known (so3_log_coeffs of the same R)
ESL_HD void dlog_right_R(const Mat3& R, const double t[3], const LogAux& a, double J[36]) {
  const double dRv[3] = {R.m[7] - R.m[5], R.m[2] - R.m[6], R.m[3] - R.m[1]};
  const double f = a.f, c = a.c, theta = a.theta;
  double fp = 0.0, cp = 0.0, inv_theta = 0.0;
  if (!a.small) {
    const double st = a.st, ct = a.d;
    const double inv_st = 1.0 / st;
    inv_theta = 1.0 / theta;
    // f(d) = theta/(2 sin theta), d theta/dd = -1/sin theta
    fp = -(st - theta * ct) * (0.5 * inv_st * inv_st * inv_st);
    // g = theta / (2 tan(theta/2)), 1/tan(theta/2) = (1 + cos theta) / sin theta
    const double it = (1 + ct) * inv_st;
    const double g = 0.5 * theta * it;
    const double gp = 0.5 * it - 0.25 * theta * (it * it + 1);
    const double ith2 = inv_theta * inv_theta;
    cp = (-gp) * ith2 - 2 * (1 - g) * (ith2 * inv_theta);
  }
  const double w[3] = {f * dRv[0], f * dRv[1], f * dRv[2]};
  double wt[3], wwt[3];
  vcross3(w, t, wt);
  vcross3(w, wt, wwt);
  // rotation directions: dR = R [e_j]x
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    // columns of R [e_j]x : col j = 0, col j1 = R col j2, col j2 = -R col j1   ([e_j]x e_j1 = e_j2, [e_j]x e_j2 = -e_j1)
    Mat3 dRm;
#pragma unroll
    for (int q = 0; q < 3; ++q) { dRm.m[q * 3 + j] = 0; dRm.m[q * 3 + j1] = R.m[q * 3 + j2]; dRm.m[q * 3 + j2] = -R.m[q * 3 + j1]; }
    const double dd = 0.5 * (dRm.m[0] + dRm.m[4] + dRm.m[8]);
    const double ddR[3] = {dRm.m[7] - dRm.m[5], dRm.m[2] - dRm.m[6], dRm.m[3] - dRm.m[1]};
    double dw[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) dw[q] = fp * dd * dRv[q] + f * ddR[q];
    // d upsilon = dVinv t,  dVinv = -dOm/2 + cp dtheta Om^2 + c (dOm Om + Om dOm)   -- as cross products
    const double dtheta = a.small ? 0.0 : (w[0] * dw[0] + w[1] * dw[1] + w[2] * dw[2]) * inv_theta;
    double dwt[3], dw_wt[3], w_dwt[3];
    vcross3(dw, t, dwt);
    vcross3(dw, wt, dw_wt);
    vcross3(w, dwt, w_dwt);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      J[q * 6 + j] = dw[q];
      J[(3 + q) * 6 + j] = -0.5 * dwt[q] + (cp * dtheta) * wwt[q] + c * (dw_wt[q] + w_dwt[q]);
    }
  }
  // translation directions: dt = R e_j -> d upsilon = Vinv R e_j ; d omega = 0
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double col[3] = {R.m[j], R.m[3 + j], R.m[6 + j]};
    double wc[3], wwc[3];
    vcross3(w, col, wc);
    vcross3(w, wc, wwc);
#pragma unroll
    for (int q = 0; q < 3; ++q) { J[q * 6 + 3 + j] = 0.0; J[(3 + q) * 6 + 3 + j] = col[q] - 0.5 * wc[q] + c * wwc[q]; }
  }
}
ESL_HD void dlog_right(const SE3& E, double J[36]) {
  const Mat3 R = q_to_R(E.r);
  LogAux a;
  so3_log_coeffs(0.5 * (R.m[0] + R.m[4] + R.m[8] - 1), a);
  dlog_right_R(R, E.t, a, J);
}

// Ad(T) for twists ordered [omega, upsilon]  (SE3Quat::adj, se3quat.h:324-333)
ESL_HD void se3_adj(const SE3& T, double A[36]) {
  const Mat3 R = q_to_R(T.r);
  const Mat3 tR = m3_mul(skew(T.t), R);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      A[a * 6 + b] = R.m[a * 3 + b];
      A[a * 6 + 3 + b] = 0.0;
      A[(3 + a) * 6 + b] = tR.m[a * 3 + b];
      A[(3 + a) * 6 + 3 + b] = R.m[a * 3 + b];
    }
}

// The 3-D edge's Jacobian wrt the ellipsoid is [[Jp (6x6), 0], [0, I3]]: the scale rows are s - s_k.  Jp only:
ESL_HD void jac_e3d_pose(const SE3& Tcw, const Ell& est, const Ell& meas, const YawTable& yt, double r[9], double Jp[36]) {
  E3dHyp h;
  res_e3d(Tcw, est, meas, yt, r, &h);
  dlog_right_R(h.R, h.t, h.a, Jp);
}

// Analytic Jacobians of the 3-D edge.  Jo 9x9, Jc 9x6 (may be null).
ESL_HD void jac_e3d(const SE3& Tcw, const Ell& est, const Ell& meas, const YawTable& yt, double r[9],
                    double* Jo, double* Jc) {
  E3dHyp h;
  res_e3d(Tcw, est, meas, yt, r, &h);
  double Jp[36];
  dlog_right_R(h.R, h.t, h.a, Jp);
  if (Jo) {
#pragma unroll
    for (int a = 0; a < 9; ++a)
#pragma unroll
      for (int b = 0; b < 9; ++b) Jo[a * 9 + b] = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) Jo[a * 9 + b] = Jp[a * 6 + b];
    Jo[6 * 9 + 6] = 1.0; Jo[7 * 9 + 7] = 1.0; Jo[8 * 9 + 8] = 1.0;
  }
  if (Jc) {
    // exp(d) Tcw  ==  right perturbation of E by Ad((Tcw T_est)^-1) d
    const SE3 Tco = se3_mul(Tcw, est.pose);
    double Ad[36];
    se3_adj(se3_inv(Tco), Ad);
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += Jp[a * 6 + k] * Ad[k * 6 + b];
        Jc[a * 6 + b] = s;
      }
#pragma unroll
    for (int a = 6; a < 9; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) Jc[a * 6 + b] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------------
// gravity prior
// ------------------------------------------------------------------------------------------------
ESL_HD double res_grav(const Ell& e, const double nrm[3]) {
  const Mat3 R = q_to_R(e.pose.r);
  const double z[3] = {R.m[2], R.m[5], R.m[8]};
  const double dot = z[0] * nrm[0] + z[1] * nrm[1] + z[2] * nrm[2];
  const double zn = sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
  const double nn = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
  double c = dot / zn / nn;
  if (c > 1) c = c - 0.0001;
  else if (c < -1) c = c + 0.0001;
  return acos(c);
}
ESL_HD double jac_grav(const Ell& e, const double nrm[3], double Jo[9]) {
  const Mat3 R = q_to_R(e.pose.r);
  const double nn = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
  const double n[3] = {nrm[0] / nn, nrm[1] / nn, nrm[2] / nn};
  const double zn = sqrt(R.m[2] * R.m[2] + R.m[5] * R.m[5] + R.m[8] * R.m[8]);
  double c = (R.m[2] * n[0] + R.m[5] * n[1] + R.m[8] * n[2]) / zn;
  const double c0 = (R.m[0] * n[0] + R.m[3] * n[1] + R.m[6] * n[2]) / zn;  // x-axis . n
  const double c1 = (R.m[1] * n[0] + R.m[4] * n[1] + R.m[7] * n[2]) / zn;  // y-axis . n
  if (c > 1) c = c - 0.0001;
  else if (c < -1) c = c + 0.0001;
  const double s2 = 1 - c * c;
#pragma unroll
  for (int i = 0; i < 9; ++i) Jo[i] = 0.0;
  if (s2 > 1e-24) {
    const double is = 1.0 / sqrt(s2);
    // z' = z + wy * x_axis - wx * y_axis  ->  dc/dwx = -c1, dc/dwy = c0 ; d acos = -dc / sin
    Jo[0] = c1 * is;
    Jo[1] = -c0 * is;
  }
  return acos(c);
}

// ------------------------------------------------------------------------------------------------
// odometry  r = log(Z Ti Tj^-1)
// ------------------------------------------------------------------------------------------------
ESL_HD void res_odom(const SE3& Ti, const SE3& Tj, const SE3& Z, double r[6], SE3* E_out = nullptr) {
  const SE3 E = se3_mul(se3_mul(Z, Ti), se3_inv(Tj));
  se3_log(E, r);
  if (E_out) *E_out = E;
}
ESL_HD void jac_odom(const SE3& Ti, const SE3& Tj, const SE3& Z, double r[6], double* Ji, double* Jj) {
  SE3 E;
  res_odom(Ti, Tj, Z, r, &E);
  double Jp[36];
  dlog_right(E, Jp);
  if (Jj) {
#pragma unroll
    for (int i = 0; i < 36; ++i) Jj[i] = -Jp[i];
  }
  if (Ji) {
    double Ad[36];
    se3_adj(se3_mul(Tj, se3_inv(Ti)), Ad);
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += Jp[a * 6 + k] * Ad[k * 6 + b];
        Ji[a * 6 + b] = s;
      }
  }
}

// ------------------------------------------------------------------------------------------------
// small SPD solve: (H + lambda I) x = b for one 9x9 (or dxd) block, Cholesky-free LDL^T without
// pivoting; returns false on a non-positive pivot.  H is the packed upper triangle, row-major.
// ------------------------------------------------------------------------------------------------
template <int D>
ESL_HD bool ldlt_solve_packed(const double* Hp, double lambda, const double* b, double* x) {
  double L[D * D];
  // unpack
  int p = 0;
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = i; j < D; ++j) { const double v = Hp[p++]; L[i * D + j] = v; L[j * D + i] = v; }
#pragma unroll
  for (int i = 0; i < D; ++i) L[i * D + i] += lambda;
  bool ok = true;
  double dinv[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    double dk = L[k * D + k];
#pragma unroll
    for (int j = 0; j < k; ++j) dk -= L[k * D + j] * L[k * D + j] * L[j * D + j];
    L[k * D + k] = dk;
    if (!(dk > 0)) ok = false;
    dinv[k] = 1.0 / dk;
#pragma unroll
    for (int i = k + 1; i < D; ++i) {
      double v = L[i * D + k];
#pragma unroll
      for (int j = 0; j < k; ++j) v -= L[i * D + j] * L[k * D + j] * L[j * D + j];
      L[i * D + k] = v * dinv[k];
    }
  }
  double y[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double s = b[i];
#pragma unroll
    for (int j = 0; j < i; ++j) s -= L[i * D + j] * y[j];
    y[i] = s;
  }
#pragma unroll
  for (int i = 0; i < D; ++i) y[i] *= dinv[i];
#pragma unroll
  for (int i = D - 1; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int j = i + 1; j < D; ++j) s -= L[j * D + i] * x[j];
    x[i] = s;
  }
  return ok;
}

// g2o's robust kernels (core/robust_kernel_impl.cpp), rho0 = rho(e) and rho1 = rho'(e) of the squared error e for the
// esl_robust_kind `kind` with width delta; e <= delta^2 is the inlier test.  The rho2 term is not needed (g2o leaves it out of
// robustInformation).  g2o's Tukey keeps delta^2 and its reciprocal in float members; here they are double.
__host__ __device__ __forceinline__ void robustify(int kind, double delta, double e, double& rho0, double& rho1) {
  const double dsqr = delta * delta;
  if (kind == 1) {          // Huber
    if (e <= dsqr) { rho0 = e; rho1 = 1.; }
    else { const double sqrte = sqrt(e); rho0 = 2 * sqrte * delta - dsqr; rho1 = delta / sqrte; }
  } else if (kind == 2) {   // PseudoHuber
    const double aux2 = sqrt((1. / dsqr) * e + 1.0);
    rho0 = 2 * dsqr * (aux2 - 1); rho1 = 1. / aux2;
  } else if (kind == 3) {   // Cauchy
    const double aux = (1. / dsqr) * e + 1.0;
    rho0 = dsqr * log(aux); rho1 = 1. / aux;
  } else if (kind == 4) {   // Tukey
    if (e <= dsqr) { const double d = 1 - e * (1. / dsqr), dd = d * d; rho0 = dsqr * (1 - dd * d); rho1 = 3 * dd; }
    else { rho0 = dsqr; rho1 = 0.; }
  } else { rho0 = e; rho1 = 1.; }
}

}  // namespace esl
