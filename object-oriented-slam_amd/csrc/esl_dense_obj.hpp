// esl_dense_obj.hpp — the arithmetic of esl_dense_objects (include/esl.h, "per-instance ellipsoids from the dense map"; the steps'
// numbers below are the header's): the normalised plane, a voxel's centre and height (step 1), the host's choice of a component per
// label and an object's status (steps 3 to 5: dobj_choose, dobj_status), the guard of the moments (step 5), the
// gravity basis and the frame of a component (step 6), the projections and the order-preserving encoding their minima and maxima are
// reduced in (step 7), and the output row (step 8).  Plain C++ for host and device like esl_dense_key.hpp, no HIP include:
// tests/dense_obj_main.cpp compiles it with an ordinary compiler.  Every translation unit that includes it is built with
// -ffp-contract=off.  What is `inline` only runs on the host: one compiler decides every bit of the frame.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "esl_dense_key.hpp"

namespace esl {

constexpr int kDobjMoments = 9;   // s_x s_y s_z, M_xx M_xy M_xz M_yy M_yz M_zz
constexpr int kDobjRow = 8;       // a row of the component table on the device: label, size, samples, root, kx, ky, kz, 0
constexpr long long kDobjGuard = 1ll << 62;

struct DobjPlane { double n[3], d, u[3], v[3]; };   // n^, d^ (step 1); u, v (step 6)

// steps 1 and 6: false for a non-finite plane number or |n| < 1e-12
inline bool dobj_plane(const double g[4], DobjPlane& P) {
  for (int a = 0; a < 4; ++a) if (!std::isfinite(g[a])) return false;
  const double nn = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  if (!std::isfinite(nn) || !(nn >= 1e-12)) return false;
  for (int a = 0; a < 3; ++a) P.n[a] = g[a] / nn;
  P.d = g[3] / nn;
  int k = 0;
  for (int a = 1; a < 3; ++a) if (std::fabs(P.n[a]) < std::fabs(P.n[k])) k = a;
  double e[3] = {0, 0, 0};
  e[k] = 1;
  const double* n = P.n;
  double* u = P.u;
  u[0] = e[1] * n[2] - e[2] * n[1]; u[1] = e[2] * n[0] - e[0] * n[2]; u[2] = e[0] * n[1] - e[1] * n[0];
  const double un = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int a = 0; a < 3; ++a) u[a] /= un;
  P.v[0] = n[1] * u[2] - n[2] * u[1]; P.v[1] = n[2] * u[0] - n[0] * u[2]; P.v[2] = n[0] * u[1] - n[1] * u[0];
  return true;
}

// step 1: the centre of voxel k along one axis; step 7: a projection of a centre; step 1: the height above the ground
ESL_DENSE_HD double dobj_center(int k, double leaf) { return ((double)k + 0.5) * leaf; }
ESL_DENSE_HD double dobj_proj(const double a[3], const double p[3]) { return (a[0] * p[0] + a[1] * p[1]) + a[2] * p[2]; }
ESL_DENSE_HD double dobj_height(const double n[3], double d, const double x[3]) { return dobj_proj(n, x) + d; }

// step 5: n span^2 >= 2^62, in integers without overflowing (n >= 1, 1 <= span <= 2^31)
ESL_DENSE_HD bool dobj_guard(long long n, long long span) {
  const long long s2 = span * span;          // < 2^62
  return n > (kDobjGuard - 1) / s2;          // n s2 >= 2^62  <=>  n > floor((2^62 - 1) / s2)
}

// an order-preserving map of the doubles (no NaN) onto the unsigned 64-bit integers, and back
ESL_DENSE_HD unsigned long long dobj_enc(double v) {
  union { double d; unsigned long long u; } b;
  b.d = v;
  return (b.u >> 63) ? ~b.u : (b.u | 0x8000000000000000ull);
}
ESL_DENSE_HD double dobj_dec(unsigned long long e) {
  union { double d; unsigned long long u; } b;
  b.u = (e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e;
  return b.d;
}

// Steps 3 and 4 on the host, from the table of the components of min_component voxels or more as the device left it: R rows of
// kDobjRow ints in any order, every label below N.  order: the rows sorted by label, then size descending, then the root's index
// (the order of the packed keys).  Per sorted row its root and the object it is chosen for or -1; per label its chosen sorted row or
// -1 (the first of its rows) and the number of its rows; the first comp_cap sorted rows go to comp_out (6 ints each).
struct DobjChoice { std::vector<int> order, rowroot, rowobj, chosen, nrows; };
inline void dobj_choose(const int* tab, long long R, int N, long long comp_cap, int32_t* comp_out, DobjChoice& c) {
  c.order.resize((size_t)R);
  for (long long r = 0; r < R; ++r) c.order[(size_t)r] = (int)r;
  std::sort(c.order.begin(), c.order.end(), [&](int x, int y) {
    const int* tx = tab + (size_t)x * kDobjRow; const int* ty = tab + (size_t)y * kDobjRow;
    if (tx[0] != ty[0]) return tx[0] < ty[0];
    if (tx[1] != ty[1]) return tx[1] > ty[1];
    return tx[3] < ty[3];
  });
  c.rowroot.assign((size_t)R, 0); c.rowobj.assign((size_t)R, -1); c.chosen.assign((size_t)N, -1); c.nrows.assign((size_t)N, 0);
  for (long long r = 0; r < R; ++r) {
    const int* t = tab + (size_t)c.order[(size_t)r] * kDobjRow;
    c.rowroot[(size_t)r] = t[3];
    ++c.nrows[(size_t)t[0]];
    if (c.chosen[(size_t)t[0]] < 0) { c.chosen[(size_t)t[0]] = (int)r; c.rowobj[(size_t)r] = t[0]; }
    if (r < comp_cap) {
      int32_t* co = comp_out + 6 * r;
      co[0] = t[0]; co[1] = t[1]; co[2] = t[2]; co[3] = t[4]; co[4] = t[5]; co[5] = t[6];
    }
  }
}

// steps 4 and 5: an object's status -- 1: no voxel of its label is kept, 2: no component of min_component voxels, 6: the guard of
// the moments over the chosen component's size and its box kb = kmin, kmax; 0 otherwise
inline int dobj_status(int labkept, int chosen, const int kb[6], long long size) {
  if (labkept == 0) return 1;
  if (chosen < 0) return 2;
  long long span = 1;
  for (int e = 0; e < 3; ++e) span = std::max<long long>(span, (long long)kb[3 + e] - kb[e] + 1);
  return dobj_guard(size, span) ? 6 : 0;
}

// a^T C b of the symmetric C = {c00, c01, c02, c11, c12, c22}: rows summed left to right, then the three rows left to right
inline double dobj_quad(const double a[3], const double C[6], const double b[3]) {
  const double r0 = (C[0] * b[0] + C[1] * b[1]) + C[2] * b[2];
  const double r1 = (C[1] * b[0] + C[3] * b[1]) + C[4] * b[2];
  const double r2 = (C[2] * b[0] + C[4] * b[1]) + C[5] * b[2];
  return (a[0] * r0 + a[1] * r1) + a[2] * r2;
}

// step 6: the axes x, y, n^ (rows of A, three numbers each) of a component of n voxels with the moments mom (kDobjMoments)
inline void dobj_frame(const DobjPlane& P, long long n, const long long mom[kDobjMoments], double A[9]) {
  const double dn = (double)n;
  const double m[3] = {(double)mom[0] / dn, (double)mom[1] / dn, (double)mom[2] / dn};
  const double C[6] = {(double)mom[3] / dn - m[0] * m[0], (double)mom[4] / dn - m[0] * m[1], (double)mom[5] / dn - m[0] * m[2],
                       (double)mom[6] / dn - m[1] * m[1], (double)mom[7] / dn - m[1] * m[2], (double)mom[8] / dn - m[2] * m[2]};
  const double cuu = dobj_quad(P.u, C, P.u), cuv = dobj_quad(P.u, C, P.v), cvv = dobj_quad(P.v, C, P.v);
  const double th = 0.5 * std::atan2(2 * cuv, cuu - cvv);
  const double c = std::cos(th), s = std::sin(th);
  const double* nn = P.n;
  double* x = A; double* y = A + 3;
  for (int a = 0; a < 3; ++a) x[a] = c * P.u[a] + s * P.v[a];
  y[0] = nn[1] * x[2] - nn[2] * x[1]; y[1] = nn[2] * x[0] - nn[0] * x[2]; y[2] = nn[0] * x[1] - nn[1] * x[0];
  for (int a = 0; a < 3; ++a) A[6 + a] = nn[a];
}

// the library's q_from_R (esl_math.hpp: branch on the largest diagonal combination) of the row-major R, negated when w < 0
inline void dobj_quat(const double R[9], double q[4]) {
  double x, y, z, w;
  double t = R[0] + R[4] + R[8];
  if (t > 0) {
    t = std::sqrt(t + 1.0);
    w = 0.5 * t; t = 0.5 / t;
    x = (R[7] - R[5]) * t; y = (R[2] - R[6]) * t; z = (R[3] - R[1]) * t;
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    t = std::sqrt(R[0] - R[4] - R[8] + 1.0);
    x = 0.5 * t; t = 0.5 / t;
    w = (R[7] - R[5]) * t; y = (R[3] + R[1]) * t; z = (R[6] + R[2]) * t;
  } else if (R[4] >= R[8]) {
    t = std::sqrt(R[4] - R[8] - R[0] + 1.0);
    y = 0.5 * t; t = 0.5 / t;
    w = (R[2] - R[6]) * t; z = (R[7] + R[5]) * t; x = (R[1] + R[3]) * t;
  } else {
    t = std::sqrt(R[8] - R[0] - R[4] + 1.0);
    z = 0.5 * t; t = 0.5 / t;
    w = (R[3] - R[1]) * t; x = (R[2] + R[6]) * t; y = (R[5] + R[7]) * t;
  }
  if (w < 0) { x = -x; y = -y; z = -z; w = -w; }
  q[0] = x; q[1] = y; q[2] = z; q[3] = w;
}

// steps 7 and 8: the row (t, q, half-axes) from the axes and the minima / maxima of the members' projections
inline void dobj_row(const double A[9], const double mn[3], const double mx[3], double leaf, double row[10]) {
  double c[3];
  for (int a = 0; a < 3; ++a) {
    c[a] = (mn[a] + mx[a]) / 2;
    row[7 + a] = (mx[a] - mn[a]) / 2 + leaf / 2;
  }
  for (int a = 0; a < 3; ++a) row[a] = (A[a] * c[0] + A[3 + a] * c[1]) + A[6 + a] * c[2];
  const double R[9] = {A[0], A[3], A[6], A[1], A[4], A[7], A[2], A[5], A[8]};   // R = [x y n^]: the axes are its columns
  dobj_quat(R, row + 3);
}

}  // namespace esl
