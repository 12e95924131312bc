// esl_init.hip — esl_init_quadric: quadric from >= 9 bbox tangent planes (SVD null vector), one
// wavefront per object.  Replaces EllipsoidSLAM::Initializer::initializeQuadric
// (reference src/core/Initializer.cpp:24-56) = getPlanesHomo (:58-91), fromDetectionsToLines (:107-145),
// getVectorFromPlanesHomo (:147-164), getQStarFromVectors (:166-184), getEllipsoidFromQStar (:186-248).
//
// The plane rows (<= 4 per observation, 10 monomials each) are staged in LDS; the null vector comes
// from a one-sided (Hestenes) Jacobi SVD whose column dot-products are lane-strided sums finished with
// a butterfly all-reduce; the 4x4 / 3x3 decompositions that follow are a few hundred flops on lane 0.
//
// esl_init_quadrics (second half of the file) is the same arithmetic for every object of an edge list in one call: its own kernel
// beside k_init_quadric, which it leaves as it is.
#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "esl_ctx.hpp"
#include "esl_init_group.hpp"
#include "esl_init_sample.hpp"
#include "esl_kernels_map.hpp"

namespace esl {

__device__ __forceinline__ double wave_allsum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// cyclic Jacobi eigen-solver, symmetric N x N row-major; eigenvalues ascending, eigenvectors in columns,
// each column signed so that its largest-magnitude component is positive
template <int N>
__device__ void sym_eig(const double* Ain, double* w, double* V) {
  double A[N * N];
  for (int i = 0; i < N * N; ++i) A[i] = Ain[i];
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) V[i * N + j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
    for (int p = 0; p < N; ++p)
      for (int q = p + 1; q < N; ++q) off += A[p * N + q] * A[p * N + q];
    if (off < 1e-300) break;
    for (int p = 0; p < N; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p * N + q];
        if (apq == 0.0) continue;
        const double theta = (A[q * N + q] - A[p * N + p]) / (2 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
        const double c = 1 / sqrt(t * t + 1), s = t * c;
        for (int k = 0; k < N; ++k) { const double a = A[k * N + p], b = A[k * N + q]; A[k * N + p] = c * a - s * b; A[k * N + q] = s * a + c * b; }
        for (int k = 0; k < N; ++k) { const double a = A[p * N + k], b = A[q * N + k]; A[p * N + k] = c * a - s * b; A[q * N + k] = s * a + c * b; }
        for (int k = 0; k < N; ++k) { const double a = V[k * N + p], b = V[k * N + q]; V[k * N + p] = c * a - s * b; V[k * N + q] = s * a + c * b; }
      }
  }
  for (int i = 0; i < N; ++i) w[i] = A[i * N + i];
  for (int i = 0; i < N; ++i) {
    int m = i;
    for (int j = i + 1; j < N; ++j)
      if (w[j] < w[m]) m = j;
    if (m != i) {
      const double t = w[i]; w[i] = w[m]; w[m] = t;
      for (int k = 0; k < N; ++k) { const double u = V[k * N + i]; V[k * N + i] = V[k * N + m]; V[k * N + m] = u; }
    }
  }
  for (int j = 0; j < N; ++j) {
    int m = 0;
    for (int k = 1; k < N; ++k)
      if (fabs(V[k * N + j]) > fabs(V[m * N + j])) m = k;
    if (V[m * N + j] < 0)
      for (int k = 0; k < N; ++k) V[k * N + j] = -V[k * N + j];
  }
}

// Gauss-Jordan inverse with partial pivoting; returns the determinant
template <int N>
__device__ double inv_det(const double* Ain, double* inv) {
  double A[N * N], det = 1;
  for (int i = 0; i < N * N; ++i) A[i] = Ain[i];
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) inv[i * N + j] = (i == j) ? 1.0 : 0.0;
  for (int c = 0; c < N; ++c) {
    int p = c;
    for (int r = c + 1; r < N; ++r)
      if (fabs(A[r * N + c]) > fabs(A[p * N + c])) p = r;
    if (p != c) {
      for (int k = 0; k < N; ++k) {
        double t = A[c * N + k]; A[c * N + k] = A[p * N + k]; A[p * N + k] = t;
        t = inv[c * N + k]; inv[c * N + k] = inv[p * N + k]; inv[p * N + k] = t;
      }
      det = -det;
    }
    const double d = A[c * N + c];
    det *= d;
    for (int k = 0; k < N; ++k) { A[c * N + k] /= d; inv[c * N + k] /= d; }
    for (int r = 0; r < N; ++r)
      if (r != c) {
        const double f = A[r * N + c];
        for (int k = 0; k < N; ++k) { A[r * N + k] -= f * A[c * N + k]; inv[r * N + k] -= f * inv[c * N + k]; }
      }
  }
  return det;
}

// mode 0: initializeQuadric; 1: getEllipsoidFromQStar of a given Q* (extra[0..15]); 2: quadricErrorWithPlanes of a given
// ellipsoid (extra[0..9]).  a_glob != null: the plane matrix lives in global memory (more observations than LDS holds).
struct InitArgs { double K[4]; int n, rows, cols, faithful, mode; double extra[16]; double* a_glob; };

__device__ void decompose_qstar(const double* Qs, int faithful, double* __restrict__ out);

// out: [0..9] ellipsoid 10-vector, [10..25] Q* row-major, [26] ok, [27] plane error (mode 2)
static __global__ __launch_bounds__(64) void k_init_quadric(const double* __restrict__ poses, const double* __restrict__ boxes,
                                                            InitArgs a, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* V = sm;                                   // 10 x 10
  double* A = a.a_glob ? a.a_glob : sm + 100;       // m x 10
  const int lane = threadIdx.x;
  if (a.mode == 1) {
    if (lane == 0) {
      for (int i = 0; i < 16; ++i) out[10 + i] = a.extra[i];
      for (int i = 0; i < 10; ++i) out[i] = 0;
      out[26] = 0; out[27] = 0;
      decompose_qstar(a.extra, a.faithful, out);
    }
    return;
  }
  int m = 0;  // rows so far (wave-uniform)
  for (int base = 0; base < a.n; base += 64) {
    const int i = base + lane;
    double rowsv[4][10];
    int cnt = 0;
    if (i < a.n) {
      const double* d = boxes + 4 * i;
      if (!(d[0] < 1 && d[1] < 1 && d[2] < 1 && d[3] < 1)) {
        SE3 Twc = se3_load(poses + 7 * i);
        Twc.r = q_normalize_pos(Twc.r);  // SE3Quat(Vector7d) ctor normalises (se3quat.h:66-69)
        const SE3 Tcw = se3_inv(Twc);
        const Mat3 R = q_to_R(Tcw.r);
        double P[12];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double c0 = c < 3 ? R.m[c] : Tcw.t[0], c1 = c < 3 ? R.m[3 + c] : Tcw.t[1], c2 = c < 3 ? R.m[6 + c] : Tcw.t[2];
          P[c] = a.K[0] * c0 + a.K[2] * c2; P[4 + c] = a.K[1] * c1 + a.K[3] * c2; P[8 + c] = c2;
        }
        const double lines[4][3] = {{1, 0, -d[0]}, {0, 1, -d[1]}, {1, 0, -d[2]}, {0, 1, -d[3]}};
        const bool keep[4] = {d[0] > 0 && d[0] < a.cols - 1, d[1] > 0 && d[1] < a.rows - 1, d[2] > 0 && d[2] < a.cols - 1,
                              d[3] > 0 && d[3] < a.rows - 1};
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          if (!keep[l]) continue;
          double p[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) p[c] = P[c] * lines[l][0] + P[4 + c] * lines[l][1] + P[8 + c] * lines[l][2];
          double* v = rowsv[cnt++];
          v[0] = p[0] * p[0]; v[1] = 2 * p[0] * p[1]; v[2] = 2 * p[0] * p[2]; v[3] = 2 * p[0] * p[3]; v[4] = p[1] * p[1];
          v[5] = 2 * p[1] * p[2]; v[6] = 2 * p[1] * p[3]; v[7] = p[2] * p[2]; v[8] = 2 * p[2] * p[3]; v[9] = p[3] * p[3];
        }
      }
    }
    // exclusive prefix sum of cnt over the wave -> compacted row offsets (keeps observation order)
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    const int excl = incl - cnt;
    for (int k = 0; k < cnt; ++k)
      for (int c = 0; c < 10; ++c) A[(size_t)(m + excl + k) * 10 + c] = rowsv[k][c];
    m += __shfl(incl, 63, 64);
  }
  for (int idx = lane; idx < 100; idx += 64) V[idx] = (idx / 10 == idx % 10) ? 1.0 : 0.0;
  __syncthreads();
  if (a.mode == 2) {   // quadricErrorWithPlanes (Initializer.cpp:271-284): sum over the planes of (v(pi) . q_hat)^2
    SE3 T = se3_load(a.extra);
    const Mat3 R = q_to_R(T.r);
    const double d[4] = {a.extra[7] * a.extra[7], a.extra[8] * a.extra[8], a.extra[9] * a.extra[9], -1.0};
    double Z[16], Qs[16];   // Q* = Z diag(a^2, b^2, c^2, -1) Z^T (Ellipsoid.cpp:290-300)
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Z[i * 4 + j] = R.m[i * 3 + j]; Z[i * 4 + 3] = T.t[i]; Z[12 + i] = 0; }
    Z[15] = 1;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) { double v = 0; for (int k = 0; k < 4; ++k) v += Z[i * 4 + k] * d[k] * Z[j * 4 + k]; Qs[i * 4 + j] = v; }
    const double qh[10] = {Qs[0], Qs[1], Qs[2], Qs[3], Qs[5], Qs[6], Qs[7], Qs[10], Qs[11], Qs[15]};
    double err = 0;
    for (int r = lane; r < m; r += 64) {
      double v = 0;
      for (int k = 0; k < 10; ++k) v += A[(size_t)r * 10 + k] * qh[k];
      err += v * v;
    }
    err = wave_allsum(err);
    if (lane < 27) out[lane] = 0.0;
    if (lane == 0) { out[27] = err; out[26] = 1.0; }
    return;
  }
  if (m < 9) {  // at least 9 planes are needed (Initializer.cpp:38)
    if (lane < 28) out[lane] = 0.0;
    return;
  }
  // one-sided Jacobi SVD on the columns of A
  for (int sweep = 0; sweep < 60; ++sweep) {
    int rotated = 0;
    for (int p = 0; p < 10; ++p)
      for (int q = p + 1; q < 10; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int r = lane; r < m; r += 64) {
          const double ap = A[(size_t)r * 10 + p], aq = A[(size_t)r * 10 + q];
          al += ap * ap; be += aq * aq; ga += ap * aq;
        }
        al = wave_allsum(al); be = wave_allsum(be); ga = wave_allsum(ga);
        if (fabs(ga) <= 1e-15 * sqrt(al * be) || ga == 0.0) continue;
        rotated = 1;
        const double zeta = (be - al) / (2 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1 + zeta * zeta));
        const double cs = 1 / sqrt(1 + t * t), sn = cs * t;
        for (int r = lane; r < m; r += 64) {
          const double ap = A[(size_t)r * 10 + p], aq = A[(size_t)r * 10 + q];
          A[(size_t)r * 10 + p] = cs * ap - sn * aq;
          A[(size_t)r * 10 + q] = sn * ap + cs * aq;
        }
        if (lane < 10) {
          const double vp = V[lane * 10 + p], vq = V[lane * 10 + q];
          V[lane * 10 + p] = cs * vp - sn * vq;
          V[lane * 10 + q] = sn * vp + cs * vq;
        }
        __syncthreads();
      }
    if (!rotated) break;
  }
  int best = 0;
  double bn = -1;
  for (int c = 0; c < 10; ++c) {
    double s = 0;
    for (int r = lane; r < m; r += 64) s += A[(size_t)r * 10 + c] * A[(size_t)r * 10 + c];
    s = wave_allsum(s);
    if (bn < 0 || s < bn) { bn = s; best = c; }
  }
  if (lane != 0) return;
  double q[10];
  for (int r = 0; r < 10; ++r) q[r] = V[r * 10 + best];
  if (q[9] < 0)
    for (int r = 0; r < 10; ++r) q[r] = -q[r];  // sign convention: Q*_33 > 0
  const double Qs[16] = {q[0], q[1], q[2], q[3], q[1], q[4], q[5], q[6], q[2], q[5], q[7], q[8], q[3], q[6], q[8], q[9]};
  for (int i = 0; i < 16; ++i) out[10 + i] = Qs[i];
  for (int i = 0; i < 10; ++i) out[i] = 0;
  out[26] = 0; out[27] = 0;
  decompose_qstar(Qs, a.faithful, out);
}

// getEllipsoidFromQStar (Initializer.cpp:186-248); faithful = 0: the exact decomposition through Q_33
__device__ void decompose_qstar(const double* Qs, int faithful, double* __restrict__ out) {
  const double t[3] = {Qs[3] / Qs[15], Qs[7] / Qs[15], Qs[11] / Qs[15]};
  double s[3], Rm[9];
  if (faithful) {
    double Qi[16], Q[16], w4[4], V4[16], tmp[16];
    const double cb = cbrt(inv_det<4>(Qs, Qi));
    for (int i = 0; i < 16; ++i) Q[i] = Qi[i] * cb;
    for (int i = 0; i < 4; ++i)
      for (int j = i + 1; j < 4; ++j) { const double v = 0.5 * (Q[i * 4 + j] + Q[j * 4 + i]); Q[i * 4 + j] = v; Q[j * 4 + i] = v; }
    sym_eig<4>(Q, w4, V4);
    int np = 0, nn = 0;
    for (int i = 0; i < 4; ++i) { np += w4[i] > 0; nn += w4[i] < 0; }
    if (!((np == 3 && nn == 1) || (np == 1 && nn == 3))) return;
    if (w4[3] > 0) {
      for (int i = 0; i < 16; ++i) Q[i] = -Q[i];
      sym_eig<4>(Q, w4, V4);
    }
    const double Q33[9] = {Q[0], Q[1], Q[2], Q[4], Q[5], Q[6], Q[8], Q[9], Q[10]};
    const double k = inv_det<4>(Q, tmp) / inv_det<3>(Q33, tmp);
    for (int i = 0; i < 3; ++i) s[i] = sqrt(fabs(-k * (1.0 / w4[i])));
    double w3[3];
    sym_eig<3>(Q33, w3, Rm);
  } else {
    const double sc = -1.0 / Qs[15];
    double M[9], w3[3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) M[i * 3 + j] = Qs[i * 4 + j] * sc + t[i] * t[j];
    for (int i = 0; i < 3; ++i)
      for (int j = i + 1; j < 3; ++j) { const double v = 0.5 * (M[i * 3 + j] + M[j * 3 + i]); M[i * 3 + j] = v; M[j * 3 + i] = v; }
    sym_eig<3>(M, w3, Rm);
    if (!(w3[0] > 0)) return;
    for (int i = 0; i < 3; ++i) s[i] = sqrt(w3[i]);
    const double det = Rm[0] * (Rm[4] * Rm[8] - Rm[5] * Rm[7]) - Rm[1] * (Rm[3] * Rm[8] - Rm[5] * Rm[6]) + Rm[2] * (Rm[3] * Rm[7] - Rm[4] * Rm[6]);
    if (det < 0)
      for (int r = 0; r < 3; ++r) Rm[r * 3 + 2] = -Rm[r * 3 + 2];
  }
  // rot_to_euler_zyx (src/utils/matrix_utils.cpp:75-95) then ellipsoid::fromMinimalVector (Ellipsoid.cpp:16-22)
  double roll, pitch, yaw;
  pitch = asin(-Rm[6]);
  if (fabs(pitch - M_PI / 2.0) < 1.0e-3) { roll = 0.0; yaw = atan2(Rm[5] - Rm[1], Rm[2] + Rm[4]) + roll; }
  else if (fabs(pitch + M_PI / 2.0) < 1.0e-3) { roll = 0.0; yaw = atan2(Rm[5] - Rm[1], Rm[2] + Rm[4]) - roll; }
  else { roll = atan2(Rm[7], Rm[8]); yaw = atan2(Rm[3], Rm[0]); }
  const double sy = sin(yaw * 0.5), cy = cos(yaw * 0.5), sp = sin(pitch * 0.5), cp = cos(pitch * 0.5);
  const double sr = sin(roll * 0.5), cr = cos(roll * 0.5);
  Quat qq;
  qq.w = cr * cp * cy + sr * sp * sy;
  qq.x = sr * cp * cy - cr * sp * sy;
  qq.y = cr * sp * cy + sr * cp * sy;
  qq.z = cr * cp * sy - sr * sp * cy;
  qq = q_normalize_pos(qq);
  out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
  out[3] = qq.x; out[4] = qq.y; out[5] = qq.z; out[6] = qq.w;
  out[7] = s[0]; out[8] = s[1]; out[9] = s[2];
  out[26] = 1.0;
}

// ---- esl_init_quadrics: the same per-object arithmetic for many objects in one call -------------------------------------------------
// One workgroup of one wavefront per object.  The host groups the observation list by object (esl_init_group.hpp) and sorts the
// objects by falling observation count; an object's plane matrix (320 bytes per observation) lives
//   - in LDS in a tile of kInitTileSmall observations  (k_init_quadrics<kInitTileSmall>: 31.8 KB, five workgroups per CU),
//   - in LDS in a tile of kInitTile observations       (k_init_quadrics<kInitTile>: 80.4 KB, two workgroups per CU),
//   - or in its rows of a global slab when it has more than kInitTile observations (stats[3] = 1; launched with the small tile, which
//     it does not use, so that it does not take a large tile's place).
// Which of the three holds depends on the object's own observation count alone, and the arithmetic is the same code over either
// pointer, so an object's result does not depend on what else is in the batch.
#ifndef ESL_INIT_TILE
#define ESL_INIT_TILE 248
#endif
#ifndef ESL_INIT_TILE_SMALL
#define ESL_INIT_TILE_SMALL 96
#endif
constexpr int kInitTile = ESL_INIT_TILE;              // T of include/esl.h: the most observations whose plane matrix stays on chip
constexpr int kInitTileSmall = ESL_INIT_TILE_SMALL;
static_assert(kInitTileSmall >= 1 && kInitTileSmall <= kInitTile, "the small tile is the first bin");
static_assert((132 + (size_t)kInitTile * 40) * sizeof(double) <= 160 * 1024, "the tile has to fit a CU's LDS");

struct InitBatchArgs {
  const double* cams;                       // Tcw, 7 doubles per frame
  const int* obs_cam; const double* obs_box; // the caller's list as given
  const int* idx;                           // positions in the list, grouped by object
  const InitObj* order;                     // the launch list: [first, first + count) of this launch
  double K[4];
  int rows, cols, faithful, min_obs;
  double* slab;
  double* ell; double* qstar; double* perr; int* stats;   // qstar, perr, stats may be null
};

// getPlanesHomo (Initializer.cpp:58-91) for the observations of one object: the kept lines' monomial rows to A, compacted in
// observation order; returns the row count (wave-uniform).  The row arithmetic is k_init_quadric's, on Tcw as given.
static __device__ int init_plane_rows(const InitBatchArgs& a, const InitObj& e, double* A) {
  const int lane = threadIdx.x;
  int m = 0;
  for (int base = 0; base < e.n; base += 64) {
    const int i = base + lane;
    double rowsv[4][10];
    int cnt = 0;
    if (i < e.n) {
      const int k = a.idx[e.first + i];
      const double* d = a.obs_box + 4 * (size_t)k;
      if (!(d[0] < 1 && d[1] < 1 && d[2] < 1 && d[3] < 1)) {
        SE3 Tcw = se3_load(a.cams + 7 * (size_t)a.obs_cam[k]);
        Tcw.r = q_normalize_pos(Tcw.r);  // SE3Quat(Vector7d) ctor normalises (se3quat.h:66-69)
        const Mat3 R = q_to_R(Tcw.r);
        double P[12];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double c0 = c < 3 ? R.m[c] : Tcw.t[0], c1 = c < 3 ? R.m[3 + c] : Tcw.t[1], c2 = c < 3 ? R.m[6 + c] : Tcw.t[2];
          P[c] = a.K[0] * c0 + a.K[2] * c2; P[4 + c] = a.K[1] * c1 + a.K[3] * c2; P[8 + c] = c2;
        }
        const double lines[4][3] = {{1, 0, -d[0]}, {0, 1, -d[1]}, {1, 0, -d[2]}, {0, 1, -d[3]}};
        const bool keep[4] = {d[0] > 0 && d[0] < a.cols - 1, d[1] > 0 && d[1] < a.rows - 1, d[2] > 0 && d[2] < a.cols - 1,
                              d[3] > 0 && d[3] < a.rows - 1};
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          if (!keep[l]) continue;
          double p[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) p[c] = P[c] * lines[l][0] + P[4 + c] * lines[l][1] + P[8 + c] * lines[l][2];
          double* v = rowsv[cnt++];
          v[0] = p[0] * p[0]; v[1] = 2 * p[0] * p[1]; v[2] = 2 * p[0] * p[2]; v[3] = 2 * p[0] * p[3]; v[4] = p[1] * p[1];
          v[5] = 2 * p[1] * p[2]; v[6] = 2 * p[1] * p[3]; v[7] = p[2] * p[2]; v[8] = 2 * p[2] * p[3]; v[9] = p[3] * p[3];
        }
      }
    }
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    const int excl = incl - cnt;
    for (int k = 0; k < cnt; ++k)
      for (int c = 0; c < 10; ++c) A[(size_t)(m + excl + k) * 10 + c] = rowsv[k][c];
    m += __shfl(incl, 63, 64);
  }
  return m;
}

// every output of an object that is not initialised (statuses 1 and 2) is zero
static __device__ void init_reject(const InitBatchArgs& a, const InitObj& e, int status, int planes) {
  const int lane = threadIdx.x;
  if (lane < 10) a.ell[(size_t)e.obj * 10 + lane] = 0.0;
  if (a.qstar && lane < 16) a.qstar[(size_t)e.obj * 16 + lane] = 0.0;
  if (lane == 0) {
    if (a.perr) a.perr[e.obj] = 0.0;
    if (a.stats) { int* s = a.stats + (size_t)e.obj * 4; s[0] = status; s[1] = e.n; s[2] = planes; s[3] = (status == 2 && e.spill >= 0) ? 1 : 0; }
  }
}

template <int TILE>
static __global__ __launch_bounds__(64) void k_init_quadrics(InitBatchArgs a, int first) {
  // V 10 x 10 | the result as k_init_quadric lays it out (28) + padding | the tile
  __shared__ __attribute__((aligned(16))) double sm[132 + TILE * 40];
  const InitObj e = a.order[first + blockIdx.x];
  const int lane = threadIdx.x;
  if (e.n < a.min_obs) { init_reject(a, e, 1, 0); return; }
  double* V = sm;
  double* res = sm + 100;
  double* A = e.spill >= 0 ? a.slab + (size_t)e.spill * 40 : sm + 132;   // e.spill < 0 only when e.n <= TILE (the host's bins)
  const int m = init_plane_rows(a, e, A);
  for (int idx = lane; idx < 100; idx += 64) V[idx] = (idx / 10 == idx % 10) ? 1.0 : 0.0;
  __syncthreads();
  if (m < 9) { init_reject(a, e, 2, m); return; }   // at least 9 planes are needed (Initializer.cpp:38)
  // one-sided Jacobi SVD on the columns of A, as in k_init_quadric
  for (int sweep = 0; sweep < 60; ++sweep) {
    int rotated = 0;
    for (int p = 0; p < 10; ++p)
      for (int q = p + 1; q < 10; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int r = lane; r < m; r += 64) {
          const double ap = A[(size_t)r * 10 + p], aq = A[(size_t)r * 10 + q];
          al += ap * ap; be += aq * aq; ga += ap * aq;
        }
        al = wave_allsum(al); be = wave_allsum(be); ga = wave_allsum(ga);
        if (fabs(ga) <= 1e-15 * sqrt(al * be) || ga == 0.0) continue;
        rotated = 1;
        const double zeta = (be - al) / (2 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1 + zeta * zeta));
        const double cs = 1 / sqrt(1 + t * t), sn = cs * t;
        for (int r = lane; r < m; r += 64) {
          const double ap = A[(size_t)r * 10 + p], aq = A[(size_t)r * 10 + q];
          A[(size_t)r * 10 + p] = cs * ap - sn * aq;
          A[(size_t)r * 10 + q] = sn * ap + cs * aq;
        }
        if (lane < 10) {
          const double vp = V[lane * 10 + p], vq = V[lane * 10 + q];
          V[lane * 10 + p] = cs * vp - sn * vq;
          V[lane * 10 + q] = sn * vp + cs * vq;
        }
        __syncthreads();
      }
    if (!rotated) break;
  }
  int best = 0;
  double bn = -1;
  for (int c = 0; c < 10; ++c) {
    double s = 0;
    for (int r = lane; r < m; r += 64) s += A[(size_t)r * 10 + c] * A[(size_t)r * 10 + c];
    s = wave_allsum(s);
    if (bn < 0 || s < bn) { bn = s; best = c; }
  }
  if (lane == 0) {
    double q[10];
    for (int r = 0; r < 10; ++r) q[r] = V[r * 10 + best];
    if (q[9] < 0)
      for (int r = 0; r < 10; ++r) q[r] = -q[r];  // sign convention: Q*_33 > 0
    const double Qs[16] = {q[0], q[1], q[2], q[3], q[1], q[4], q[5], q[6], q[2], q[5], q[7], q[8], q[3], q[6], q[8], q[9]};
    for (int i = 0; i < 16; ++i) res[10 + i] = Qs[i];
    for (int i = 0; i < 10; ++i) res[i] = 0;
    res[26] = 0; res[27] = 0;
    decompose_qstar(Qs, a.faithful, res);
  }
  __syncthreads();
  const bool ok = res[26] > 0.5;
  if (lane < 10) a.ell[(size_t)e.obj * 10 + lane] = res[lane];
  if (a.qstar && lane < 16) a.qstar[(size_t)e.obj * 16 + lane] = res[10 + lane];
  if (lane == 0 && a.stats) { int* s = a.stats + (size_t)e.obj * 4; s[0] = ok ? 0 : 3; s[1] = e.n; s[2] = m; s[3] = e.spill >= 0 ? 1 : 0; }
  if (!a.perr) return;
  double err = 0;
  if (ok) {
    // quadricErrorWithPlanes of the ellipsoid just returned over this object's planes: the SVD rotated A away, so the rows are built
    // again, then k_init_quadric's mode 2
    (void)init_plane_rows(a, e, A);
    __syncthreads();
    SE3 T = se3_load(res);
    const Mat3 R = q_to_R(T.r);
    const double d[4] = {res[7] * res[7], res[8] * res[8], res[9] * res[9], -1.0};
    double Z[16], Qs[16];   // Q* = Z diag(a^2, b^2, c^2, -1) Z^T (Ellipsoid.cpp:290-300)
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Z[i * 4 + j] = R.m[i * 3 + j]; Z[i * 4 + 3] = T.t[i]; Z[12 + i] = 0; }
    Z[15] = 1;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) { double v = 0; for (int k = 0; k < 4; ++k) v += Z[i * 4 + k] * d[k] * Z[j * 4 + k]; Qs[i * 4 + j] = v; }
    const double qh[10] = {Qs[0], Qs[1], Qs[2], Qs[3], Qs[5], Qs[6], Qs[7], Qs[10], Qs[11], Qs[15]};
    for (int r = lane; r < m; r += 64) {
      double v = 0;
      for (int k = 0; k < 10; ++k) v += A[(size_t)r * 10 + k] * qh[k];
      err += v * v;
    }
    err = wave_allsum(err);
  }
  if (lane == 0) a.perr[e.obj] = err;
}

// ---- esl_init_quadrics_robust: consensus over small view subsets (include/esl.h, "consensus SVD initialisation") ----------------------
// One kernel, three passes over it (the launch's `pass`), one workgroup of one wavefront each:
//   pass 0  grid N x H: workgroup (o, h) fits hypothesis h of object o (at most 16 views = 64 plane rows in LDS, the Jacobi SVD and
//           decomposition above) and scores it over all of o's entries, lane-strided; its row of `hyp` is valid, planes, inliers, cost
//   pass 1  grid N: the statuses 1, 2 and 4, the winner of the object's rows by the total order (inliers down, cost up, h up), then the
//           winner's fit and score AGAIN through the same instructions as pass 0 -- the same bits, so nothing but four numbers per
//           hypothesis is kept between the passes -- with the per-entry residuals and flags and the plane error written this time
//   pass 2  grid N: the score of the refit's ellipsoid (esl_init_quadrics on the winner's inliers, called by the host in between)
// A lane adds its own entries' squared residuals in rising entry order and the 64 partial sums meet in the butterfly of wave_allsum:
// the order of every sum is fixed by n alone.  No atomics.
struct InitRobustArgs {
  InitBatchArgs b;          // cams, obs_cam, obs_box, idx, K, rows, cols, faithful, min_obs; the rest of it is not used
  const InitObj* objs;      // object o's entries are idx[first .. first + n); in object order, spill unused
  int H, sample_size, min_inliers;
  double inlier_px;
  unsigned long long seed;
  double* hyp;              // N x H x 4
  // per pass p = 1, 2 at [p - 1]: oi 8 ints per object (pass 1: status, planes, inliers, valid hypotheses, winner; pass 2: valid, inliers),
  // od 28 doubles per object (ellipsoid 10, Q* 16, cost, plane error), the residual and the flag of every list entry
  int* oi[2]; double* od[2]; double* res_e[2]; int* inl_e[2];
  const double* rf_ell; const int* rf_ok;   // pass 2: the refit's ellipsoids, and whether object o has one
};

__device__ __forceinline__ int wave_allsum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// which of the four lines of a box are kept (fromDetectionsToLines, Initializer.cpp:107-145); false when the detection contributes nothing
static __device__ bool init_entry_lines(const InitBatchArgs& a, const double* d, bool keep[4]) {
  keep[0] = d[0] > 0 && d[0] < a.cols - 1; keep[1] = d[1] > 0 && d[1] < a.rows - 1;
  keep[2] = d[2] > 0 && d[2] < a.cols - 1; keep[3] = d[3] > 0 && d[3] < a.rows - 1;
  if (d[0] < 1 && d[1] < 1 && d[2] < 1 && d[3] < 1) return false;
  return keep[0] || keep[1] || keep[2] || keep[3];
}

// the plane rows of list entry k: init_plane_rows' arithmetic for one observation; returns their count
static __device__ int init_entry_rows(const InitBatchArgs& a, int k, double rowsv[4][10]) {
  const double* d = a.obs_box + 4 * (size_t)k;
  bool keep[4];
  if (!init_entry_lines(a, d, keep)) return 0;
  SE3 Tcw = se3_load(a.cams + 7 * (size_t)a.obs_cam[k]);
  Tcw.r = q_normalize_pos(Tcw.r);
  const Mat3 R = q_to_R(Tcw.r);
  double P[12];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double c0 = c < 3 ? R.m[c] : Tcw.t[0], c1 = c < 3 ? R.m[3 + c] : Tcw.t[1], c2 = c < 3 ? R.m[6 + c] : Tcw.t[2];
    P[c] = a.K[0] * c0 + a.K[2] * c2; P[4 + c] = a.K[1] * c1 + a.K[3] * c2; P[8 + c] = c2;
  }
  const double lines[4][3] = {{1, 0, -d[0]}, {0, 1, -d[1]}, {1, 0, -d[2]}, {0, 1, -d[3]}};
  int cnt = 0;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    if (!keep[l]) continue;
    double p[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) p[c] = P[c] * lines[l][0] + P[4 + c] * lines[l][1] + P[8 + c] * lines[l][2];
    double* v = rowsv[cnt++];
    v[0] = p[0] * p[0]; v[1] = 2 * p[0] * p[1]; v[2] = 2 * p[0] * p[2]; v[3] = 2 * p[0] * p[3]; v[4] = p[1] * p[1];
    v[5] = 2 * p[1] * p[2]; v[6] = 2 * p[1] * p[3]; v[7] = p[2] * p[2]; v[8] = 2 * p[2] * p[3]; v[9] = p[3] * p[3];
  }
  return cnt;
}

// r_i of step 4: the largest |b_k - d_k| over the kept lines, b the unclipped box the bbox edge projects; +inf when the entry has no
// kept line, the edge's visibility predicate fails or b is not finite
static __device__ double init_entry_residual(const InitBatchArgs& a, int k, const Ell& e) {
  const double inf = __builtin_inf();
  const double* d = a.obs_box + 4 * (size_t)k;
  bool keep[4];
  if (!init_entry_lines(a, d, keep)) return inf;
  SE3 Tcw = se3_load(a.cams + 7 * (size_t)a.obs_cam[k]);
  Tcw.r = q_normalize_pos(Tcw.r);
  if (!bbox_edge_visible(Tcw, e, a.K, a.rows, a.cols)) return inf;
  BoxGeom g;
  box_geom(Tcw, e, a.K, g);
  double bb[4], sq[2];
  box_from_conic(g, bb, sq);
  double r = 0;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    if (!(fabs(bb[l]) < inf)) return inf;   // NaN or infinite
    if (keep[l]) r = fmax(r, fabs(bb[l] - d[l]));
  }
  return r;
}

static __global__ __launch_bounds__(64) void k_init_robust(InitRobustArgs a, int pass) {
  // V 10 x 10 | the result as k_init_quadric lays it out (28) + padding | at most 16 views x 4 plane rows
  __shared__ __attribute__((aligned(16))) double sm[132 + 4 * kInitSampleMax * 10];
  __shared__ int smp[kInitSampleMax];   // the list positions of the hypothesis's entries
  const int lane = threadIdx.x;
  const int o = pass == 0 ? (int)(blockIdx.x / (unsigned)a.H) : (int)blockIdx.x;
  int h = pass == 0 ? (int)(blockIdx.x % (unsigned)a.H) : -1;
  const InitObj e = a.objs[o];
  double* V = sm;
  double* res = sm + 100;
  double* A = sm + 132;
  const int nh = init_sample_count(e.n, a.sample_size, a.H);
  double* rows_o = a.hyp + (size_t)o * a.H * 4;
  int planes = 0, nvalid = 0;
  if (pass == 0 && (e.n < a.b.min_obs || h >= nh)) {
    if (lane < 4) rows_o[(size_t)h * 4 + lane] = 0.0;
    return;
  }
  if (pass == 1) {
    int status = 0;
    if (e.n < a.b.min_obs) status = 1;
    else {
      for (int i = lane; i < e.n; i += 64) {
        const double* d = a.b.obs_box + 4 * (size_t)a.b.idx[e.first + i];
        bool keep[4];
        if (init_entry_lines(a.b, d, keep)) planes += (int)keep[0] + (int)keep[1] + (int)keep[2] + (int)keep[3];
      }
      planes = wave_allsum_i(planes);
      if (planes < 9) status = 2;   // at least 9 planes are needed (Initializer.cpp:38)
    }
    // the winner of the object's rows: inliers down, then cost up, then h up -- a total order, so the butterfly's pairing does not matter
    int bn = -1, bh = 0x7fffffff;
    double bc = 0;
    if (!status) {
      for (int hh = lane; hh < nh; hh += 64) {
        const double* row = rows_o + (size_t)hh * 4;
        if (!(row[0] > 0.5)) continue;
        ++nvalid;
        const int n = (int)row[2];
        const double cst = row[3];
        if (n > bn || (n == bn && (cst < bc || (cst == bc && hh < bh)))) { bn = n; bc = cst; bh = hh; }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const int on = __shfl_xor(bn, off, 64), oh = __shfl_xor(bh, off, 64);
        const double oc = __shfl_xor(bc, off, 64);
        if (on > bn || (on == bn && (oc < bc || (oc == bc && oh < bh)))) { bn = on; bc = oc; bh = oh; }
      }
      nvalid = wave_allsum_i(nvalid);
      if (bn < 0) status = 4;
    }
    if (status) {
      if (status != 4)
        for (int t = lane; t < a.H * 4; t += 64) rows_o[t] = 0.0;
      if (lane < 28) a.od[0][(size_t)o * 28 + lane] = 0.0;
      if (lane < 8) a.oi[0][(size_t)o * 8 + lane] = lane == 0 ? status : lane == 1 ? planes : lane == 4 ? -1 : 0;
      return;
    }
    h = bh;
  }
  int m = 0;
  bool valid = false;
  if (pass != 2) {
    const int s = init_sample_views(e.n, a.sample_size);
    if (lane == 0) {
      int32_t loc[kInitSampleMax];
      init_sample(a.seed, h, e.n, a.sample_size, loc);
      for (int k = 0; k < s; ++k) smp[k] = a.b.idx[e.first + loc[k]];
    }
    __syncthreads();
    double rowsv[4][10];
    const int cnt = lane < s ? init_entry_rows(a.b, smp[lane], rowsv) : 0;
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    const int excl = incl - cnt;
    for (int k = 0; k < cnt; ++k)
      for (int c = 0; c < 10; ++c) A[(excl + k) * 10 + c] = rowsv[k][c];
    m = __shfl(incl, 63, 64);   // <= 4 s <= 64
    for (int idx = lane; idx < 100; idx += 64) V[idx] = (idx / 10 == idx % 10) ? 1.0 : 0.0;
    if (lane < 32) res[lane] = 0.0;
    __syncthreads();
    if (m >= 9) {
      // one-sided Jacobi SVD on the columns of A and the decomposition, as in k_init_quadrics
      for (int sweep = 0; sweep < 60; ++sweep) {
        int rotated = 0;
        for (int p = 0; p < 10; ++p)
          for (int q = p + 1; q < 10; ++q) {
            double al = 0, be = 0, ga = 0;
            for (int r = lane; r < m; r += 64) {
              const double ap = A[(size_t)r * 10 + p], aq = A[(size_t)r * 10 + q];
              al += ap * ap; be += aq * aq; ga += ap * aq;
            }
            al = wave_allsum(al); be = wave_allsum(be); ga = wave_allsum(ga);
            if (fabs(ga) <= 1e-15 * sqrt(al * be) || ga == 0.0) continue;
            rotated = 1;
            const double zeta = (be - al) / (2 * ga);
            const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1 + zeta * zeta));
            const double cs = 1 / sqrt(1 + t * t), sn = cs * t;
            for (int r = lane; r < m; r += 64) {
              const double ap = A[(size_t)r * 10 + p], aq = A[(size_t)r * 10 + q];
              A[(size_t)r * 10 + p] = cs * ap - sn * aq;
              A[(size_t)r * 10 + q] = sn * ap + cs * aq;
            }
            if (lane < 10) {
              const double vp = V[lane * 10 + p], vq = V[lane * 10 + q];
              V[lane * 10 + p] = cs * vp - sn * vq;
              V[lane * 10 + q] = sn * vp + cs * vq;
            }
            __syncthreads();
          }
        if (!rotated) break;
      }
      int best = 0;
      double bn = -1;
      for (int c = 0; c < 10; ++c) {
        double sq = 0;
        for (int r = lane; r < m; r += 64) sq += A[(size_t)r * 10 + c] * A[(size_t)r * 10 + c];
        sq = wave_allsum(sq);
        if (bn < 0 || sq < bn) { bn = sq; best = c; }
      }
      if (lane == 0) {
        double q[10];
        for (int r = 0; r < 10; ++r) q[r] = V[r * 10 + best];
        if (q[9] < 0)
          for (int r = 0; r < 10; ++r) q[r] = -q[r];  // sign convention: Q*_33 > 0
        const double Qs[16] = {q[0], q[1], q[2], q[3], q[1], q[4], q[5], q[6], q[2], q[5], q[7], q[8], q[3], q[6], q[8], q[9]};
        for (int i = 0; i < 16; ++i) res[10 + i] = Qs[i];
        decompose_qstar(Qs, a.b.faithful, res);
      }
      __syncthreads();
      valid = res[26] > 0.5;
    }
  } else {
    valid = a.rf_ok[o] != 0;
    if (lane < 10) res[lane] = a.rf_ell[(size_t)o * 10 + lane];
    __syncthreads();
  }
  // the score over all entries of the object; passes 1 and 2 also leave every entry's residual and flag, and the plane error of the
  // ellipsoid over the inliers' planes (quadricErrorWithPlanes, Initializer.cpp:271-284)
  int n_in = 0;
  double cost = 0, perr = 0;
  if (valid) {
    const Ell el = ell_load(res);
    double qh[10];
    if (pass != 0) {
      const Mat3 R = q_to_R(el.pose.r);
      const double d[4] = {el.s[0] * el.s[0], el.s[1] * el.s[1], el.s[2] * el.s[2], -1.0};
      double Z[16], Qs[16];   // Q* = Z diag(a^2, b^2, c^2, -1) Z^T (Ellipsoid.cpp:290-300)
      for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Z[i * 4 + j] = R.m[i * 3 + j]; Z[i * 4 + 3] = el.pose.t[i]; Z[12 + i] = 0; }
      Z[15] = 1;
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { double v = 0; for (int k = 0; k < 4; ++k) v += Z[i * 4 + k] * d[k] * Z[j * 4 + k]; Qs[i * 4 + j] = v; }
      qh[0] = Qs[0]; qh[1] = Qs[1]; qh[2] = Qs[2]; qh[3] = Qs[3]; qh[4] = Qs[5]; qh[5] = Qs[6]; qh[6] = Qs[7]; qh[7] = Qs[10]; qh[8] = Qs[11]; qh[9] = Qs[15];
    }
    for (int i = lane; i < e.n; i += 64) {
      const int k = a.b.idx[e.first + i];
      const double r = init_entry_residual(a.b, k, el);
      const bool in = r <= a.inlier_px;
      if (in) { ++n_in; cost += r * r; }
      if (pass != 0) {
        a.res_e[pass - 1][k] = r;
        a.inl_e[pass - 1][k] = in ? 1 : 0;
        if (in) {
          double rowsv[4][10];
          const int cnt = init_entry_rows(a.b, k, rowsv);
          for (int l = 0; l < cnt; ++l) {
            double v = 0;
            for (int c = 0; c < 10; ++c) v += rowsv[l][c] * qh[c];
            perr += v * v;
          }
        }
      }
    }
    n_in = wave_allsum_i(n_in);
    cost = wave_allsum(cost);
    if (pass != 0) perr = wave_allsum(perr);
  }
  if (pass == 0) {
    if (lane < 4) rows_o[(size_t)h * 4 + lane] = lane == 0 ? (valid ? 1.0 : 0.0) : lane == 1 ? (double)m : lane == 2 ? (double)n_in : cost;
    return;
  }
  double* od = a.od[pass - 1] + (size_t)o * 28;
  int* oi = a.oi[pass - 1] + (size_t)o * 8;
  if (lane < 26) od[lane] = valid ? res[lane] : 0.0;
  if (lane == 26) od[26] = cost;
  if (lane == 27) od[27] = perr;
  if (pass == 1) {
    const int status = !valid ? 4 : n_in < a.min_inliers ? 5 : 0;   // !valid cannot happen: pass 0 found this hypothesis valid
    if (lane < 8) oi[lane] = lane == 0 ? status : lane == 1 ? planes : lane == 2 ? n_in : lane == 3 ? nvalid : lane == 4 ? h : 0;
  } else {
    if (lane < 8) oi[lane] = lane == 0 ? (valid ? 1 : 0) : lane == 1 ? n_in : 0;
  }
}

struct InitRobustState {   // InitBatchState::rob
  enum { R_CAMS, R_OCAM, R_BOX, R_IDX, R_OBJS, R_HYP, R_OI, R_OD, R_RES, R_INL, R_RFELL, R_RFOK, kBufs };
  ScratchSet<kBufs> set;
  // the host's grouping, what comes back from the passes and the refit's list and results, kept for their capacity
  std::vector<int32_t> offsets, idx, masked, oi, inl, rf_ok, rf_stats;
  std::vector<InitObj> objs;
  std::vector<double> od, res, rf_ell, rf_qs, rf_perr;
};

struct InitBatchState {   // esl_ctx::init_batch
  enum { B_CAMS, B_OCAM, B_BOX, B_IDX, B_ORDER, B_SLAB, B_ELL, B_QS, B_PERR, B_STATS, kBufs };
  ScratchSet<kBufs> set;
  std::vector<int32_t> offsets, idx;   // the host's grouping, kept for their capacity
  std::vector<InitObj> order;
  InitRobustState* rob = nullptr;      // esl_init_quadrics_robust's own buffers
};

void init_batch_release(esl_ctx* c) {   // called by esl_ctx_destroy
  InitBatchState* s = c->init_batch;
  if (!s) return;
  s->set.release();
  if (s->rob) s->rob->set.release();
  delete s->rob;
  delete s;
  c->init_batch = nullptr;
}

void init_scratch_stats(const esl_ctx* c, bool robust, int64_t* allocs, int64_t* bytes) {
  const InitBatchState* s = c->init_batch;
  if (s && !robust) { *allocs = s->set.allocs(); *bytes = (int64_t)s->set.held(); }
  if (s && robust && s->rob) { *allocs = s->rob->set.allocs(); *bytes = (int64_t)s->rob->set.held(); }
}

}  // namespace esl

using namespace esl;

namespace {
struct DevBuf {   // released on every exit path
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) { ESL_HIP_TRY(hipMalloc(&p, bytes ? bytes : 8)); return ESL_OK; }
};
// the plane matrix (40 doubles per observation) stays in LDS while it fits what the context's device offers per workgroup
// (gfx950: 160 KB => up to 480 observations); beyond that it goes to HBM

int init_launch(esl_ctx* c, const double* poses_Twc, const double* bboxes, int32_t n, const double K[4], int32_t rows, int32_t cols,
                int32_t faithful, int mode, const double* extra, int n_extra, double h[28]) {
  ESL_HIP_TRY(hipSetDevice(c->device));
  DevBuf dp, db, dout, dA;
  int rc;
  if ((rc = dp.alloc((size_t)n * 7 * sizeof(double))) || (rc = db.alloc((size_t)n * 4 * sizeof(double))) || (rc = dout.alloc(28 * sizeof(double))))
    return rc;
  if (n) {
    ESL_HIP_TRY(hipMemcpyAsync(dp.p, poses_Twc, (size_t)n * 7 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(db.p, bboxes, (size_t)n * 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  InitArgs a{};
  a.K[0] = K[0]; a.K[1] = K[1]; a.K[2] = K[2]; a.K[3] = K[3];
  a.n = n; a.rows = rows; a.cols = cols; a.faithful = faithful; a.mode = mode;
  for (int i = 0; i < n_extra; ++i) a.extra[i] = extra[i];
  size_t lds = 100 * sizeof(double);
  int lds_max = 0;
  ESL_HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
  if (lds + (size_t)n * 40 * sizeof(double) > (size_t)lds_max) {
    if ((rc = dA.alloc((size_t)n * 40 * sizeof(double)))) return rc;
    a.a_glob = (double*)dA.p;
  } else {
    lds += (size_t)n * 40 * sizeof(double);
  }
  ESL_HIP_TRY(hipFuncSetAttribute((const void*)k_init_quadric, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_init_quadric, dim3(1), dim3(64), lds, c->stream, (const double*)dp.p, (const double*)db.p, a, (double*)dout.p);
  ESL_HIP_TRY(hipGetLastError());
  ESL_HIP_TRY(hipMemcpyAsync(h, dout.p, 28 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  return ESL_OK;
}
}  // namespace

extern "C" int esl_init_quadric(esl_ctx* c, const double* poses_Twc, const double* bboxes, int32_t n, const double K[4],
                                int32_t rows, int32_t cols, int32_t faithful, double ellipsoid_out[10], double qstar_out[16],
                                int32_t* ok) {
  if (!c || !poses_Twc || !bboxes || !K || !ellipsoid_out || !qstar_out || !ok || n < 0) return ESL_ERR_INVALID;
  *ok = 0;
  for (int i = 0; i < 10; ++i) ellipsoid_out[i] = 0;
  for (int i = 0; i < 16; ++i) qstar_out[i] = 0;
  if (n < 3) return ESL_OK;  // < 9 planes possible only
  double h[28];
  const int rc = init_launch(c, poses_Twc, bboxes, n, K, rows, cols, faithful, 0, nullptr, 0, h);
  if (rc) return rc;
  for (int i = 0; i < 10; ++i) ellipsoid_out[i] = h[i];
  for (int i = 0; i < 16; ++i) qstar_out[i] = h[10 + i];
  *ok = h[26] > 0.5 ? 1 : 0;
  return ESL_OK;
}

extern "C" int esl_init_from_qstar(esl_ctx* c, const double qstar[16], int32_t faithful, double ellipsoid_out[10], int32_t* ok) {
  if (!c || !qstar || !ellipsoid_out || !ok) return ESL_ERR_INVALID;
  const double K[4] = {1, 1, 0, 0};
  double h[28];
  const int rc = init_launch(c, nullptr, nullptr, 0, K, 0, 0, faithful, 1, qstar, 16, h);
  if (rc) return rc;
  for (int i = 0; i < 10; ++i) ellipsoid_out[i] = h[i];
  *ok = h[26] > 0.5 ? 1 : 0;
  return ESL_OK;
}

extern "C" int esl_init_plane_error(esl_ctx* c, const double* poses_Twc, const double* bboxes, int32_t n, const double K[4],
                                    int32_t rows, int32_t cols, const double ellipsoid[10], double* error_out) {
  if (!c || !K || !ellipsoid || !error_out || n < 0 || (n && (!poses_Twc || !bboxes))) return ESL_ERR_INVALID;
  double h[28];
  const int rc = init_launch(c, poses_Twc, bboxes, n, K, rows, cols, 1, 2, ellipsoid, 10, h);
  if (rc) return rc;
  *error_out = h[27];
  return ESL_OK;
}

namespace {

int init_batch_fail(const char* what, int rc) { set_error(std::string("esl_init_quadrics: ") + what); return rc; }

}  // namespace

extern "C" int esl_init_quadrics(esl_ctx* c, const double* cams, int32_t F, int32_t N, const int32_t* obs_cam, const int32_t* obs_obj,
                                 const double* obs_boxes, int64_t n_obs, const double K[4], int32_t rows, int32_t cols, int32_t faithful,
                                 int32_t min_observations, double* ellipsoids_out, double* qstar_out, double* plane_error_out,
                                 int32_t* stats_out) {
  if (!c || !K || F < 0 || N < 0 || n_obs < 0 || min_observations < 0) return init_batch_fail("bad argument (null pointer or negative count)", ESL_ERR_INVALID);
  if (n_obs > INT32_MAX) return init_batch_fail("more than 2^31 - 1 observations", ESL_ERR_INVALID);
  if (n_obs > 0 && (!obs_cam || !obs_obj || !obs_boxes)) return init_batch_fail("null observation array", ESL_ERR_INVALID);
  if (N > 0 && !ellipsoids_out) return init_batch_fail("null ellipsoids_out", ESL_ERR_INVALID);
  if (rows < 1 || cols < 1) return init_batch_fail("rows or cols < 1", ESL_ERR_INVALID);
  if (!cams) {
    if (!c->graph_loaded || !c->states_loaded) return init_batch_fail("cams == NULL needs a resident graph with states", ESL_ERR_STATE);
    if (F != c->g.n_cams) return init_batch_fail("F differs from the resident graph's n_cams", ESL_ERR_INVALID);
  }
  if (!c->init_batch) c->init_batch = new InitBatchState();
  InitBatchState* s = c->init_batch;
  typedef InitBatchState B;
  ScratchSet<B::kBufs>& d = s->set;
  int64_t bad = 0;
  const int grc = init_group(n_obs, N, F, obs_cam, obs_obj, s->offsets, s->idx, &bad);
  if (grc == INIT_GROUP_BAD_OBJ) return init_batch_fail(("obs_obj >= N at entry " + std::to_string(bad)).c_str(), ESL_ERR_INVALID);
  if (grc == INIT_GROUP_BAD_CAM) return init_batch_fail(("obs_cam outside [0, F) at entry " + std::to_string(bad)).c_str(), ESL_ERR_INVALID);
  if (N == 0) return ESL_OK;
  const int64_t slab = init_order(N, s->offsets, kInitTile, min_observations, s->order);
  if (slab < 0) return init_batch_fail("the spilled objects hold more than 2^31 - 1 observations", ESL_ERR_INVALID);
  // the launch list falls in n: [0, n_over) more than kInitTile observations, [n_over, n_mid) more than kInitTileSmall, the rest
  int n_over = 0, n_mid = 0;
  while (n_over < N && s->order[n_over].n > kInitTile) ++n_over;
  n_mid = n_over;
  while (n_mid < N && s->order[n_mid].n > kInitTileSmall) ++n_mid;

  ESL_HIP_TRY(hipSetDevice(c->device));
  InitBatchArgs k{};
  const size_t kept = s->idx.size();
  if (const int rc = source(c, d, B::B_CAMS, cams, c->cams, (size_t)F * 7 * sizeof(double), &k.cams)) return rc;
  if (const int rc = d.grow(c, B::B_OCAM, (size_t)n_obs * sizeof(int32_t))) return rc;
  if (const int rc = d.grow(c, B::B_BOX, (size_t)n_obs * 4 * sizeof(double))) return rc;
  if (const int rc = d.grow(c, B::B_IDX, kept * sizeof(int32_t))) return rc;
  if (const int rc = d.grow(c, B::B_SLAB, (size_t)slab * 40 * sizeof(double))) return rc;
  if (const int rc = d.grow(c, B::B_ELL, (size_t)N * 10 * sizeof(double))) return rc;
  if (kept) {   // entries that no object keeps are never read
    ESL_HIP_TRY(hipMemcpyAsync(d.buf[B::B_OCAM], obs_cam, (size_t)n_obs * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(d.buf[B::B_BOX], obs_boxes, (size_t)n_obs * 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(d.buf[B::B_IDX], s->idx.data(), kept * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  }
  if (const int rc = upload(c, d, B::B_ORDER, (const InitObj*)s->order.data(), (size_t)N * sizeof(InitObj), &k.order)) return rc;
  k.obs_cam = d.at<const int>(B::B_OCAM); k.obs_box = d.at<const double>(B::B_BOX);
  k.idx = d.at<const int>(B::B_IDX);
  k.slab = d.at<double>(B::B_SLAB); k.ell = d.at<double>(B::B_ELL);
  if (qstar_out) {
    if (const int rc = d.grow(c, B::B_QS, (size_t)N * 16 * sizeof(double))) return rc;
    k.qstar = d.at<double>(B::B_QS);
  }
  if (plane_error_out) {
    if (const int rc = d.grow(c, B::B_PERR, (size_t)N * sizeof(double))) return rc;
    k.perr = d.at<double>(B::B_PERR);
  }
  if (stats_out) {
    if (const int rc = d.grow(c, B::B_STATS, (size_t)N * 4 * sizeof(int32_t))) return rc;
    k.stats = d.at<int>(B::B_STATS);
  }
  for (int i = 0; i < 4; ++i) k.K[i] = K[i];
  k.rows = rows; k.cols = cols; k.faithful = faithful; k.min_obs = min_observations;
  {
    ProfScope ps(c, 4);
    // the objects of the slab do not use the tile: they run with the small one, so that more of them are resident
    if (n_over) hipLaunchKernelGGL(k_init_quadrics<kInitTileSmall>, dim3((unsigned)n_over), dim3(64), 0, c->stream, k, 0);
    if (n_mid > n_over) hipLaunchKernelGGL(k_init_quadrics<kInitTile>, dim3((unsigned)(n_mid - n_over)), dim3(64), 0, c->stream, k, n_over);
    if (N > n_mid) hipLaunchKernelGGL(k_init_quadrics<kInitTileSmall>, dim3((unsigned)(N - n_mid)), dim3(64), 0, c->stream, k, n_mid);
  }
  ESL_HIP_TRY(hipGetLastError());
  ESL_HIP_TRY(hipMemcpyAsync(ellipsoids_out, k.ell, (size_t)N * 10 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (qstar_out) ESL_HIP_TRY(hipMemcpyAsync(qstar_out, k.qstar, (size_t)N * 16 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (plane_error_out) ESL_HIP_TRY(hipMemcpyAsync(plane_error_out, k.perr, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (stats_out) ESL_HIP_TRY(hipMemcpyAsync(stats_out, k.stats, (size_t)N * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's arrays are free again, the outputs filled
  return ESL_OK;
}

// ---- esl_init_quadrics_robust ---------------------------------------------------------------------------------------------------
namespace {

int rob_fail(const char* what, int rc) { set_error(std::string("esl_init_quadrics_robust: ") + what); return rc; }

}  // namespace

extern "C" void esl_init_robust_params_default(esl_init_robust_params* p) {
  if (!p) return;
  p->sample_size = 5; p->n_hypotheses = 64; p->inlier_px = 10.0; p->min_inliers = 8; p->refine = 1; p->seed = 0;
}

extern "C" int esl_init_quadrics_robust(esl_ctx* c, const double* cams, int32_t F, int32_t N, const int32_t* obs_cam, const int32_t* obs_obj,
                                        const double* obs_boxes, int64_t n_obs, const double K[4], int32_t rows, int32_t cols,
                                        int32_t faithful, int32_t min_observations, const esl_init_robust_params* params,
                                        double* ellipsoids_out, double* qstar_out, double* plane_error_out, int32_t* stats_out,
                                        int32_t* inlier_out, double* residual_out, double* hyp_out) {
  if (!c || !K || F < 0 || N < 0 || n_obs < 0 || min_observations < 0) return rob_fail("bad argument (null pointer or negative count)", ESL_ERR_INVALID);
  if (n_obs > INT32_MAX) return rob_fail("more than 2^31 - 1 observations", ESL_ERR_INVALID);
  if (n_obs > 0 && (!obs_cam || !obs_obj || !obs_boxes)) return rob_fail("null observation array", ESL_ERR_INVALID);
  if (N > 0 && !ellipsoids_out) return rob_fail("null ellipsoids_out", ESL_ERR_INVALID);
  if (rows < 1 || cols < 1) return rob_fail("rows or cols < 1", ESL_ERR_INVALID);
  esl_init_robust_params p;
  if (params) p = *params; else esl_init_robust_params_default(&p);
  if (p.sample_size < 3 || p.sample_size > kInitSampleMax) return rob_fail("sample_size outside 3..16", ESL_ERR_INVALID);
  if (p.n_hypotheses < 1 || p.n_hypotheses > 1024) return rob_fail("n_hypotheses outside 1..1024", ESL_ERR_INVALID);
  if (!std::isfinite(p.inlier_px) || !(p.inlier_px > 0)) return rob_fail("inlier_px not finite or not > 0", ESL_ERR_INVALID);
  if (p.min_inliers < 1) return rob_fail("min_inliers < 1", ESL_ERR_INVALID);
  const int H = p.n_hypotheses;
  if ((int64_t)N * H > INT32_MAX) return rob_fail("N * n_hypotheses above 2^31 - 1", ESL_ERR_INVALID);
  if (!cams) {
    if (!c->graph_loaded || !c->states_loaded) return rob_fail("cams == NULL needs a resident graph with states", ESL_ERR_STATE);
    if (F != c->g.n_cams) return rob_fail("F differs from the resident graph's n_cams", ESL_ERR_INVALID);
  }
  if (!c->init_batch) c->init_batch = new InitBatchState();
  InitBatchState* bs = c->init_batch;
  if (!bs->rob) bs->rob = new InitRobustState();
  InitRobustState* s = bs->rob;
  int64_t bad = 0;
  const int grc = init_group(n_obs, N, F, obs_cam, obs_obj, s->offsets, s->idx, &bad);
  if (grc == INIT_GROUP_BAD_OBJ) return rob_fail(("obs_obj >= N at entry " + std::to_string(bad)).c_str(), ESL_ERR_INVALID);
  if (grc == INIT_GROUP_BAD_CAM) return rob_fail(("obs_cam outside [0, F) at entry " + std::to_string(bad)).c_str(), ESL_ERR_INVALID);
  // skipped entries, and those of objects that are not initialised, keep these
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  if (inlier_out) std::fill(inlier_out, inlier_out + n_obs, 0);
  if (residual_out) std::fill(residual_out, residual_out + n_obs, qnan);
  if (N == 0) return ESL_OK;
  s->objs.resize((size_t)N);
  for (int32_t o = 0; o < N; ++o) s->objs[o] = InitObj{o, s->offsets[o], s->offsets[(size_t)o + 1] - s->offsets[o], -1};

  ESL_HIP_TRY(hipSetDevice(c->device));
  typedef InitRobustState R;
  ScratchSet<R::kBufs>& d = s->set;
  InitRobustArgs k{};
  const size_t kept = s->idx.size(), nobs = (size_t)n_obs;
  if (const int rc = source(c, d, R::R_CAMS, cams, c->cams, (size_t)F * 7 * sizeof(double), &k.b.cams)) return rc;
  const size_t want[R::kBufs] = {0, nobs * sizeof(int32_t), nobs * 4 * sizeof(double), kept * sizeof(int32_t), (size_t)N * sizeof(InitObj),
                                 (size_t)N * H * 4 * sizeof(double), (size_t)N * 16 * sizeof(int32_t), (size_t)N * 56 * sizeof(double),
                                 nobs * 2 * sizeof(double), nobs * 2 * sizeof(int32_t), (size_t)N * 10 * sizeof(double), (size_t)N * sizeof(int32_t)};
  for (int b = R::R_OCAM; b < R::kBufs; ++b)
    if (const int rc = d.grow(c, b, want[b])) return rc;
  if (kept) {   // entries that no object keeps are never read
    ESL_HIP_TRY(hipMemcpyAsync(d.buf[R::R_OCAM], obs_cam, nobs * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(d.buf[R::R_BOX], obs_boxes, nobs * 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(d.buf[R::R_IDX], s->idx.data(), kept * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  }
  ESL_HIP_TRY(hipMemcpyAsync(d.buf[R::R_OBJS], s->objs.data(), (size_t)N * sizeof(InitObj), hipMemcpyHostToDevice, c->stream));
  k.b.obs_cam = d.at<const int>(R::R_OCAM); k.b.obs_box = d.at<const double>(R::R_BOX); k.b.idx = d.at<const int>(R::R_IDX);
  for (int i = 0; i < 4; ++i) k.b.K[i] = K[i];
  k.b.rows = rows; k.b.cols = cols; k.b.faithful = faithful; k.b.min_obs = min_observations;
  k.objs = d.at<const InitObj>(R::R_OBJS);
  k.H = H; k.sample_size = p.sample_size; k.min_inliers = p.min_inliers; k.inlier_px = p.inlier_px; k.seed = p.seed;
  k.hyp = d.at<double>(R::R_HYP);
  for (int q = 0; q < 2; ++q) {
    k.oi[q] = d.at<int>(R::R_OI) + (size_t)q * N * 8; k.od[q] = d.at<double>(R::R_OD) + (size_t)q * N * 28;
    k.res_e[q] = d.at<double>(R::R_RES) + (size_t)q * nobs; k.inl_e[q] = d.at<int>(R::R_INL) + (size_t)q * nobs;
  }
  k.rf_ell = d.at<const double>(R::R_RFELL); k.rf_ok = d.at<const int>(R::R_RFOK);
  {
    ProfScope ps(c, 4);
    hipLaunchKernelGGL(k_init_robust, dim3((unsigned)((int64_t)N * H)), dim3(64), 0, c->stream, k, 0);
    hipLaunchKernelGGL(k_init_robust, dim3((unsigned)N), dim3(64), 0, c->stream, k, 1);
  }
  ESL_HIP_TRY(hipGetLastError());
  s->oi.resize((size_t)N * 16); s->od.resize((size_t)N * 56); s->inl.resize(nobs * 2); s->res.resize(nobs * 2);
  ESL_HIP_TRY(hipMemcpyAsync(s->oi.data(), k.oi[0], (size_t)N * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(s->od.data(), k.od[0], (size_t)N * 28 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (kept) {
    ESL_HIP_TRY(hipMemcpyAsync(s->inl.data(), k.inl_e[0], nobs * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(s->res.data(), k.res_e[0], nobs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  if (hyp_out) ESL_HIP_TRY(hipMemcpyAsync(hyp_out, k.hyp, (size_t)N * H * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));

  // refine: esl_init_quadrics itself over the list with everything but the winners' inliers skipped, then pass 2 scores its ellipsoids
  const int32_t* oi1 = s->oi.data();
  const int32_t* oi2 = oi1 + (size_t)N * 8;
  const double* od1 = s->od.data();
  const double* od2 = od1 + (size_t)N * 28;
  bool refit = false;
  if (p.refine)
    for (int32_t o = 0; o < N && !refit; ++o) refit = oi1[(size_t)o * 8] == 0;
  if (refit) {
    s->masked.assign(nobs, -1);
    for (int32_t o = 0; o < N; ++o)
      if (oi1[(size_t)o * 8] == 0)
        for (int32_t j = s->offsets[o]; j < s->offsets[(size_t)o + 1]; ++j)
          if (s->inl[(size_t)s->idx[j]]) s->masked[(size_t)s->idx[j]] = o;
    s->rf_ell.resize((size_t)N * 10); s->rf_qs.resize((size_t)N * 16); s->rf_perr.resize((size_t)N); s->rf_stats.resize((size_t)N * 4);
    s->rf_ok.resize((size_t)N);
    if (const int rc = esl_init_quadrics(c, cams, F, N, obs_cam, s->masked.data(), obs_boxes, n_obs, K, rows, cols, faithful, 0, s->rf_ell.data(),
                                         s->rf_qs.data(), s->rf_perr.data(), s->rf_stats.data()))
      return rc;
    for (int32_t o = 0; o < N; ++o) s->rf_ok[o] = oi1[(size_t)o * 8] == 0 && s->rf_stats[(size_t)o * 4] == 0;
    ESL_HIP_TRY(hipMemcpyAsync(d.buf[R::R_RFELL], s->rf_ell.data(), (size_t)N * 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(d.buf[R::R_RFOK], s->rf_ok.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    {
      ProfScope ps(c, 4);
      hipLaunchKernelGGL(k_init_robust, dim3((unsigned)N), dim3(64), 0, c->stream, k, 2);
    }
    ESL_HIP_TRY(hipGetLastError());
    ESL_HIP_TRY(hipMemcpyAsync(s->oi.data() + (size_t)N * 8, k.oi[1], (size_t)N * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(s->od.data() + (size_t)N * 28, k.od[1], (size_t)N * 28 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (kept) {
      ESL_HIP_TRY(hipMemcpyAsync(s->inl.data() + nobs, k.inl_e[1], nobs * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      ESL_HIP_TRY(hipMemcpyAsync(s->res.data() + nobs, k.res_e[1], nobs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  }

  // per object: the winner's result or the refit's (kept iff valid and its (inliers, cost) is not worse)
  for (int32_t o = 0; o < N; ++o) {
    const int32_t* w = oi1 + (size_t)o * 8;
    const double* wd = od1 + (size_t)o * 28;
    const int status = w[0], n = s->objs[o].n;
    double* ell = ellipsoids_out + (size_t)o * 10;
    int32_t st[8] = {status, n, w[1], 0, 0, w[3], w[4], 0};
    const double* src = nullptr;   // ellipsoid 10 | Q* 16
    double perr = 0;
    int set = 0;                   // whose per-entry results are final
    if (status == 5) st[4] = w[2];
    if (status == 0) {
      src = wd; perr = wd[27]; st[4] = w[2];
      if (refit) {
        st[3] = s->rf_stats[(size_t)o * 4 + 3];
        const int32_t* r = oi2 + (size_t)o * 8;
        const double* rd = od2 + (size_t)o * 28;
        if (s->rf_ok[o] && r[0] && (r[1] > w[2] || (r[1] == w[2] && rd[26] <= wd[26]))) {
          st[7] = 1; st[4] = r[1]; set = 1;
          // the refit's own plane error is over the planes it was given: the final inliers' when the re-score kept the set
          bool same = true;
          for (int32_t j = s->offsets[o]; j < s->offsets[(size_t)o + 1] && same; ++j)
            same = s->inl[(size_t)s->idx[j]] == s->inl[nobs + (size_t)s->idx[j]];
          perr = same ? s->rf_perr[o] : rd[27];
        }
      }
      for (int32_t j = s->offsets[o]; j < s->offsets[(size_t)o + 1]; ++j) {
        const size_t i = (size_t)s->idx[j];
        if (inlier_out) inlier_out[i] = s->inl[(size_t)set * nobs + i];
        if (residual_out) residual_out[i] = s->res[(size_t)set * nobs + i];
      }
    }
    for (int i = 0; i < 10; ++i) ell[i] = src ? (set ? s->rf_ell[(size_t)o * 10 + i] : src[i]) : 0.0;
    if (qstar_out)
      for (int i = 0; i < 16; ++i) qstar_out[(size_t)o * 16 + i] = src ? (set ? s->rf_qs[(size_t)o * 16 + i] : src[10 + i]) : 0.0;
    if (plane_error_out) plane_error_out[o] = perr;
    if (stats_out)
      for (int i = 0; i < 8; ++i) stats_out[(size_t)o * 8 + i] = st[i];
  }
  return ESL_OK;
}
