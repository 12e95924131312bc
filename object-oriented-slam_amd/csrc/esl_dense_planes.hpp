// esl_dense_planes.hpp — the arithmetic of esl_dense_planes (include/esl.h, "dominant planes and the ground from the dense map"; the
// steps' numbers below are the header's): the sampler and the validity of a hypothesis with its plane (step 3), the inlier test (step
// 4), the winner (step 5), the guard, the Jacobi, the refit and its acceptance (step 6), the centroid and the two orientation rules (steps 8
// and 9) and the ground choice (step 9).  Plain C++ for host and device like esl_dense_obj.hpp, no HIP include:
// tests/dense_planes_main.cpp compiles it with an ordinary compiler.  Every translation unit that includes it is built with
// -ffp-contract=off.  What is `inline` only runs on the host: one compiler decides every bit of a plane.  The device uses
// dobj_center / dobj_height (esl_dense_obj.hpp), dpl_inlier, the integer sampler and, for esl_dense_normals, dpl_jacobi_min.
#pragma once
#include <cmath>
#include <cstdint>

#include "esl_dense_obj.hpp"
#include "esl_init_sample.hpp"

namespace esl {

constexpr int kDplMoments = 11;    // n, samples, s_x s_y s_z, M_xx M_xy M_xz M_yy M_yz M_zz of a plane's inliers (relative to kmin)
constexpr int kDplSweeps = 8;      // cyclic Jacobi: sweeps over the pivots (0,1), (0,2), (1,2)

// step 3: entry i_k of hypothesis h of round r in a list of n_r >= 1 entries (integers only: host and device agree)
ESL_DENSE_HD uint64_t dpl_mix(uint64_t seed, int r, int n_hypotheses, int h, int k) {
  return init_sample_finalise(seed, 4ull * ((uint64_t)r * (uint64_t)n_hypotheses + (uint64_t)h) + (uint64_t)k + 1ull);
}
ESL_DENSE_HD int dpl_index(uint64_t seed, int r, int n_hypotheses, int h, int k, int n_r) {
  return (int)((dpl_mix(seed, r, n_hypotheses, h, k) >> 11) % (uint64_t)n_r);
}

// step 4: |h| <= dist_tol
ESL_DENSE_HD bool dpl_inlier(const double pl[4], const double x[3], double dist_tol) {
  return std::fabs(dobj_height(pl, pl[3], x)) <= dist_tol;
}

inline int dpl_cheb(const int a[3], const int b[3]) {
  int m = 0;
  for (int c = 0; c < 3; ++c) {
    const int d = a[c] > b[c] ? a[c] - b[c] : b[c] - a[c];
    if (d > m) m = d;
  }
  return m;
}

// step 3: the plane of the keys a, b, c (entries i[0..2] of U_r) or false for an invalid hypothesis
inline bool dpl_hypothesis(const int i[3], const int a[3], const int b[3], const int c[3], int min_baseline, double leaf, double pl[4]) {
  pl[0] = pl[1] = pl[2] = pl[3] = 0;
  if (i[0] == i[1] || i[0] == i[2] || i[1] == i[2]) return false;
  if (dpl_cheb(a, b) < min_baseline || dpl_cheb(a, c) < min_baseline || dpl_cheb(b, c) < min_baseline) return false;
  const long long u[3] = {(long long)b[0] - a[0], (long long)b[1] - a[1], (long long)b[2] - a[2]};
  const long long v[3] = {(long long)c[0] - a[0], (long long)c[1] - a[1], (long long)c[2] - a[2]};
  const long long N[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};   // |N_a| < 2^44
  const double n0 = (double)N[0], n1 = (double)N[1], n2 = (double)N[2];
  const double norm = std::sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  if (norm < 0.5 * ((double)min_baseline * (double)min_baseline)) return false;
  pl[0] = n0 / norm; pl[1] = n1 / norm; pl[2] = n2 / norm;
  const double x[3] = {dobj_center(a[0], leaf), dobj_center(a[1], leaf), dobj_center(a[2], leaf)};
  pl[3] = -dobj_proj(pl, x);
  return true;
}

// step 5: is (n_in, samples, h) better than the best so far?  Largest n_in, then largest samples, then smallest h.
inline bool dpl_better(long long n_in, long long samples, int h, long long best_n, long long best_s, int best_h) {
  if (n_in != best_n) return n_in > best_n;
  if (samples != best_s) return samples > best_s;
  return h < best_h;
}

// step 5: the winner among the n_hyp hypotheses of a round, or -1 when none is valid; hacc: per hypothesis its inlier voxels and its
// inlier samples.  hyp_out (or null): the round's rows  valid, inlier voxels, inlier samples.
inline int dpl_winner(const int* valid, const unsigned long long* hacc, int n_hyp, int64_t* hyp_out) {
  int win = -1;
  for (int h = 0; h < n_hyp; ++h) {
    if (hyp_out) { hyp_out[3 * h] = valid[h]; hyp_out[3 * h + 1] = (int64_t)hacc[2 * h]; hyp_out[3 * h + 2] = (int64_t)hacc[2 * h + 1]; }
    if (!valid[h]) continue;
    if (win < 0 || dpl_better((long long)hacc[2 * h], (long long)hacc[2 * h + 1], h, (long long)hacc[2 * win], (long long)hacc[2 * win + 1], win))
      win = h;
  }
  return win;
}

// step 6: the refit (n inlier voxels, s samples) is kept when it holds no fewer voxels than the winner, and with as many no fewer samples
inline bool dpl_refit_kept(long long n, long long s, long long win_n, long long win_s) { return n > win_n || (n == win_n && s >= win_s); }

// step 6: the eigenvector of the smallest eigenvalue (ties to the lowest index) of the symmetric C = {c00, c01, c02, c11, c12, c22}
// by a cyclic Jacobi: kDplSweeps sweeps over the pivots (0,1), (0,2), (1,2), only + - * / sqrt; the vector is re-normalised.  Host
// and device: esl_dense_normals runs it per voxel (esl_dense_align.hpp)
ESL_DENSE_HD void dpl_jacobi_min(const double C[6], double n[3]) {
  double a[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
  double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2};
  for (int sweep = 0; sweep < kDplSweeps; ++sweep) {
#if defined(__HIP_DEVICE_COMPILE__)   // constant pivots keep a and v in registers; the host's code is what it was
#pragma unroll
#endif
    for (int e = 0; e < 3; ++e) {
      const int p = P[e], q = Q[e];
      const double apq = a[p][q];
      if (apq == 0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2 * apq);
      double t = 1 / (std::fabs(theta) + std::sqrt(theta * theta + 1));
      if (theta < 0) t = -t;
      const double c = 1 / std::sqrt(t * t + 1), s = t * c;
      for (int k = 0; k < 3; ++k) {   // columns p and q
        const double akp = a[k][p], akq = a[k][q];
        a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq;
      }
      for (int k = 0; k < 3; ++k) {   // rows p and q
        const double apk = a[p][k], aqk = a[q][k];
        a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk;
      }
      for (int k = 0; k < 3; ++k) {
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq;
      }
    }
  }
  double lo = a[0][0], w[3] = {v[0][0], v[1][0], v[2][0]};   // the column of the smallest diagonal entry, the first of equals
  for (int e = 1; e < 3; ++e)
    if (a[e][e] < lo) { lo = a[e][e]; w[0] = v[0][e]; w[1] = v[1][e]; w[2] = v[2][e]; }
  const double nn = std::sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  for (int e = 0; e < 3; ++e) n[e] = w[e] / nn;
}

// steps 6 and 8: the mean centre of a set of voxels from its integer sums relative to kmin (mom[0] = n >= 1, mom[2..4] = s)
inline void dpl_centroid(const long long mom[kDplMoments], const int kmin[3], double leaf, double x[3]) {
  const double dn = (double)mom[0];
  for (int a = 0; a < 3; ++a) x[a] = ((double)kmin[a] + (double)mom[2 + a] / dn + 0.5) * leaf;
}

// step 6: the least-squares plane of the inliers with the moments mom
inline void dpl_refit(const long long mom[kDplMoments], const int kmin[3], double leaf, double pl[4]) {
  const double dn = (double)mom[0];
  const double m[3] = {(double)mom[2] / dn, (double)mom[3] / dn, (double)mom[4] / dn};
  const double C[6] = {(double)mom[5] / dn - m[0] * m[0], (double)mom[6] / dn - m[0] * m[1], (double)mom[7] / dn - m[0] * m[2],
                       (double)mom[8] / dn - m[1] * m[1], (double)mom[9] / dn - m[1] * m[2], (double)mom[10] / dn - m[2] * m[2]};
  dpl_jacobi_min(C, pl);
  double x[3];
  dpl_centroid(mom, kmin, leaf, x);
  pl[3] = -dobj_proj(pl, x);
}

inline void dpl_negate(double pl[4]) { for (int a = 0; a < 4; ++a) pl[a] = -pl[a]; }

// step 8: d^ > 0; with d^ == 0 the first non-zero component of n^ positive
inline void dpl_orient_out(double pl[4]) {
  bool flip = pl[3] < 0;
  if (pl[3] == 0) {
    for (int a = 0; a < 3; ++a) if (pl[a] != 0) { flip = pl[a] < 0; break; }
  }
  if (flip) dpl_negate(pl);
}

// step 9: up^ = up / |up|; false for the zero vector (no ground choice).  The caller has refused non-finite and too short vectors.
inline bool dpl_up(const double up[3], double uh[3]) {
  if (up[0] == 0 && up[1] == 0 && up[2] == 0) return false;
  const double nn = std::sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]);
  for (int a = 0; a < 3; ++a) uh[a] = up[a] / nn;
  return true;
}
inline bool dpl_up_valid(const double up[3]) {
  for (int a = 0; a < 3; ++a) if (!std::isfinite(up[a])) return false;
  if (up[0] == 0 && up[1] == 0 && up[2] == 0) return true;
  const double nn = std::sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]);
  return std::isfinite(nn) && nn > 1e-12;
}

// step 9: the candidate with the most inlier voxels (ties to the lowest index) among the n_planes reported planes (rows of 4; inliers
// in stats[8 p]), or -1; ground = that plane with n^ . up^ > 0
inline int dpl_ground(const double* planes, const int32_t* n_in, int n_planes, const double uh[3], double up_min_cos, double ground[4]) {
  int g = -1;
  for (int p = 0; p < n_planes; ++p) {
    const double dot = dobj_proj(planes + 4 * p, uh);
    if (!(std::fabs(dot) >= up_min_cos)) continue;
    if (g < 0 || n_in[p] > n_in[g]) g = p;
  }
  for (int a = 0; a < 4; ++a) ground[a] = 0;
  if (g >= 0) {
    for (int a = 0; a < 4; ++a) ground[a] = planes[4 * g + a];
    if (dobj_proj(ground, uh) < 0) dpl_negate(ground);
  }
  return g;
}

}  // namespace esl
