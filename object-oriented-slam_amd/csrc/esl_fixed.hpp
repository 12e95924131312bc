// esl_fixed.hpp — fixed ellipsoid vertices (g2o's setFixed on a VertexEllipsoid) and the camera-chain solver.
//
// esl_graph_upload_fixed splits the caller's edges on the host (esl_graph.hip):
//   (a) edges of FREE ellipsoids       -> the ordinary device graph, untouched kernels (a fixed ellipsoid is an ellipsoid without edges)
//   (b) ANCHORED edges                 -> fixed ellipsoid, free camera: camera-only edges, the arrays below, sorted by camera slot
//   (c) INACTIVE edges                 -> fixed ellipsoid, fixed camera (g2o's allVerticesFixed): kept behind (b) for esl_edge_chi2 only
// Kernels of this file (none of them runs for a graph without flags):
//   k_anch_validate     NaN pre-check / visibility test of the anchored bbox edges (as k_bbox_validate)
//   k_anch_linearize    one lane per anchored edge: residual, Jacobian wrt the CAMERA only (6 columns: 12 residual evaluations of a
//                       numeric bbox edge instead of 30), the 27-double camera record A = Jc^T w Jc (21 packed) | g = -Jc^T w r (6) --
//                       the layout of Abb (esl_kernels_slam.hpp store_cam_terms) --, chi2 per edge
//   k_anch_gather       one wave per free camera, after k_slam_cam_gather: its records summed in list order (no floating-point
//                       atomics: bitwise reproducible) into Hcc / b_c, max |diag| and the chi2 of its anchored edges into cam_part
//   k_anch_chi2         one wave per free camera: chi2 of its anchored edges at the trial cameras -> cam_part (k_slam_chi2_all's role)
//   k_anch_edge_chi2    esl_edge_chi2 over anchored and inactive edges
//   k_chain_*           ESL_SOLVER_CAMERA_CHAIN: (Hcc + lambda I + odometry blocks) x_c = b_c, block tridiagonal in free-camera order,
//                       by parallel cyclic reduction over 6 x 6 blocks (below)
#pragma once
#include "esl_kernels_slam.hpp"

namespace esl {

static __global__ void k_anch_validate(DevGraph g, AnchGraph a, const double* __restrict__ cams, const double* __restrict__ objs,
                                       int* __restrict__ n_dropped) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_bb) return;
  const SE3 T = se3_load(cams + 7 * a.bb_cam[i]);
  const Ell e = ell_load(objs + 10 * a.bb_obj[i]);
  double r[4];
  res_box_edge(g.bbox_mode, T, e, g.K, a.bb_meas + 4 * i, r);
  const double c = a.bb_w[i] * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
  const bool bad = (c != c) || (g.check_vis && !bbox_edge_visible(T, e, g.K, g.img_rows, g.img_cols));
  a.bb_valid[i] = bad ? 0 : 1;
  if (bad) atomicAdd(n_dropped, 1);
}

// the camera record of one edge from its D x 6 camera Jacobian: the camera half of store_cam_terms, term for term
template <int D>
__device__ __forceinline__ void store_anch_record(const double* Jc, const double* r, double w, double* __restrict__ rec) {
  int p = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = a; c < 6; ++c) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < D; ++k) s += Jc[k * 6 + a] * w * Jc[k * 6 + c];
      rec[p++] = s;
    }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) s += Jc[k * 6 + a] * (w * r[k]);
    rec[21 + a] = -s;
  }
}

// TYPE 0: bbox edges (reprojection or plane tangency, g.bbox_mode), TYPE 1: 3-D edges (record index n_bb + i)
template <int JAC, int TYPE, bool ROBUST>
static __global__ __launch_bounds__(64) void k_anch_linearize(DevGraph g, AnchGraph a, const double* __restrict__ cams, const double* __restrict__ objs,
                                                              double delta, double* __restrict__ A, double* __restrict__ chi_out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (TYPE == 0) {
    if (i >= a.n_bb) return;
    double* rec = A + (size_t)i * kARec;
    if (!a.bb_valid[i]) {
#pragma unroll
      for (int k = 0; k < kARec; ++k) rec[k] = 0;
      chi_out[i] = 0;
      return;
    }
    const SE3 T = se3_load(cams + 7 * a.bb_cam[i]);
    const Ell e = ell_load(objs + 10 * a.bb_obj[i]);
    const double meas[4] = {a.bb_meas[4 * i], a.bb_meas[4 * i + 1], a.bb_meas[4 * i + 2], a.bb_meas[4 * i + 3]};
    double w = a.bb_w[i], r[4], Jc[24];
    if (JAC == ESL_JAC_ANALYTIC) {
      if (!g.bbox_mode) jac_bbox_t<false, true>(T, e, g.K, meas, r, nullptr, Jc);
      else jac_tangency_t<false, true>(T, e, g.K, meas, r, nullptr, Jc);
    } else {
      res_box_edge(g.bbox_mode, T, e, g.K, meas, r);
      const double scalar = 1.0 / (2 * delta);
#pragma unroll
      for (int k = 0; k < 24; ++k) Jc[k] = 0;
      for (int d = 0; d < 6; ++d) {   // not unrolled (one body, the column placed by a select chain: k_slam_linearize_chunks)
        double u[6], rp[4], rm[4];
#pragma unroll
        for (int q = 0; q < 6; ++q) u[q] = (q == d) ? delta : 0.0;
        res_box_edge(g.bbox_mode, cam_oplus(T, u), e, g.K, meas, rp);
#pragma unroll
        for (int q = 0; q < 6; ++q) u[q] = (q == d) ? -delta : 0.0;
        res_box_edge(g.bbox_mode, cam_oplus(T, u), e, g.K, meas, rm);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
          for (int q = 0; q < 6; ++q) if (q == d) Jc[k * 6 + q] = scalar * (rp[k] - rm[k]);
        }
      }
    }
    double chi = w * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
    robust_edge<ROBUST>(g, ESL_EDGE_BBOX, chi, w);
    store_anch_record<4>(Jc, r, w, rec);
    chi_out[i] = chi;
  } else {
    if (i >= a.n_e3) return;
    const SE3 T = se3_load(cams + 7 * a.e3_cam[i]);
    const Ell e = ell_load(objs + 10 * a.e3_obj[i]);
    const Ell m = ell_load(a.e3_meas + 10 * i);
    double w = a.e3_w[i], r[9], Jcp[36];
    if (JAC == ESL_JAC_ANALYTIC) {   // exp(d) Tcw == right perturbation of E by Ad((Tcw T_est)^-1) d  (jac_e3d)
      double Jp[36], Ad[36];
      E3dHyp h;
      res_e3d(T, e, m, g.yt, r, &h);
      dlog_right_R(h.R, h.t, h.a, Jp);
      se3_adj(se3_inv(se3_mul(T, e.pose)), Ad);
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          double sacc = 0;
#pragma unroll
          for (int k = 0; k < 6; ++k) sacc += Jp[p * 6 + k] * Ad[k * 6 + b];
          Jcp[p * 6 + b] = sacc;
        }
    } else {
      res_e3d_from_E0(e3d_E0(T, e, m), e.s, m.s, g.yt, r);
      const double scalar = 1.0 / (2 * delta);
#pragma unroll
      for (int k = 0; k < 36; ++k) Jcp[k] = 0;
      for (int d = 0; d < 6; ++d) {   // not unrolled
        double u[6], rp[9], rm[9];
#pragma unroll
        for (int q = 0; q < 6; ++q) u[q] = (q == d) ? delta : 0.0;
        res_e3d_from_E0(e3d_E0(cam_oplus(T, u), e, m), e.s, m.s, g.yt, rp);
#pragma unroll
        for (int q = 0; q < 6; ++q) u[q] = (q == d) ? -delta : 0.0;
        res_e3d_from_E0(e3d_E0(cam_oplus(T, u), e, m), e.s, m.s, g.yt, rm);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
#pragma unroll
          for (int q = 0; q < 6; ++q) if (q == d) Jcp[k * 6 + q] = scalar * (rp[k] - rm[k]);
        }
      }
    }
    double cc = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) cc += r[k] * r[k];
    double chi = w * cc;
    robust_edge<ROBUST>(g, ESL_EDGE_E3D, chi, w);
    store_anch_record<6>(Jcp, r, w, A + ((size_t)a.n_bb + i) * kARec);   // (the scale rows do not see the camera)
    chi_out[a.n_bb + i] = chi;
  }
}

// one wave per camera, lane k < 27 = entry k of the record: adds the camera's anchored edges (bbox, then 3-D, list order) to what
// k_slam_cam_gather wrote, and renews the camera's max |diag|; cam_part[0] = chi2 of its anchored edges
static __global__ __launch_bounds__(kWave* kWavesPerBlock) void k_anch_gather(DevGraph g, AnchGraph a, const double* __restrict__ A,
                                                                              const double* __restrict__ chi, double* __restrict__ Hcc,
                                                                              double* __restrict__ bc, double* __restrict__ cam_part) {
  const int lane = threadIdx.x & 63;
  const int cidx = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (cidx >= g.n_cams) return;
  const int slot = g.cam_slot[cidx];
  if (slot < 0) return;
  const int b0 = a.bb_start[slot], b1 = a.bb_start[slot + 1], e0 = a.n_bb + a.e3_start[slot], e1 = a.n_bb + a.e3_start[slot + 1];
  const int k = lane < kARec ? lane : 0;
  double acc = 0, cs = 0;
  for (int q = b0; q < b1; ++q) acc += A[(size_t)q * kARec + k];
  for (int q = e0; q < e1; ++q) acc += A[(size_t)q * kARec + k];
  for (int q = b0 + lane; q < b1; q += 64) cs += chi[q];
  for (int q = e0 + lane; q < e1; q += 64) cs += chi[q];
  cs = wave_sum(cs);
  double v = 0;
  if (lane < 21) {
    int r = 0, base = 0;
    while (lane >= base + (6 - r)) { base += 6 - r; ++r; }
    const int cc = r + (lane - base);
    v = Hcc[(size_t)slot * 36 + r * 6 + cc] + acc;
    Hcc[(size_t)slot * 36 + r * 6 + cc] = v;
    Hcc[(size_t)slot * 36 + cc * 6 + r] = v;
  } else if (lane < 27) {
    bc[(size_t)slot * 6 + (lane - 21)] += acc;
  }
  bool diag = false;
#pragma unroll
  for (int r = 0, q = 0; r < 6; ++r) { if (lane == q) diag = true; q += 6 - r; }
  const double md = wave_max(diag ? fabs(v) : 0.0);
  if (lane == 0) { cam_part[cidx * 4 + 0] = cs; cam_part[cidx * 4 + 1] = md; }
}

// chi2 of the anchored edges at the trial cameras; runs after the camera update, which zeroes cam_part[0]
template <bool ROBUST>
static __global__ __launch_bounds__(kWave* kWavesPerBlock) void k_anch_chi2(DevGraph g, AnchGraph a, const double* __restrict__ cams,
                                                                            const double* __restrict__ objs, double* __restrict__ cam_part) {
  const int lane = threadIdx.x & 63;
  const int cidx = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (cidx >= g.n_cams) return;
  const int slot = g.cam_slot[cidx];
  if (slot < 0) return;
  const SE3 T = se3_load(cams + 7 * cidx);
  double chi = 0;
  for (int i = a.bb_start[slot] + lane; i < a.bb_start[slot + 1]; i += 64) {
    if (!a.bb_valid[i]) continue;
    double r[4];
    res_box_edge(g.bbox_mode, T, ell_load(objs + 10 * a.bb_obj[i]), g.K, a.bb_meas + 4 * i, r);
    double c = a.bb_w[i] * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]), w = 1;
    robust_edge<ROBUST>(g, ESL_EDGE_BBOX, c, w);
    chi += c;
  }
  for (int i = a.e3_start[slot] + lane; i < a.e3_start[slot + 1]; i += 64) {
    double r[9];
    res_e3d(T, ell_load(objs + 10 * a.e3_obj[i]), ell_load(a.e3_meas + 10 * i), g.yt, r);
    double c = 0, w = 1;
#pragma unroll
    for (int k = 0; k < 9; ++k) c += r[k] * r[k];
    c *= a.e3_w[i];
    robust_edge<ROBUST>(g, ESL_EDGE_E3D, c, w);
    chi += c;
  }
  chi = wave_sum(chi);
  if (lane == 0) cam_part[cidx * 4 + 0] = chi;
}

// esl_edge_chi2 over the edges of fixed ellipsoids: raw chi2 and rho1 of the anchored ones, raw chi2 and weight 0 of the inactive
// ones (and of dropped bbox edges); cls = ESL_EDGE_GRAVITY: the raw value of every ellipsoid's prior (the host picks the fixed ones)
static __global__ __launch_bounds__(256) void k_anch_edge_chi2(DevGraph g, AnchGraph a, int cls, const double* __restrict__ cams,
                                                              const double* __restrict__ objs, double* __restrict__ chi_out, double* __restrict__ w_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = cls == ESL_EDGE_BBOX ? a.n_bb_all : cls == ESL_EDGE_E3D ? a.n_e3_all : g.n_objs;
  if (i >= n) return;
  double chi = 0;
  bool live = false;
  if (cls == ESL_EDGE_BBOX) {
    double r[4];
    res_box_edge(g.bbox_mode, se3_load(cams + 7 * a.bb_cam[i]), ell_load(objs + 10 * a.bb_obj[i]), g.K, a.bb_meas + 4 * i, r);
    chi = a.bb_w[i] * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
    live = i < a.n_bb && a.bb_valid[i];
  } else if (cls == ESL_EDGE_E3D) {
    double r[9];
    res_e3d(se3_load(cams + 7 * a.e3_cam[i]), ell_load(objs + 10 * a.e3_obj[i]), ell_load(a.e3_meas + 10 * i), g.yt, r);
    double c = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) c += r[k] * r[k];
    chi = a.e3_w[i] * c;
    live = i < a.n_e3;
  } else {
    const double r = res_grav(ell_load(objs + 10 * i), g.grav_n);
    chi = g.grav_w * r * r;
  }
  double r0, r1;
  robustify(g.rk_kind[cls], g.rk_delta[cls], chi, r0, r1);
  chi_out[i] = chi;
  w_out[i] = live ? r1 : 0.0;
}

// ---- ESL_SOLVER_CAMERA_CHAIN ----------------------------------------------------------------------------------------------
// No active edge joins a free camera to a free ellipsoid, so the camera system stands alone:
//     L_i x_{i-1} + D_i x_i + L_{i+1}^T x_{i+1} = r_i,   D_i = Hcc_i + lambda I,  L_i = A_{i,i-1} (odometry edges of slots i - 1, i)
// Parallel cyclic reduction: step d = 1, 2, 4 ... eliminates x_{i-d} and x_{i+d} from EVERY row with rows i - d and i + d,
//     D_i' = D_i - L_i Dm L_i^T - L_{i+d}^T Dp L_{i+d},   r_i' = r_i - L_i Dm r_{i-d} - L_{i+d}^T Dp r_{i+d},   L_i' = -L_i Dm L_{i-d}
// (Dm, Dp = inverses of D_{i-d}, D_{i+d}; the matrix stays symmetric, so only the lower couplings are kept), after which row i
// couples to i +- 2d.  ceil(log2 nf) steps of nf independent rows each -- never a serial walk over the cameras -- then x_i = D_i^-1 r_i.
// Every D_i of every step is a Schur complement of the positive definite camera matrix: solve_ok = all LDL^T pivots positive.
// Without odometry edges the couplings are zero, no step runs and the blocks are solved independently.
// Per step two launches: k_chain_inv (six lanes per row, one unit vector each through ldlt_solve_packed<6>) and k_chain_step (one
// 64-lane workgroup per row, lane = entry of a 6 x 6 block, operands through 2.1 KB of LDS).  O(nf log nf) 6 x 6 products: 1.4e8
// flop at 10k cameras, no dense matrix.
static __global__ __launch_bounds__(256) void k_chain_init(int nf, const double* __restrict__ Hcc, const double* __restrict__ bc,
                                                           const double* __restrict__ Aod, const int* __restrict__ od_start,
                                                           const int* __restrict__ od_edge, double lambda, double* __restrict__ D,
                                                           double* __restrict__ L, double* __restrict__ rhs) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long i = t / 36;
  if (i >= nf) return;
  const int e = (int)(t - i * 36), r = e / 6, c = e - 6 * r;
  D[t] = Hcc[t] + (r == c ? lambda : 0.0);
  double s = 0;
  if (i > 0)   // A_{i,i-1}: the edges of slot pair (i - 1, i); t = 1: the edge's first vertex is the lower slot (k_cf_gather_B)
    for (int q = od_start[i - 1]; q < od_start[i]; ++q) {
      const int es = od_edge[q];
      const double* Hij = Aod + (size_t)(es >> 1) * 90 + 54;
      s += (es & 1) ? Hij[c * 6 + r] : Hij[r * 6 + c];
    }
  L[t] = s;
  if (e < 6) rhs[i * 6 + e] = bc[i * 6 + e];
}
static __global__ __launch_bounds__(256) void k_chain_inv(int nf, const double* __restrict__ D, double* __restrict__ Dinv, int* __restrict__ info) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long i = t / 6;
  if (i >= nf) return;
  const int col = (int)(t - i * 6);
  double Hp[21], e[6], x[6];
  int p = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) Hp[p++] = D[i * 36 + r * 6 + c];
#pragma unroll
  for (int k = 0; k < 6; ++k) e[k] = (k == col) ? 1.0 : 0.0;
  const bool ok = ldlt_solve_packed<6>(Hp, 0.0, e, x);
#pragma unroll
  for (int k = 0; k < 6; ++k) Dinv[i * 36 + k * 6 + col] = x[k];
  if (!ok && col == 0) atomicOr(info, 1);
}
static __global__ __launch_bounds__(64) void k_chain_step(int nf, int d, const double* __restrict__ D, const double* __restrict__ L,
                                                          const double* __restrict__ rhs, const double* __restrict__ Dinv,
                                                          double* __restrict__ D2, double* __restrict__ L2, double* __restrict__ rhs2) {
  __shared__ double sLi[36], sLp[36], sLm[36], sDm[36], sDp[36], sAl[36], sGa[36], srm[6], srp[6];
  const long i = blockIdx.x;
  const int t = threadIdx.x;
  const bool hm = i - d >= 0, hp = i + d < nf;
  if (t < 36) {
    sLi[t] = hm ? L[i * 36 + t] : 0.0;
    sDm[t] = hm ? Dinv[(i - d) * 36 + t] : 0.0;
    sLm[t] = (hm && i - 2L * d >= 0) ? L[(i - d) * 36 + t] : 0.0;
    sLp[t] = hp ? L[(i + d) * 36 + t] : 0.0;
    sDp[t] = hp ? Dinv[(i + d) * 36 + t] : 0.0;
  } else if (t < 42) {
    srm[t - 36] = hm ? rhs[(i - d) * 6 + (t - 36)] : 0.0;
  } else if (t < 48) {
    srp[t - 42] = hp ? rhs[(i + d) * 6 + (t - 42)] : 0.0;
  }
  __syncthreads();
  const int r = t / 6, c = t - 6 * r;
  if (t < 36) {   // alpha = L_i Dm,  gamma = L_{i+d}^T Dp
    double al = 0, ga = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) { al += sLi[r * 6 + k] * sDm[k * 6 + c]; ga += sLp[k * 6 + r] * sDp[k * 6 + c]; }
    sAl[t] = al; sGa[t] = ga;
  }
  __syncthreads();
  if (t < 36) {
    double dv = D[i * 36 + t], lv = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      dv -= sAl[r * 6 + k] * sLi[c * 6 + k];   // alpha L_i^T
      dv -= sGa[r * 6 + k] * sLp[k * 6 + c];   // gamma L_{i+d}
      lv -= sAl[r * 6 + k] * sLm[k * 6 + c];   // -alpha L_{i-d}
    }
    D2[i * 36 + t] = dv; L2[i * 36 + t] = lv;
  } else if (t < 42) {
    const int q = t - 36;
    double rv = rhs[i * 6 + q];
#pragma unroll
    for (int k = 0; k < 6; ++k) rv -= sAl[q * 6 + k] * srm[k] + sGa[q * 6 + k] * srp[k];
    rhs2[i * 6 + q] = rv;
  }
}
// x_i = D_i^-1 r_i of the fully reduced rows (one lane per camera)
static __global__ __launch_bounds__(64) void k_chain_solve(int nf, const double* __restrict__ D, const double* __restrict__ rhs, double* __restrict__ xc,
                                                           int* __restrict__ info) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= nf) return;
  double Hp[21], b[6], x[6];
  int p = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) Hp[p++] = D[i * 36 + r * 6 + c];
#pragma unroll
  for (int k = 0; k < 6; ++k) b[k] = rhs[i * 6 + k];
  const bool ok = ldlt_solve_packed<6>(Hp, 0.0, b, x);
#pragma unroll
  for (int k = 0; k < 6; ++k) xc[i * 6 + k] = x[k];
  if (!ok) atomicOr(info, 1);
}

}  // namespace esl
