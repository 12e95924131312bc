// esl_pcg.hpp — ESL_SOLVER_PCG: block-Jacobi preconditioned conjugate gradient on the reduced camera system, S never formed.
//
// What g2o ships as LinearSolverPCG (solvers/pcg/linear_solver_pcg.hpp) applied to the Schur complement of block_solver.hpp:367-486:
//     S   = (Hcc + lambda I + odometry blocks) - sum_o W_o D_o^-1 W_o^T ,  D_o = Hoo + lambda I
//     b_s = b_c - sum_o W_o D_o^-1 b_o
// solved for x_c from x_0 = 0 with M = the 6 x 6 diagonal blocks of S; x_o follows through k_slam_backsub.  One product S p is two
// passes over the per-edge W blocks the linearisation already wrote ([54][EU], read in ellipsoid order): O(edges) time and memory.
//
// Launches of one trial:
//   k_pcg_setup_obj   one wave per ellipsoid: Dinv = D_o^-1 (lanes 0..8 one unit vector each), D_o^-1 b_o (lane 9)
//   k_pcg_setup_cam   one wave per free camera: M_c = Hcc_c + lambda I - sum over the runs of its list (sorted by ellipsoid) of
//                     (sum_e W_e) D_o^-1 (sum_e W_e)^T, b_s of the camera, M_c^-1 (lanes 0..5 one unit vector each)
//   k_pcg_update      k = -1: r = b_s, x = 0, z = M^-1 r and the per-workgroup partials of r.z, r.r
//   per iteration k = 0, 1, ...:
//   k_pcg_obj         decides convergence on r_k, derives beta; t_o = D_o^-1 sum_e W_e^T p_cam(e) (lanes over the edges, fixed-order
//                     wave reduction), then the edges' products g_e = W_e t_o ([6][EU]) -- the second pass over W, in the same order
//   k_pcg_cam         one wave per camera: p = z + beta p_old, q = (Hcc + lambda I) p + odometry neighbours - sum_e g_e, partial of p.q
//   k_pcg_update      alpha = r.z / p.q; x += alpha p, r -= alpha q, z = M^-1 r, partials of r.z and r.r
//   k_pcg_finish      after the last iteration: the verdict on r_{max_iters}, the failure flag into the solver's flag word, counters
//
// Determinism: no floating-point atomics.  Every kernel that needs a scalar (p.q, r.z, r.r) re-reduces the short array of
// per-workgroup partials the previous kernel left, all workgroups in the same order (pcg_block_sum: 256 strided sums, then a fixed
// tree), so the value does not depend on which workgroup finished last.  p = fma(beta, p_old, z) is formed by the ONE helper below
// wherever it is needed (k_pcg_obj forms it on the fly: the vector itself is only written by k_pcg_cam, into the other of two buffers).
// alpha, beta, the iteration count and the done flag live in the state block on the device; the host only peeks at the done flag
// every check_every iterations, and launches behind a finished solve return at their first instruction.
#pragma once
#include "esl_kernels_slam.hpp"

namespace esl {

constexpr int kPcgBlock = 256;
// the state block (doubles)
enum { kPcgRz0 = 0, kPcgRz1 = 1, kPcgBb = 2, kPcgBeta = 3, kPcgRr = 4, kPcgIters = 5, kPcgDone = 6, kPcgConv = 7, kPcgFail = 8, kPcgSolves = 9,
       kPcgIterSum = 10, kPcgState = 16 };

// sum of v[0 .. n) by the 256 threads of a workgroup in a fixed order; every thread gets the result
__device__ __forceinline__ double pcg_block_sum(const double* __restrict__ v, int n, double* sh) {
  double a = 0;
  for (int i = threadIdx.x; i < n; i += kPcgBlock) a += v[i];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int s = kPcgBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}
// the search direction of this iteration at one entry
__device__ __forceinline__ double pcg_dir(double beta, double p_old, double z) { return fma(beta, p_old, z); }
__device__ __forceinline__ void pcg_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

static __global__ __launch_bounds__(kWave* kWavesPerBlock) void k_pcg_setup_obj(DevGraph g, double lambda, const double* __restrict__ Hoo,
                                                                                const double* __restrict__ bo, double* __restrict__ Dinv,
                                                                                double* __restrict__ dbo, double* __restrict__ part, int* __restrict__ info) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (o >= g.n_objs) return;
  int ok = 1;
  if (lane < 10) {
    double e[9], x[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = lane < 9 ? ((i == lane) ? 1.0 : 0.0) : bo[(size_t)o * 9 + i];
    ok = ldlt_solve_packed<9>(Hoo + (size_t)o * 45, lambda, e, x) ? 1 : 0;
    if (lane < 9) {
#pragma unroll
      for (int i = 0; i < 9; ++i) Dinv[(size_t)o * 81 + i * 9 + lane] = x[i];
    } else {
#pragma unroll
      for (int i = 0; i < 9; ++i) dbo[(size_t)o * 9 + i] = x[i];
    }
  }
  ok = __all(ok);
  if (lane == 0) {
    part[o * 4 + 3] = (double)ok;
    if (!ok) atomicOr(info, 1);
  }
}

// one wave per camera.  The camera's list is sorted by (ellipsoid, u): a run = its edges at one ellipsoid (a bbox edge and a 3-D
// edge at most, both in one block of S); lane k < 54 sums entry k of the run's W blocks, then Y = Wsum D^-1 (lane k), then lane
// (a, c) < 36 subtracts row a of Y times row c of Wsum and lanes 36..41 the run's share of b_s.
static __global__ __launch_bounds__(kWave* kWavesPerBlock) void k_pcg_setup_cam(DevGraph g, double lambda, const double* __restrict__ Hcc,
                                                                                const double* __restrict__ bc, const double* __restrict__ W,
                                                                                const double* __restrict__ Dinv, const double* __restrict__ dbo,
                                                                                double* __restrict__ M, double* __restrict__ Minv, double* __restrict__ bs,
                                                                                int* __restrict__ info) {
  __shared__ double sW[kWavesPerBlock][54], sY[kWavesPerBlock][54], sD[kWavesPerBlock][81], sdb[kWavesPerBlock][9];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int cidx = blockIdx.x * kWavesPerBlock + wv;
  if (cidx >= g.n_cams) return;
  const int slot = g.cam_slot[cidx];
  if (slot < 0) return;
  const long EU = (long)g.n_bbox + g.n_e3d;
  const int a = lane < 36 ? lane / 6 : lane - 36, cc = lane < 36 ? lane - (lane / 6) * 6 : 0;
  double acc = 0;
  if (lane < 36) acc = Hcc[(size_t)slot * 36 + lane] + ((a == cc) ? lambda : 0.0);
  else if (lane < 42) acc = bc[(size_t)slot * 6 + a];
  int q = g.cu_start[slot];
  const int qe = g.cu_start[slot + 1];
  while (q < qe) {
    const int o = g.cu_obj[q];
    int q1 = q + 1;
    while (q1 < qe && g.cu_obj[q1] == o) ++q1;
    if (lane < 54) {
      double w = 0;
      for (int e = q; e < q1; ++e) {
        const long u = g.cu_id[e];
        if (u < g.n_bbox && !g.bb_valid[u]) continue;
        w += W[(long)lane * EU + u];
      }
      sW[wv][lane] = w;
    }
    for (int k = lane; k < 81; k += 64) sD[wv][k] = Dinv[(size_t)o * 81 + k];
    if (lane < 9) sdb[wv][lane] = dbo[(size_t)o * 9 + lane];
    pcg_wave_sync();
    if (lane < 54) {
      const int ya = lane / 9, yb = lane - ya * 9;
      double s = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j) s += sW[wv][ya * 9 + j] * sD[wv][j * 9 + yb];
      sY[wv][lane] = s;
    }
    pcg_wave_sync();
    if (lane < 36) {
      double s = 0;
#pragma unroll
      for (int b = 0; b < 9; ++b) s += sY[wv][a * 9 + b] * sW[wv][cc * 9 + b];
      acc -= s;
    } else if (lane < 42) {
      double s = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j) s += sW[wv][a * 9 + j] * sdb[wv][j];
      acc -= s;
    }
    pcg_wave_sync();
    q = q1;
  }
  if (lane < 36) { M[(size_t)slot * 36 + lane] = acc; sY[wv][lane] = acc; }
  else if (lane < 42) bs[(size_t)slot * 6 + a] = acc;
  pcg_wave_sync();
  int ok = 1;
  if (lane < 6) {
    double Hp[21], e[6], x[6];
    int p = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c2 = r; c2 < 6; ++c2) Hp[p++] = sY[wv][r * 6 + c2];
#pragma unroll
    for (int k = 0; k < 6; ++k) e[k] = (k == lane) ? 1.0 : 0.0;
    ok = ldlt_solve_packed<6>(Hp, 0.0, e, x) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) Minv[(size_t)slot * 36 + k * 6 + lane] = x[k];
  }
  ok = __all(ok);
  if (lane == 0 && !ok) atomicOr(info, 1);
}

// k = -1: start of the solve.  One thread per free camera (6 unknowns).
static __global__ __launch_bounds__(kPcgBlock) void k_pcg_update(int nf, int k, double* __restrict__ st, const int* __restrict__ info,
                                                                 const double* __restrict__ pq_part, int n_pq, const double* __restrict__ Minv,
                                                                 const double* __restrict__ bs, const double* __restrict__ p, const double* __restrict__ qv,
                                                                 double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                                 double* __restrict__ rz_part, double* __restrict__ rr_part, int nb) {
  __shared__ double sh[kPcgBlock];
  const int s = blockIdx.x * kPcgBlock + threadIdx.x;
  double rv[6] = {0, 0, 0, 0, 0, 0};
  if (k < 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && (info[0] & 1)) { st[kPcgDone] = 1; st[kPcgFail] = 1; }   // a non-positive pivot in the setup
    if (s < nf) {
#pragma unroll
      for (int a = 0; a < 6; ++a) { rv[a] = bs[(size_t)s * 6 + a]; x[(size_t)s * 6 + a] = 0; }
    }
  } else {
    if (st[kPcgDone] != 0) return;
    const double pq = pcg_block_sum(pq_part, n_pq, sh);
    if (!(pq > 0)) {   // breakdown (S not positive definite along p): the solve has failed
      if (blockIdx.x == 0 && threadIdx.x == 0) { st[kPcgDone] = 1; st[kPcgFail] = 1; st[kPcgIters] = k; }
      return;
    }
    const double alpha = st[k & 1] / pq;
    if (s < nf) {
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        x[(size_t)s * 6 + a] = fma(alpha, p[(size_t)s * 6 + a], x[(size_t)s * 6 + a]);
        rv[a] = fma(-alpha, qv[(size_t)s * 6 + a], r[(size_t)s * 6 + a]);
      }
    }
  }
  double rz = 0, rr = 0;
  if (s < nf) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double zs = 0;
#pragma unroll
      for (int c = 0; c < 6; ++c) zs += Minv[(size_t)s * 36 + a * 6 + c] * rv[c];
      r[(size_t)s * 6 + a] = rv[a];
      z[(size_t)s * 6 + a] = zs;
      rz += rv[a] * zs;
      rr += rv[a] * rv[a];
    }
  }
  const int par = (k + 1) & 1;
  sh[threadIdx.x] = rz;
  __syncthreads();
  for (int t = kPcgBlock / 2; t > 0; t >>= 1) { if ((int)threadIdx.x < t) sh[threadIdx.x] += sh[threadIdx.x + t]; __syncthreads(); }
  if (threadIdx.x == 0) rz_part[par * nb + blockIdx.x] = sh[0];
  __syncthreads();
  sh[threadIdx.x] = rr;
  __syncthreads();
  for (int t = kPcgBlock / 2; t > 0; t >>= 1) { if ((int)threadIdx.x < t) sh[threadIdx.x] += sh[threadIdx.x + t]; __syncthreads(); }
  if (threadIdx.x == 0) rr_part[par * nb + blockIdx.x] = sh[0];
}

// iteration k, ellipsoid side.  Every workgroup re-derives r_k.z_k and |r_k|^2 from the partials; workgroup 0 records them.
static __global__ __launch_bounds__(kWave* kWavesPerBlock) void k_pcg_obj(DevGraph g, int k, double tol2, double* __restrict__ st,
                                                                          const double* __restrict__ rz_part, const double* __restrict__ rr_part, int nb,
                                                                          const double* __restrict__ W, const double* __restrict__ Dinv,
                                                                          const double* __restrict__ z, const double* __restrict__ p_old,
                                                                          double* __restrict__ E) {
  __shared__ double sh[kPcgBlock];
  if (st[kPcgDone] != 0) return;
  const double rz = pcg_block_sum(rz_part + (k & 1) * nb, nb, sh);
  const double rr = pcg_block_sum(rr_part + (k & 1) * nb, nb, sh);
  const double bb = k == 0 ? rr : st[kPcgBb];
  const bool conv = rr <= tol2 * bb;
  const double beta = k == 0 ? 0.0 : rz / st[(k - 1) & 1];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st[k & 1] = rz; st[kPcgBeta] = beta; st[kPcgRr] = rr;
    if (k == 0) st[kPcgBb] = rr;
    if (conv) { st[kPcgDone] = 1; st[kPcgConv] = 1; st[kPcgIters] = k; }
  }
  if (conv) return;
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (o >= g.n_objs) return;
  const int q0 = g.ue_start[o], q1 = g.ue_start[o + 1];
  if (q0 == q1) return;
  const long EU = (long)g.n_bbox + g.n_e3d;
  double t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int q = q0 + lane; q < q1; q += 64) {
    const long u = g.ue_id[q];
    if (u < g.n_bbox && !g.bb_valid[u]) continue;
    const int slot = g.ue_slot[q];
    double p6[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) p6[a] = pcg_dir(beta, p_old[(size_t)slot * 6 + a], z[(size_t)slot * 6 + a]);
#pragma unroll
    for (int b = 0; b < 9; ++b) {
      double s = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) s += W[(long)(a * 9 + b) * EU + u] * p6[a];
      t[b] += s;
    }
  }
#pragma unroll
  for (int b = 0; b < 9; ++b) t[b] = wave_sum(t[b]);
#pragma unroll
  for (int b = 0; b < 9; ++b) t[b] = __shfl(t[b], 0, 64);
  double to[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    double s = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) s += Dinv[(size_t)o * 81 + i * 9 + j] * t[j];
    to[i] = s;
  }
  for (int q = q0 + lane; q < q1; q += 64) {
    const long u = g.ue_id[q];
    if (u < g.n_bbox && !g.bb_valid[u]) continue;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double s = 0;
#pragma unroll
      for (int b = 0; b < 9; ++b) s += W[(long)(a * 9 + b) * EU + u] * to[b];
      E[(long)a * EU + u] = s;
    }
  }
}

// iteration k, camera side: one wave per camera, lane a < 6 = row a of the camera's block row
static __global__ __launch_bounds__(kWave* kWavesPerBlock) void k_pcg_cam(DevGraph g, int k, double lambda, const double* __restrict__ st,
                                                                          const double* __restrict__ Hcc, const double* __restrict__ Aod,
                                                                          const double* __restrict__ E, const double* __restrict__ z,
                                                                          const double* __restrict__ p_old, double* __restrict__ p_new,
                                                                          double* __restrict__ qv, double* __restrict__ pq_part) {
  __shared__ double spq[kWavesPerBlock];
  if (st[kPcgDone] != 0) return;
  const double beta = st[kPcgBeta];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int cidx = blockIdx.x * kWavesPerBlock + wv;
  const int slot = cidx < g.n_cams ? g.cam_slot[cidx] : -1;
  double pq = 0;
  if (slot >= 0) {
    const long EU = (long)g.n_bbox + g.n_e3d;
    const int a = lane < 6 ? lane : 0;
    const double pa = pcg_dir(beta, p_old[(size_t)slot * 6 + a], z[(size_t)slot * 6 + a]);
    double p6[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) p6[c] = __shfl(pa, c, 64);
    double qa = lambda * pa;
#pragma unroll
    for (int c = 0; c < 6; ++c) qa += Hcc[(size_t)slot * 36 + a * 6 + c] * p6[c];
    for (int qi = g.cod_start[cidx]; qi < g.cod_start[cidx + 1]; ++qi) {
      const int es = g.cod_edge[qi], e = es >> 1;
      const int so = g.cam_slot[(es & 1) ? g.od_i[e] : g.od_j[e]];
      if (so < 0 || so == slot) continue;
      const double* Hij = Aod + (size_t)e * 90 + 54;   // rows = first vertex, columns = second vertex
      double s = 0;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double po = pcg_dir(beta, p_old[(size_t)so * 6 + c], z[(size_t)so * 6 + c]);
        s += ((es & 1) ? Hij[c * 6 + a] : Hij[a * 6 + c]) * po;
      }
      qa += s;
    }
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int qi = g.cu_start[slot] + lane; qi < g.cu_start[slot + 1]; qi += 64) {
      const long u = g.cu_id[qi];
      if (u < g.n_bbox && !g.bb_valid[u]) continue;
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[c] += E[(long)c * EU + u];
    }
    double mine = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double v = __shfl(wave_sum(acc[c]), 0, 64);
      if (c == a) mine = v;
    }
    qa -= mine;
    if (lane < 6) { qv[(size_t)slot * 6 + lane] = qa; p_new[(size_t)slot * 6 + lane] = pa; }
    const double prod = pa * qa;
#pragma unroll
    for (int c = 0; c < 6; ++c) pq += __shfl(prod, c, 64);
  }
  if (lane == 0) spq[wv] = pq;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) s += spq[w];
    pq_part[blockIdx.x] = s;
  }
}

// after the last launched iteration (k_end of them): if no kernel has closed the solve, r_{k_end} gets its verdict here; a solve
// that did not converge raises bit 0 of the solver's flag word (k_slam_reduce_all folds it into the "ok" partial)
static __global__ __launch_bounds__(kPcgBlock) void k_pcg_finish(int k_end, double tol2, double* __restrict__ st, const double* __restrict__ rr_part, int nb,
                                                                 int* __restrict__ info, int reset_counters) {
  __shared__ double sh[kPcgBlock];
  const bool open = st[kPcgDone] == 0;
  __syncthreads();
  if (open) {
    const double rr = pcg_block_sum(rr_part + (k_end & 1) * nb, nb, sh);
    if (threadIdx.x == 0) {
      const double bb = k_end == 0 ? rr : st[kPcgBb];
      st[kPcgRr] = rr;
      if (k_end == 0) st[kPcgBb] = rr;
      st[kPcgIters] = k_end; st[kPcgConv] = (rr <= tol2 * bb) ? 1 : 0; st[kPcgDone] = 1;
    }
  }
  if (threadIdx.x == 0) {
    if (st[kPcgConv] == 0) info[0] |= 1;
    const double s0 = reset_counters ? 0.0 : st[kPcgSolves], s1 = reset_counters ? 0.0 : st[kPcgIterSum];
    st[kPcgSolves] = s0 + 1; st[kPcgIterSum] = s1 + st[kPcgIters];
  }
}

}  // namespace esl
