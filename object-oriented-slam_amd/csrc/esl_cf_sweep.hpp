// esl_cf_sweep.hpp — form 3 of the camera-first elimination (esl_cf.hpp, "one-sided assembly") without the interior slab Xc.
//
// The assembly reads V and Y = L_ii^T (G_p^-1 W) only.  The parent's route to Y writes x = L_p^-1 W for every interior slot
// (k_cf_forward<2>), reads it back for the segment's backward sweep (k_cf_seg_back) and a third time for z = y - X x_o
// (k_cf_z_sparse): the backward sweep needs x at every slot, and a lane's column (6 (stride - 1) doubles) does not fit registers.
// A block-tridiagonal positive definite G_p can instead be solved from both ends with six doubles of state per direction (a
// "twisted" factorisation: forward pivots from the first slot, backward pivots from the last, combined at every slot).  In the
// library's scaling (V_i = L_ii^-1 w_i; tests/cf_twisted_ref.py has the derivation and the numpy statement):
//     forward     x_i = V_i - M_i x_{i-1}                      (k_cf_forward's recurrence, operation for operation)
//     backward    u_i = V_i - Q_i u_{i+1}                      Q_i = H_i^T K_{i+1}^-1 L_{i+1,i+1},  H_i = K_{i+1}^-1 G_i^T,  K_i = chol(D-_i),
//                                                              D-_i = A_i - L_ii H_i^T H_i L_ii^T the pivots of the elimination from the last slot
//     combine     Y_i = P_i (x_i + u_i - V_i)                  P_i = (I - H_i^T H_i)^-1: the twisted pivot D+_i + D-_i - A_i = L_ii P_i^-1 L_ii^T
// with Q = 0 and P = I at the last interior slot.  P and Q depend on the trial's lambda, not on the column: k_cf_twist, one wave per
// segment, stride - 1 serial steps.  x_i is zero in front of a column's first entry, u_i behind its last one and u_i = V_i exactly
// AT the last one, so one lane per column (k_cf_sweep, k_cf_forward<2>'s work list)
//     runs forward and stores P_i x_i from its first entry on        (final behind the last entry),
//     runs backward and stores P_i u_i in front of its first entry   (final),
//     and adds P_i (u_i - V_i) to its own earlier store between its first and its last entry only (most columns have one entry in
//     a segment: no such slot).
// The forward pass keeps the separator sums acc = sum Zt_j^T x_j (into R) and the six rows of the last interior slot (into a thin
// buffer XL, read by k_cf_sep_rhs in place of the slab) with their operation order: Xs, the rank-K update and the separators'
// chain have the parent's bits.  z of the interior rows: X_I x_o = L_II^-1 (W_I x_o), so k_cf_wxo forms d_i = vy_i - sum over the
// entries at slot i of V_k x_o(k) (a by-slot index of the entry lists, fixed order, no atomics) and k_cf_z_fwd runs the segment's
// forward recurrence on that one vector.
// ESL_CF_SWEEP=0 (read when the context is created) keeps the parent's kernels and bits.
#pragma once
#include "esl_cf.hpp"

namespace esl {

constexpr int kCfSweepSI = 3 * kCfFwdCh - 1;   // interior slots of the longest segment of form 3

#define CF_LT(r, c) ((r) * ((r) + 1) / 2 + (c))
// in-place Cholesky of a packed lower 6 x 6 (k_cf_chain's: hardware 1 / sqrt + two Newton steps); is[] = 1 / diagonal
__device__ __forceinline__ void cf_chol6(double (&d)[21], double (&is)[6], bool& ok) {
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double p = d[CF_LT(j, j)];
    ok = ok && (p > 0);
    double q = __builtin_amdgcn_rsq(p);
    q = q * (1.5 - 0.5 * p * q * q);
    q = q * (1.5 - 0.5 * p * q * q);
    is[j] = q;
    d[CF_LT(j, j)] = p * q;
#pragma unroll
    for (int r = j + 1; r < 6; ++r) d[CF_LT(r, j)] *= q;
#pragma unroll
    for (int r = j + 1; r < 6; ++r)
#pragma unroll
      for (int c = j + 1; c <= r; ++c) d[CF_LT(r, c)] -= d[CF_LT(r, j)] * d[CF_LT(c, j)];
  }
}

// ---- P_i and Q_i of every interior slot: workgroup p = segment p, one wave, serial from the last interior slot down ----------------
// Every lane carries the whole 6 x 6 problem (k_cf_chain's form); the segment's Hcc, G and L_ii are staged in LDS in front of the loop
// and P_i / Q_i take the place of Hcc_i / G_i there (each is read for the last time in the step that writes over it), leaving as
// coalesced stores.  A pivot that is not positive (never, where the forward chain's were) marks the trial like k_cf_chain's.
static __global__ __launch_bounds__(64) void k_cf_twist(int nf_all, int stride, const double* __restrict__ Hcc, double lambda,
                                                        const double* __restrict__ Lfac, const double* __restrict__ Gfac,
                                                        double* __restrict__ Pm, double* __restrict__ Qm, int* __restrict__ info) {
  __shared__ double sH[kCfSweepSI * 36], sG[kCfSweepSI * 36], sL[kCfSweepSI * 21];
  const int lane = threadIdx.x;
  const int beg = (int)blockIdx.x * stride;
  const int len = ((beg + stride - 1 < nf_all) ? beg + stride - 1 : nf_all) - beg;
  if (len <= 0) return;
  {   // fixed trip counts, clamped addresses: the loads go out together
    constexpr int kQ = (kCfSweepSI * 36 + 63) / 64, kL = (kCfSweepSI * 21 + 63) / 64;
    double th[kQ], tg[kQ], tl[kL];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const int idx = q * 64 + lane, cl = idx < len * 36 ? idx : 0;
      th[q] = Hcc[(size_t)beg * 36 + cl]; tg[q] = Gfac[(size_t)beg * 36 + cl];
    }
#pragma unroll
    for (int q = 0; q < kL; ++q) { const int idx = q * 64 + lane; tl[q] = Lfac[(size_t)beg * 21 + (idx < len * 21 ? idx : 0)]; }
#pragma unroll
    for (int q = 0; q < kQ; ++q) if (q * 64 + lane < kCfSweepSI * 36) { sH[q * 64 + lane] = th[q]; sG[q * 64 + lane] = tg[q]; }
#pragma unroll
    for (int q = 0; q < kL; ++q) if (q * 64 + lane < kCfSweepSI * 21) sL[q * 64 + lane] = tl[q];
  }
  __builtin_amdgcn_wave_barrier();
  bool ok = true;
  double K[21], isk[6];   // chol(D-_{i+1}) and the reciprocals of its diagonal
#pragma unroll
  for (int k = 0; k < 21; ++k) K[k] = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) isk[k] = 0;
  for (int i = len - 1; i >= 0; --i) {
    double dm[21], P[36], Q[36];
    if (i == len - 1) {   // nothing behind the last interior slot (its coupling to the separator is not part of G_p)
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) { P[r * 6 + c] = r == c ? 1.0 : 0.0; Q[r * 6 + c] = 0.0; }
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) dm[CF_LT(r, c)] = sH[i * 36 + r * 6 + c] + ((r == c) ? lambda : 0.0);
    } else {
      double g[36], h[36], L[21], Ln[21];
#pragma unroll
      for (int k = 0; k < 36; ++k) g[k] = sG[i * 36 + k];
#pragma unroll
      for (int k = 0; k < 21; ++k) { L[k] = sL[i * 21 + k]; Ln[k] = sL[(i + 1) * 21 + k]; }
      // H = K^-1 G^T: column c solves K h = (row c of G)^T
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double v = g[c * 6 + r];
#pragma unroll
          for (int k = 0; k < r; ++k) v -= K[CF_LT(r, k)] * h[k * 6 + c];
          h[r * 6 + c] = v * isk[r];
        }
      // S = H^T H (symmetric)
      double S[36];
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
          double v = 0;
#pragma unroll
          for (int r = 0; r < 6; ++r) v += h[r * 6 + a] * h[r * 6 + b];
          S[a * 6 + b] = v; S[b * 6 + a] = v;
        }
      // P = (I - S)^-1 through its Cholesky factor C: P = C^-T C^-1
      double C[21], ic[6], Ci[36];
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) C[CF_LT(a, b)] = ((a == b) ? 1.0 : 0.0) - S[a * 6 + b];
      cf_chol6(C, ic, ok);
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          if (r < c) { Ci[r * 6 + c] = 0; continue; }
          double v = (r == c) ? 1.0 : 0.0;
#pragma unroll
          for (int k = c; k < r; ++k) v -= C[CF_LT(r, k)] * Ci[k * 6 + c];
          Ci[r * 6 + c] = v * ic[r];
        }
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
          double v = 0;
#pragma unroll
          for (int k = a; k < 6; ++k) v += Ci[k * 6 + a] * Ci[k * 6 + b];
          P[a * 6 + b] = v; P[b * 6 + a] = v;
        }
      // Q = H^T (K^-1 L_{i+1,i+1}): both factors lower triangular, so is K^-1 L
      double t1[36];
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          if (r < c) { t1[r * 6 + c] = 0; continue; }
          double v = Ln[CF_LT(r, c)];
#pragma unroll
          for (int k = c; k < r; ++k) v -= K[CF_LT(r, k)] * t1[k * 6 + c];
          t1[r * 6 + c] = v * isk[r];
        }
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          double v = 0;
#pragma unroll
          for (int r = b; r < 6; ++r) v += h[r * 6 + a] * t1[r * 6 + b];
          Q[a * 6 + b] = v;
        }
      // D-_i = A_i - L S L^T
      double U[36];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          double v = 0;
#pragma unroll
          for (int k = 0; k <= r; ++k) v += L[CF_LT(r, k)] * S[k * 6 + c];
          U[r * 6 + c] = v;
        }
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
          double v = sH[i * 36 + r * 6 + c] + ((r == c) ? lambda : 0.0);
#pragma unroll
          for (int k = 0; k <= c; ++k) v -= U[r * 6 + k] * L[CF_LT(c, k)];
          dm[CF_LT(r, c)] = v;
        }
    }
    cf_chol6(dm, isk, ok);
#pragma unroll
    for (int k = 0; k < 21; ++k) K[k] = dm[k];
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 36; ++k) { sH[i * 36 + k] = P[k]; sG[i * 36 + k] = Q[k]; }
    }
  }
  __builtin_amdgcn_wave_barrier();
  for (int idx = lane; idx < len * 36; idx += 64) { Pm[(size_t)beg * 36 + idx] = sH[idx]; Qm[(size_t)beg * 36 + idx] = sG[idx]; }
  if (!ok && lane == 0) atomicOr(info, 1);
}
#undef CF_LT

// ---- Y in one sweep per segment: workgroup = entry of k_cf_forward<2>'s work list (segment, 64 compact columns), lane = column ------
// Both passes keep k_cf_forward<2>'s shape, so that no global load sits inside a serial loop: per chunk of kCfFwdCh slots the
// wave-uniform matrices through LDS, per PART of a chunk (kCfFwdCh / PARTS slots; the LDS per one-wave workgroup sets the waves in
// flight) the lane's V records added into its LDS column in list order, the part's steps on LDS only, the part's stores straight-line
// in batches of eight.  A part in which no lane of the wave has anything to do -- forward: in front of every lane's first entry,
// backward: behind every lane's last one -- is left out (x and u are exact zeros there).  The read-modify-write batch runs only in a
// part where some lane has a slot between its first and last entry.
// XL: the last interior slot's rows of x, segment p at 6 (xoff[p] / xl_rows) + row xld[p] + column (xl_rows = rows of a slab in xoff).
template <int PARTS>
static __global__ __launch_bounds__(64) void k_cf_sweep(int nf_all, int n_o, int n_chunks, const int* __restrict__ oe_cst, const int* __restrict__ oe_slot,
                                                        const double* __restrict__ V, const double* __restrict__ vy, const double* __restrict__ Mm,
                                                        const double* __restrict__ Zt, const double* __restrict__ Pm, const double* __restrict__ Qm,
                                                        double* __restrict__ R, long ldx, int stride, CfSegs sg, double* __restrict__ Y,
                                                        double* __restrict__ Yr, double* __restrict__ XL, long long xl_rows) {
  static_assert(PARTS == 2 || PARTS == 4 || PARTS == 8, "halves, quarters or eighths of a chunk");
  constexpr int CH = kCfFwdCh / PARTS;
  constexpr int kQ = kCfFwdCh * 36 / 64;
  __shared__ double sA[kCfFwdCh * 36], sB[kCfFwdCh * 36], sP[kCfFwdCh * 36];   // forward: M, Zt, P; backward: Q, -, P
  __shared__ double sv[CH * 6 * 64];
  __shared__ double svy[kCfFwdCh * 6];
  const int lane = threadIdx.x;
  const int seg = sg.fwork[2 * blockIdx.x];
  const int j = sg.fwork[2 * blockIdx.x + 1] * 64 + lane;
  const int ob = sg.seg_start[seg];
  const int jr = 9 * (sg.seg_start[seg + 1] - ob);   // the right-hand side's column
  const bool on = j <= jr, rhs = j == jr, col = on && !rhs;
  const int oi = col ? j / 9 : 0, b = j - 9 * oi;
  const int o = col ? sg.seg_obj[ob + oi] : 0;
  const long tcol = rhs ? (long)n_o : 9L * (sg.rank ? sg.rank[o] : o) + b;   // this lane's column of R
  const int SI = stride - 1;
  const int beg = seg * stride;
  const int nf = (beg + SI < nf_all) ? beg + SI : nf_all;
  if (beg >= nf) return;
  const int len = nf - beg;
  const bool use_z = Zt != nullptr && seg >= 1;
  const int* cst = oe_cst + (size_t)o * (n_chunks + 1);
  // the lane's first and last entry among the segment's interior slots (the separator's entries end the segment's range)
  // A column with at most kE entries in the segment (C4: 1.5 on average) holds them in registers, and where every column of the wave
  // does (`fast`, wave-uniform) no part of either pass walks the list in memory: the only global loads left in the loops are the
  // chunks' matrices.  Same entries, same order, same sums as the walk.
  constexpr int kE = 4;
  int s_first = len, s_last = -1, ecnt = 0;
  int eslot[kE];
  double erec[kE][6];
#pragma unroll
  for (int e = 0; e < kE; ++e) {
    eslot[e] = -1;
#pragma unroll
    for (int a = 0; a < 6; ++a) erec[e][a] = 0.0;
  }
  if (rhs) { s_first = 0; s_last = len - 1; }
  else if (col) {
    const int c0 = beg / kCfFwdCh, c1 = (c0 + stride / kCfFwdCh < n_chunks) ? c0 + stride / kCfFwdCh : n_chunks;
    const int ka = cst[c0], kb = cst[c1];
    if (ka < kb) {
      const int f = oe_slot[ka] - beg;
      int k = kb - 1, l = oe_slot[k] - beg;
      while (l >= len && k > ka) { --k; l = oe_slot[k] - beg; }
      if (f < len) {
        s_first = f; s_last = l; ecnt = k - ka + 1;
#pragma unroll
        for (int e = 0; e < kE; ++e) {
          const int kk = e < ecnt ? ka + e : ka;
          eslot[e] = oe_slot[kk] - beg;
          const double* src = V + ((size_t)kk * 9 + b) * 6;
#pragma unroll
          for (int a = 0; a < 6; ++a) erec[e][a] = src[a];
        }
      }
    }
  }
  const bool fast = !__any(ecnt > kE);
  double* dst = rhs ? Yr + (size_t)beg * 6 : Y + ((size_t)(ob + oi) * SI) * 54 + b * 6;
  const int dstep = rhs ? 6 : 54;
  // the lane's V records of the slots [p0, p0 + hl) of the segment, added into its LDS column in list order (chunk ch's entry range)
  auto gather = [&](int ch, int h0, int p0, int hl) {
#pragma unroll
    for (int q = 0; q < CH * 6; ++q) sv[q * 64 + lane] = 0.0;
    __builtin_amdgcn_wave_barrier();
    if (rhs) {
#pragma unroll
      for (int q = 0; q < CH * 6; ++q) sv[q * 64 + lane] = (q < hl * 6) ? svy[h0 * 6 + q] : 0.0;
    } else if (col && fast) {
#pragma unroll
      for (int e = 0; e < kE; ++e) {
        const int at = eslot[e] - p0;
        if (e < ecnt && at >= 0 && at < hl) {
#pragma unroll
          for (int a = 0; a < 6; ++a) sv[(at * 6 + a) * 64 + lane] += erec[e][a];
        }
      }
    } else if (col) {
      const int ka = cst[ch], kb = cst[ch + 1];
      for (int k = ka; k < kb; k += 4) {   // batches of four entries: slots and records of a batch in flight together
        int sl[4];
        double rec[4][6];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int kk = (k + e < kb) ? k + e : ka;
          sl[e] = oe_slot[kk];
          const double* src = V + ((size_t)kk * 9 + b) * 6;
#pragma unroll
          for (int a = 0; a < 6; ++a) rec[e][a] = src[a];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int at = sl[e] - beg - p0;
          if (k + e < kb && at >= 0 && at < hl) {   // (slots behind the segment's end in this chunk: the separator's entries)
#pragma unroll
            for (int a = 0; a < 6; ++a) sv[(at * 6 + a) * 64 + lane] += rec[e][a];
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  };
  // ---- forward: x_i = V_i - M_i x_{i-1}, the separator sums, P_i x_i stored from the first entry on ----
  double x[6] = {0, 0, 0, 0, 0, 0}, acc[6] = {0, 0, 0, 0, 0, 0};
  for (int i0 = beg; i0 < nf; i0 += kCfFwdCh) {
    const int ch = i0 / kCfFwdCh;
    const int clen = (nf - i0 < kCfFwdCh) ? nf - i0 : kCfFwdCh;
    if (!__any(on && s_first < i0 - beg + clen)) continue;
    __builtin_amdgcn_wave_barrier();
    {
      double tm[kQ], tz[kQ], tp[kQ], ty[2];
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        const int idx = q * 64 + lane, cl = idx < clen * 36 ? idx : 0;
        tm[q] = Mm[(size_t)i0 * 36 + cl];
        tz[q] = use_z ? Zt[(size_t)i0 * 36 + cl] : 0.0;
        tp[q] = Pm[(size_t)i0 * 36 + cl];
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) { const int idx = q * 64 + lane; ty[q] = vy[(size_t)i0 * 6 + (idx < clen * 6 ? idx : 0)]; }
#pragma unroll
      for (int q = 0; q < kQ; ++q) { sA[q * 64 + lane] = tm[q]; sB[q * 64 + lane] = tz[q]; sP[q * 64 + lane] = tp[q]; }
#pragma unroll
      for (int q = 0; q < 2; ++q) if (q * 64 + lane < kCfFwdCh * 6) svy[q * 64 + lane] = ty[q];
    }
    __builtin_amdgcn_wave_barrier();
    for (int h0 = 0; h0 < clen; h0 += CH) {
      const int hl = (clen - h0 < CH) ? clen - h0 : CH;
      const int p0 = i0 - beg + h0;   // the part's first slot of the segment
      if (!__any(on && s_first < p0 + hl)) continue;
      gather(ch, h0, p0, hl);
      for (int ii = 0; ii < hl; ++ii) {
        const double* M = sA + (h0 + ii) * 36;
        double xn[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double t = sv[(ii * 6 + a) * 64 + lane];
#pragma unroll
          for (int q = 0; q < 6; ++q) t -= M[a * 6 + q] * x[q];
          xn[a] = t;
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) x[a] = xn[a];
        if (use_z) {
          const double* Z = sB + (h0 + ii) * 36;
#pragma unroll
          for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[a] += Z[q * 6 + a] * xn[q];
        }
        const double* P = sP + (h0 + ii) * 36;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double t = 0;
#pragma unroll
          for (int q = 0; q < 6; ++q) t += P[a * 6 + q] * xn[q];
          sv[(ii * 6 + a) * 64 + lane] = t;
        }
      }
      // out: batches of eight LDS reads, then their stores; straight-line (a run-time loop waits for the last batch's stores at its head)
      if (on) {
#pragma unroll
        for (int q0 = 0; q0 < CH * 6; q0 += 8) {
          double t[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) t[e] = sv[((q0 + e < hl * 6) ? q0 + e : 0) * 64 + lane];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int q = q0 + e, pos = p0 + q / 6;
            if (q < hl * 6 && pos >= s_first) dst[(size_t)pos * dstep + q % 6] = t[e];
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (use_z && on) {
#pragma unroll
    for (int a = 0; a < 6; ++a) R[(size_t)tcol + (size_t)(6 * (seg - 1) + a) * (size_t)ldx] = acc[a];
  }
  if (on && len == SI) {   // a separator follows: x of the last interior slot, k_cf_sep_rhs's
    double* xl = XL + (size_t)(sg.xoff[seg] / xl_rows) * 6 + (size_t)j;
    const size_t ld = (size_t)sg.xld[seg];
#pragma unroll
    for (int a = 0; a < 6; ++a) xl[(size_t)a * ld] = x[a];
  }
  // ---- backward: u_i = V_i - Q_i u_{i+1}; P_i u_i in front of the first entry, P_i (u_i - V_i) added between first and last ----
  double u[6] = {0, 0, 0, 0, 0, 0};
  for (int i0 = beg + ((len - 1) / kCfFwdCh) * kCfFwdCh; i0 >= beg; i0 -= kCfFwdCh) {
    const int ch = i0 / kCfFwdCh;
    const int clen = (nf - i0 < kCfFwdCh) ? nf - i0 : kCfFwdCh;
    if (!__any(on && s_last >= i0 - beg)) continue;
    __builtin_amdgcn_wave_barrier();
    {
      double tq[kQ], tp[kQ], ty[2];
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        const int idx = q * 64 + lane, cl = idx < clen * 36 ? idx : 0;
        tq[q] = Qm[(size_t)i0 * 36 + cl];
        tp[q] = Pm[(size_t)i0 * 36 + cl];
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) { const int idx = q * 64 + lane; ty[q] = vy[(size_t)i0 * 6 + (idx < clen * 6 ? idx : 0)]; }
#pragma unroll
      for (int q = 0; q < kQ; ++q) { sA[q * 64 + lane] = tq[q]; sP[q * 64 + lane] = tp[q]; }
#pragma unroll
      for (int q = 0; q < 2; ++q) if (q * 64 + lane < kCfFwdCh * 6) svy[q * 64 + lane] = ty[q];
    }
    __builtin_amdgcn_wave_barrier();
    for (int h0 = ((clen - 1) / CH) * CH; h0 >= 0; h0 -= CH) {
      const int hl = (clen - h0 < CH) ? clen - h0 : CH;
      const int p0 = i0 - beg + h0;
      if (!__any(on && s_last >= p0)) continue;
      gather(ch, h0, p0, hl);
      for (int ii = hl - 1; ii >= 0; --ii) {
        const double* Qi = sA + (h0 + ii) * 36;
        const bool both = p0 + ii >= s_first;
        double un[6], d[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          const double v = sv[(ii * 6 + a) * 64 + lane];
          double t = v;
#pragma unroll
          for (int q = 0; q < 6; ++q) t -= Qi[a * 6 + q] * u[q];
          un[a] = t;
          d[a] = both ? t - v : t;
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) u[a] = un[a];
        const double* P = sP + (h0 + ii) * 36;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double t = 0;
#pragma unroll
          for (int q = 0; q < 6; ++q) t += P[a * 6 + q] * d[q];
          sv[(ii * 6 + a) * 64 + lane] = t;
        }
      }
      if (on) {
        const bool rmw = __any(s_first < s_last && s_first < p0 + hl && p0 < s_last) != 0;   // (wave-uniform; `on` lanes only have entries)
#pragma unroll
        for (int q0 = 0; q0 < CH * 6; q0 += 8) {
          double t[8], old[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) t[e] = sv[((q0 + e < hl * 6) ? q0 + e : 0) * 64 + lane];
          if (rmw) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int q = q0 + e, pos = p0 + q / 6;
              old[e] = (q < hl * 6 && pos >= s_first && pos < s_last) ? dst[(size_t)pos * dstep + q % 6] : 0.0;
            }
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) old[e] = 0.0;
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int q = q0 + e, pos = p0 + q / 6;
            if (q < hl * 6 && pos < s_last) dst[(size_t)pos * dstep + q % 6] = (pos >= s_first) ? old[e] + t[e] : t[e];
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---- z of the interior rows without the slab ------------------------------------------------------------------------------------------
// d_i = vy_i - sum over the list entries k at slot i of V_k x_o(ellipsoid of k): workgroup = interior slot, one wave, lane = element
// 6 b + a of a V record; the entries in the order of the layout's by-slot index (sl_start / sl_ent / sl_obj), the nine b of a row
// added in ascending order.  Written over z's rows of the slot.
static __global__ __launch_bounds__(64) void k_cf_wxo(int stride, const int* __restrict__ sl_start, const int* __restrict__ sl_ent,
                                                      const int* __restrict__ sl_obj, const double* __restrict__ V, const double* __restrict__ vy,
                                                      const double* __restrict__ xo, double* __restrict__ z) {
  __shared__ double red[64];
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i % stride == stride - 1) return;   // a separator: k_cf_z_sparse's dense row
  const int l = lane < 54 ? lane : 0, b = l / 6;
  const int qa = sl_start[i], qb = sl_start[i + 1];
  double s = 0;
  for (int q = qa; q < qb; q += 4) {   // batches of four entries in flight
    double v[4], w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int qq = (q + e < qb) ? q + e : qa;
      v[e] = V[(size_t)sl_ent[qq] * 54 + l];
      w[e] = xo[(size_t)9 * sl_obj[qq] + b];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) if (q + e < qb) s += v[e] * w[e];
  }
  red[lane] = s;
  __builtin_amdgcn_wave_barrier();
  if (lane < 6) {
    double t = 0;
#pragma unroll
    for (int bb = 0; bb < 9; ++bb) t += red[6 * bb + lane];
    z[(size_t)i * 6 + lane] = vy[(size_t)i * 6 + lane] - t;
  }
}
// z_i = d_i - M_i z_{i-1} over the segment's interior slots, in place: workgroup = segment, one wave, lanes 0..5 = the components
static __global__ __launch_bounds__(64) void k_cf_z_fwd(int nf_all, int stride, const double* __restrict__ Mm, double* __restrict__ z) {
  __shared__ double sM[kCfSweepSI * 36], sz[kCfSweepSI * 6];
  const int lane = threadIdx.x;
  const int beg = (int)blockIdx.x * stride;
  const int len = ((beg + stride - 1 < nf_all) ? beg + stride - 1 : nf_all) - beg;
  if (len <= 0) return;
  {
    constexpr int kQ = (kCfSweepSI * 36 + 63) / 64, kZ = (kCfSweepSI * 6 + 63) / 64;
    double tm[kQ], tz[kZ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) { const int idx = q * 64 + lane; tm[q] = Mm[(size_t)beg * 36 + (idx < len * 36 ? idx : 0)]; }
#pragma unroll
    for (int q = 0; q < kZ; ++q) { const int idx = q * 64 + lane; tz[q] = z[(size_t)beg * 6 + (idx < len * 6 ? idx : 0)]; }
#pragma unroll
    for (int q = 0; q < kQ; ++q) if (q * 64 + lane < kCfSweepSI * 36) sM[q * 64 + lane] = tm[q];
#pragma unroll
    for (int q = 0; q < kZ; ++q) if (q * 64 + lane < kCfSweepSI * 6) sz[q * 64 + lane] = tz[q];
  }
  __builtin_amdgcn_wave_barrier();
  const int a = lane < 6 ? lane : 5;
  double za = 0;
  for (int ii = 0; ii < len; ++ii) {
    double zp[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) zp[k] = cf_readlane(za, k);
    double t = sz[ii * 6 + a];
#pragma unroll
    for (int k = 0; k < 6; ++k) t -= sM[ii * 36 + a * 6 + k] * zp[k];
    za = t;
    if (lane < 6) sz[ii * 6 + lane] = t;
  }
  __builtin_amdgcn_wave_barrier();
  for (int idx = lane; idx < len * 6; idx += 64) z[(size_t)beg * 6 + idx] = sz[idx];
}

}  // namespace esl
