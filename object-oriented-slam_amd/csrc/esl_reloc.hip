// esl_reloc.hip — esl_reloc_set_map / esl_relocalize: camera pose and detection -> map association against a fixed map with no pose
// prior (include/esl.h, "relocalisation").  An exhaustive hypothesise-and-score search:
//   k_reloc_prep       gravity-frame coordinates and sorted half-axes (the map once per esl_reloc_set_map, the detections per call)
//   k_reloc_gate       the D x M candidate gate; per-wave ballot counts, then (second instantiation) the ordered fill
//   k_reloc_scan       one workgroup: exclusive scan of the wave counts -> the (d, m)-ordered CSR, P
//   k_reloc_hyp_gate   one lane per candidate PAIR of a slice: the survivors' keys are appended to a list (wave-aggregated integer
//                      atomic: the order of the list is free, the total order of esl_reloc_key.hpp decides the winner)
//   k_reloc_score      one lane per surviving hypothesis, dense; every lane of a wave walks the same candidate at the same time, the
//                      candidate table is read at wave-uniform addresses (scalar loads); wave / workgroup reduction of (n, cost, key)
//   k_reloc_merge      one workgroup: the partial winners + the running winner of the earlier slices
//   k_reloc_final      one wave: re-fit, rescore, one-to-one association, the result record
// No floating-point atomics anywhere: a hypothesis's score does not depend on which lane computes it, so runs are bit-reproducible.
// Everything lives in buffers of its own (esl_ctx::reloc) on the context's stream; nothing of the resident graph is written.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "esl_ctx.hpp"
#include "esl_reloc_key.hpp"

namespace esl {

static_assert(sizeof(esl_reloc_params) == 48 && sizeof(esl_reloc_result) == 120, "include/esl.h states these sizes");
constexpr int kRelocMaxDet = 64;          // one lane per detection in k_reloc_final
constexpr int kRelocMaxCand = 1 << 20;    // esl_reloc_params::max_candidates at most
constexpr int kRelocScoreBlocks = 1024;   // grid of k_reloc_score (grid-stride over the survivors)
constexpr uint64_t kRelocSlice = 1ull << 21;   // candidate pairs per slice = capacity of the survivor list (16 MB of keys)

struct RelocFrame { double A[9]; double d; };   // G(x) = A x + (0, 0, d)

struct RelocGates {
  double center_tol2, two_tol, height_tol, log_ratio, min_baseline;
  int min_inliers, match_labels, refine, size_gate;
};

// what the device returns: one small copy
struct RelocOut {
  int32_t status, n_candidates;
  int64_t n_hypotheses, best_key;
  int32_t n_inliers, refined;
  double cost, yaw, tx, ty;
  int32_t assoc[kRelocMaxDet];
};

struct RelocState {
  bool have_map = false;
  int M = 0;
  RelocFrame Gw;
  // the map (double objs, xyh, ax; int lab), the detections (the same four, kRelocMaxDet of them), the candidate compaction (int
  // wave_cnt, wave_off, row[kRelocMaxDet + 1], c_d, c_m; double2 c_p), the hypotheses (u64 surv; u64 counters[4]: [0] survivors of the
  // current slice, [1] hypotheses so far, [2] P; RelocBest part[kRelocScoreBlocks], best; RelocOut out)
  enum { M_OBJS, M_XYH, M_AX, M_LAB, D_OBJS, D_XYH, D_AX, D_LAB, WAVE_CNT, WAVE_OFF, ROW, C_D, C_M, C_P, SURV, COUNTERS, PART, BEST, OUT,
         kBufs };
  ScratchSet<kBufs> set;
  char* host = nullptr;                     // pinned: detections in, RelocOut / counters back
};

// ---------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_reloc_prep(const double* __restrict__ objs, int n, RelocFrame f,
                                                           double* __restrict__ xyh, double* __restrict__ ax) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= n) return;
  const double* e = objs + (size_t)o * 10;
  const double x = e[0], y = e[1], z = e[2];
  xyh[o * 3 + 0] = f.A[0] * x + f.A[1] * y + f.A[2] * z;
  xyh[o * 3 + 1] = f.A[3] * x + f.A[4] * y + f.A[5] * z;
  xyh[o * 3 + 2] = f.A[6] * x + f.A[7] * y + f.A[8] * z + f.d;
  double a = e[7], b = e[8], c = e[9], t;
  if (a > b) { t = a; a = b; b = t; }
  if (b > c) { t = b; b = c; c = t; }
  if (a > b) { t = a; a = b; b = t; }
  ax[o * 3 + 0] = a; ax[o * 3 + 1] = b; ax[o * 3 + 2] = c;
}

struct RelocGateArgs {
  const double* m_xyh; const double* m_ax; const int* m_lab;
  const double* d_xyh; const double* d_ax; const int* d_lab;
  int M, D, wpd;            // wpd = waves per detection = ceil(M / 64)
  int* wave_cnt; const int* wave_off;
  int* c_d; int* c_m; double2* c_p; int cand_cap;
  RelocGates g;
};

// grid (ceil(M / 256), D).  FILL = false: the ballot count of every wave; FILL = true: the same ballot again, every candidate to its
// place behind the scanned count of its wave -- (d, m) lexicographic whatever order the waves run in.
template <bool FILL>
static __global__ __launch_bounds__(256) void k_reloc_gate(RelocGateArgs a) {
  const int m = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
  bool ok = false;
  if (m < a.M) {
    ok = !a.g.match_labels || a.m_lab[m] == a.d_lab[d];
    ok = ok && fabs(a.d_xyh[d * 3 + 2] - a.m_xyh[(size_t)m * 3 + 2]) <= a.g.height_tol;
    if (a.g.size_gate) {
      double lr = 0;
      for (int k = 0; k < 3; ++k) lr = fmax(lr, fabs(log(a.d_ax[d * 3 + k] / a.m_ax[(size_t)m * 3 + k])));
      // fmax drops a NaN: a non-positive half-axis must fail the gate
      const bool pos = a.d_ax[d * 3] > 0 && a.m_ax[(size_t)m * 3] > 0;
      ok = ok && pos && lr <= a.g.log_ratio;
    }
  }
  const unsigned long long mask = __ballot(ok);
  const int wv = m >> 6, lane = threadIdx.x & 63;
  if (wv >= a.wpd) return;
  const size_t w = (size_t)d * a.wpd + wv;
  if (!FILL) {
    if (lane == 0) a.wave_cnt[w] = __popcll(mask);
  } else if (ok) {
    const int pos = a.wave_off[w] + __popcll(mask & ((1ull << lane) - 1ull));
    if (pos < a.cand_cap) {
      a.c_d[pos] = d; a.c_m[pos] = m;
      a.c_p[pos] = make_double2(a.m_xyh[(size_t)m * 3], a.m_xyh[(size_t)m * 3 + 1]);
    }
  }
}

// one workgroup: exclusive scan of nw wave counts, the rows of the CSR, P; resets the counters and the running winner
static __global__ __launch_bounds__(256) void k_reloc_scan(const int* __restrict__ wave_cnt, int* __restrict__ wave_off, long long nw,
                                                           int D, int wpd, int* __restrict__ row, unsigned long long* __restrict__ counters,
                                                           RelocBest* __restrict__ best) {
  __shared__ long long s_sum[256];
  const long long len = (nw + 255) / 256, lo = std::min<long long>(threadIdx.x * len, nw), hi = std::min<long long>(lo + len, nw);
  long long sum = 0;
  for (long long k = lo; k < hi; ++k) sum += wave_cnt[k];
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = 0;
    for (int k = 0; k < 256; ++k) { const long long v = s_sum[k]; s_sum[k] = run; run += v; }
    counters[0] = 0; counters[1] = 0; counters[2] = (unsigned long long)run;
    row[D] = (int)std::min<long long>(run, 0x7fffffff);
    best->key = -1; best->cost = 0; best->n = 0; best->pad = 0;
  }
  __syncthreads();
  long long run = s_sum[threadIdx.x];
  for (long long k = lo; k < hi; ++k) {
    const int v = wave_cnt[k];
    const int off = (int)std::min<long long>(run, 0x7fffffff);
    wave_off[k] = off;
    if (k % wpd == 0) row[k / wpd] = off;
    run += v;
  }
}

struct RelocHyp { double c, s, tx, ty; };
// the planar motion that carries the detection pair (qi, qj) onto the map pair (pi, pj)
static __device__ __forceinline__ RelocHyp reloc_motion(double2 qi, double2 qj, double2 pi, double2 pj, double* psi_out) {
  const double psi = atan2(pj.y - pi.y, pj.x - pi.x) - atan2(qj.y - qi.y, qj.x - qi.x);
  RelocHyp h;
  h.c = cos(psi); h.s = sin(psi);
  const double mqx = 0.5 * (qi.x + qj.x), mqy = 0.5 * (qi.y + qj.y);
  h.tx = 0.5 * (pi.x + pj.x) - (h.c * mqx - h.s * mqy);
  h.ty = 0.5 * (pi.y + pj.y) - (h.s * mqx + h.c * mqy);
  if (psi_out) *psi_out = psi;
  return h;
}

// one lane per pair t in [t0, t1): the gates of step 3; the survivors' keys go to surv[]
static __global__ __launch_bounds__(256) void k_reloc_hyp_gate(const int* __restrict__ c_d, const int* __restrict__ c_m,
                                                               const double2* __restrict__ c_p, const double* __restrict__ d_xyh,
                                                               unsigned long long P, unsigned long long t0, unsigned long long t1,
                                                               double min_baseline, double two_tol, unsigned long long* __restrict__ surv,
                                                               unsigned long long surv_cap, unsigned long long* __restrict__ counters) {
  const unsigned long long t = t0 + (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  bool ok = false;
  uint64_t i = 0, j = 0;
  if (t < t1) {
    reloc_pair_decode(t, i, j);
    const int di = c_d[i], dj = c_d[j];
    if (di != dj && c_m[i] != c_m[j]) {
      const double2 pi = c_p[i], pj = c_p[j];
      const double qx = d_xyh[dj * 3] - d_xyh[di * 3], qy = d_xyh[dj * 3 + 1] - d_xyh[di * 3 + 1];
      const double px = pj.x - pi.x, py = pj.y - pi.y;
      const double lq = sqrt(qx * qx + qy * qy), lp = sqrt(px * px + py * py);
      ok = lq >= min_baseline && fabs(lq - lp) <= two_tol;
    }
  }
  const unsigned long long mask = __ballot(ok);
  if (mask == 0) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)mask) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(&counters[0], (unsigned long long)__popcll(mask));
  base = __shfl(base, leader, 64);
  if (ok) {
    const unsigned long long pos = base + __popcll(mask & ((1ull << lane) - 1ull));
    if (pos < surv_cap) surv[pos] = i * P + j;
  }
}

static __device__ __forceinline__ void reloc_best_wave(int& n, double& cost, long long& key) {
  for (int off = 32; off > 0; off >>= 1) {
    const int n2 = __shfl_xor(n, off, 64);
    const double c2 = __shfl_xor(cost, off, 64);
    const long long k2 = __shfl_xor(key, off, 64);
    if (reloc_better(n2, c2, k2, n, cost, key)) { n = n2; cost = c2; key = k2; }
  }
}
// (n, cost, key) of 256 threads -> thread 0
static __device__ __forceinline__ void reloc_best_block(int& n, double& cost, long long& key) {
  __shared__ int s_n[4]; __shared__ double s_c[4]; __shared__ long long s_k[4];
  reloc_best_wave(n, cost, key);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_n[wv] = n; s_c[wv] = cost; s_k[wv] = key; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < 4; ++k)
      if (reloc_better(s_n[k], s_c[k], s_k[k], n, cost, key)) { n = s_n[k]; cost = s_c[k]; key = s_k[k]; }
}

// one lane per surviving hypothesis (grid-stride).  The two loops below run over wave-uniform bounds and read row[], d_xyh[] and c_p[]
// at wave-uniform addresses: scalar loads, one per wave, and every lane spends its time on its own hypothesis's arithmetic.
static __global__ __launch_bounds__(256) void k_reloc_score(const int* __restrict__ row, const int* __restrict__ c_d,
                                                            const double2* __restrict__ c_p, const double* __restrict__ d_xyh, int D,
                                                            unsigned long long P, const unsigned long long* __restrict__ surv,
                                                            unsigned long long surv_cap, const unsigned long long* __restrict__ counters,
                                                            double tol2, RelocBest* __restrict__ part) {
  const unsigned long long S = std::min<unsigned long long>(counters[0], surv_cap);
  int bn = 0; double bc = 0; long long bk = -1;
  for (unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x; s < S; s += (unsigned long long)gridDim.x * 256) {
    const unsigned long long key = surv[s];
    const unsigned long long i = key / P, j = key - i * P;
    const int di = c_d[i], dj = c_d[j];
    const RelocHyp h = reloc_motion(make_double2(d_xyh[di * 3], d_xyh[di * 3 + 1]), make_double2(d_xyh[dj * 3], d_xyh[dj * 3 + 1]),
                                    c_p[i], c_p[j], nullptr);
    int n = 0; double cost = 0;
    for (int d = 0; d < D; ++d) {
      const int k0 = row[d], k1 = row[d + 1];
      if (k0 == k1) continue;
      const double qx = d_xyh[d * 3], qy = d_xyh[d * 3 + 1];
      const double mx = h.c * qx - h.s * qy + h.tx, my = h.s * qx + h.c * qy + h.ty;
      double best = INFINITY;
      for (int k = k0; k < k1; ++k) {
        const double2 p = c_p[k];
        const double ex = mx - p.x, ey = my - p.y;
        best = fmin(best, ex * ex + ey * ey);
      }
      if (best <= tol2) { ++n; cost += best; }
    }
    if (reloc_better(n, cost, (long long)key, bn, bc, bk)) { bn = n; bc = cost; bk = (long long)key; }
  }
  reloc_best_block(bn, bc, bk);
  if (threadIdx.x == 0) { RelocBest b; b.key = bk; b.cost = bc; b.n = bn; b.pad = 0; part[blockIdx.x] = b; }
}

// one workgroup: partial winners of a slice + the running winner; closes the slice's counters
static __global__ __launch_bounds__(256) void k_reloc_merge(const RelocBest* __restrict__ part, int n_part, RelocBest* __restrict__ best,
                                                            unsigned long long* __restrict__ counters, unsigned long long surv_cap) {
  int bn = 0; double bc = 0; long long bk = -1;
  for (int k = threadIdx.x; k < n_part; k += 256) {
    const RelocBest b = part[k];
    if (reloc_better(b.n, b.cost, b.key, bn, bc, bk)) { bn = b.n; bc = b.cost; bk = b.key; }
  }
  reloc_best_block(bn, bc, bk);
  if (threadIdx.x == 0) {
    if (reloc_better(bn, bc, bk, best->n, best->cost, best->key)) { best->n = bn; best->cost = bc; best->key = bk; }
    counters[1] += std::min<unsigned long long>(counters[0], surv_cap);
    counters[0] = 0;
  }
}

struct RelocFinalArgs {
  const int* row; const int* c_d; const int* c_m; const double2* c_p; const double* d_xyh;
  const RelocBest* best; const unsigned long long* counters;
  int D; RelocGates g; RelocOut* out;
};

// nearest candidate of detection d after the motion (c, s, tx, ty), map objects in claim[0 .. n_claim) excluded: all 64 lanes walk the
// row together; (squared distance, candidate) comes back wave-uniform, the lowest candidate on a tie, k = INT_MAX when there is none
static __device__ __forceinline__ void reloc_nearest(const RelocFinalArgs& a, int d, double c, double s, double tx, double ty,
                                                     const int* claim, int n_claim, double& d2_out, int& k_out) {
  const int lane = threadIdx.x & 63;
  const double qx = a.d_xyh[d * 3], qy = a.d_xyh[d * 3 + 1];
  const double mx = c * qx - s * qy + tx, my = s * qx + c * qy + ty;
  double bd = INFINITY; int bk = 0x7fffffff;
  for (int k = a.row[d] + lane; k < a.row[d + 1]; k += 64) {
    const int m = a.c_m[k];
    bool taken = false;
    for (int u = 0; u < n_claim; ++u) taken = taken || claim[u] == m;
    if (taken) continue;
    const double2 p = a.c_p[k];
    const double ex = mx - p.x, ey = my - p.y, d2 = ex * ex + ey * ey;
    if (d2 < bd) { bd = d2; bk = k; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double d2 = __shfl_xor(bd, off, 64);
    const int k2 = __shfl_xor(bk, off, 64);
    if (k2 != 0x7fffffff && (bk == 0x7fffffff || d2 < bd || (d2 == bd && k2 < bk))) { bd = d2; bk = k2; }
  }
  d2_out = bd; k_out = bk;
}

// one wave; every value below is wave-uniform (each lane carries the same sums, taken in detection order)
static __global__ __launch_bounds__(64) void k_reloc_final(RelocFinalArgs a) {
  __shared__ int s_near[kRelocMaxDet], s_claim[kRelocMaxDet];
  const int lane = threadIdx.x;
  RelocOut* o = a.out;
  const RelocBest b = *a.best;
  const unsigned long long P = a.counters[2];
  if (lane == 0) {
    o->status = 1; o->n_candidates = (int32_t)P; o->n_hypotheses = (int64_t)a.counters[1]; o->best_key = b.key;
    o->n_inliers = 0; o->refined = 0; o->cost = 0; o->yaw = 0; o->tx = 0; o->ty = 0;
  }
  o->assoc[lane] = -1;
  if (b.key < 0) return;
  const unsigned long long bi = (unsigned long long)b.key / P, bj = (unsigned long long)b.key - bi * P;
  const int di = a.c_d[bi], dj = a.c_d[bj];
  double psi;
  RelocHyp h = reloc_motion(make_double2(a.d_xyh[di * 3], a.d_xyh[di * 3 + 1]), make_double2(a.d_xyh[dj * 3], a.d_xyh[dj * 3 + 1]),
                            a.c_p[bi], a.c_p[bj], &psi);
  const double tol2 = a.g.center_tol2;
  // the winner's inlier pairs
  int n0 = 0; double cost0 = 0;
  for (int d = 0; d < a.D; ++d) {
    double d2; int k;
    reloc_nearest(a, d, h.c, h.s, h.tx, h.ty, s_claim, 0, d2, k);
    const bool in = k != 0x7fffffff && d2 <= tol2;
    if (in) { ++n0; cost0 += d2; }
    if (lane == 0) s_near[d] = in ? k : -1;
  }
  __syncthreads();
  if (n0 < a.g.min_inliers) {
    if (lane == 0) { o->status = 2; o->n_inliers = n0; o->cost = cost0; }
    return;
  }
  int refined = 0;
  if (a.g.refine && n0 >= 3) {
    double mqx = 0, mqy = 0, mpx = 0, mpy = 0;
    for (int d = 0; d < a.D; ++d) {
      const int k = s_near[d];
      if (k < 0) continue;
      mqx += a.d_xyh[d * 3]; mqy += a.d_xyh[d * 3 + 1];
      const double2 p = a.c_p[k]; mpx += p.x; mpy += p.y;
    }
    mqx /= n0; mqy /= n0; mpx /= n0; mpy /= n0;
    double sc = 0, sd = 0;
    for (int d = 0; d < a.D; ++d) {
      const int k = s_near[d];
      if (k < 0) continue;
      const double ax = a.d_xyh[d * 3] - mqx, ay = a.d_xyh[d * 3 + 1] - mqy;
      const double2 p = a.c_p[k];
      const double bx = p.x - mpx, by = p.y - mpy;
      sc += ax * by - ay * bx; sd += ax * bx + ay * by;
    }
    const double psi1 = atan2(sc, sd);
    RelocHyp h1;
    h1.c = cos(psi1); h1.s = sin(psi1);
    h1.tx = mpx - (h1.c * mqx - h1.s * mqy); h1.ty = mpy - (h1.s * mqx + h1.c * mqy);
    int n1 = 0; double cost1 = 0;
    for (int d = 0; d < a.D; ++d) {
      double d2; int k;
      reloc_nearest(a, d, h1.c, h1.s, h1.tx, h1.ty, s_claim, 0, d2, k);
      if (k != 0x7fffffff && d2 <= tol2) { ++n1; cost1 += d2; }
    }
    if (n1 > n0 || (n1 == n0 && cost1 <= cost0)) { h = h1; psi = psi1; refined = 1; }
  }
  // association: detections in index order, nearest unclaimed candidate within center_tol
  int nc = 0; double cost = 0;
  for (int d = 0; d < a.D; ++d) {
    double d2; int k;
    reloc_nearest(a, d, h.c, h.s, h.tx, h.ty, s_claim, nc, d2, k);
    if (k != 0x7fffffff && d2 <= tol2) {
      const int m = a.c_m[k];
      __syncthreads();                    // every lane has read the claims of this round
      if (lane == 0) { s_claim[nc] = m; o->assoc[d] = m; }
      __syncthreads();
      ++nc; cost += d2;
    }
  }
  if (lane == 0) {
    o->status = 0; o->n_inliers = nc; o->refined = refined; o->cost = cost;
    o->yaw = atan2(h.s, h.c); o->tx = h.tx; o->ty = h.ty;
    (void)psi;
  }
}

// ---------------------------------------------------------------------------------------------------
void reloc_scratch_stats(const esl_ctx* c, int64_t* allocs, int64_t* bytes) {
  if (c->reloc) { *allocs = c->reloc->set.allocs(); *bytes = (int64_t)c->reloc->set.held(); }
}

void reloc_release(esl_ctx* c) {   // called by esl_ctx_destroy
  RelocState* r = c->reloc;
  if (!r) return;
  r->set.release();
  if (r->host) (void)hipHostFree(r->host);
  delete r;
  c->reloc = nullptr;
}

}  // namespace esl

using namespace esl;

namespace {

// the buffers whose size never changes
int reloc_state(esl_ctx* c, RelocState** out) {
  if (!c->reloc) c->reloc = new RelocState();
  RelocState* r = c->reloc;
  *out = r;
  if (r->host) return ESL_OK;
  using R = RelocState;
  const int slot[9] = {R::D_OBJS, R::D_XYH, R::D_AX, R::D_LAB, R::ROW, R::COUNTERS, R::PART, R::BEST, R::OUT};
  const size_t bytes[9] = {kRelocMaxDet * 10 * sizeof(double), kRelocMaxDet * 3 * sizeof(double), kRelocMaxDet * 3 * sizeof(double),
                           kRelocMaxDet * sizeof(int), (kRelocMaxDet + 1) * sizeof(int), 4 * sizeof(unsigned long long),
                           kRelocScoreBlocks * sizeof(RelocBest), sizeof(RelocBest), sizeof(RelocOut)};
  for (int i = 0; i < 9; ++i)
    if (const int rc = r->set.grow(c, slot[i], bytes[i])) return rc;
  ESL_HIP_TRY(hipHostMalloc((void**)&r->host, 8192, hipHostMallocDefault));
  return ESL_OK;
}

// gravity frame of a plane (include/esl.h, step 1); false for a normal shorter than 1e-12 or a non-finite plane
bool reloc_frame(const double pl[4], RelocFrame& f) {
  const double nn = std::sqrt(pl[0] * pl[0] + pl[1] * pl[1] + pl[2] * pl[2]);
  if (!(nn >= 1e-12) || !std::isfinite(nn) || !std::isfinite(pl[3])) return false;
  const double n[3] = {pl[0] / nn, pl[1] / nn, pl[2] / nn};
  int k = 0;
  for (int a = 1; a < 3; ++a) if (std::fabs(n[a]) < std::fabs(n[k])) k = a;
  double e[3] = {0, 0, 0}; e[k] = 1;
  double u[3] = {e[1] * n[2] - e[2] * n[1], e[2] * n[0] - e[0] * n[2], e[0] * n[1] - e[1] * n[0]};
  const double un = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (double& v : u) v /= un;
  const double v[3] = {n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]};
  for (int a = 0; a < 3; ++a) { f.A[a] = u[a]; f.A[3 + a] = v[a]; f.A[6 + a] = n[a]; }
  f.d = pl[3] / nn;
  return true;
}

// rotation (row-major) -> x y z w with w >= 0, largest-component branch
void reloc_rot_to_quat(const double R[9], double q[4]) {
  const double v[4] = {1 + R[0] + R[4] + R[8], 1 + R[0] - R[4] - R[8], 1 - R[0] + R[4] - R[8], 1 - R[0] - R[4] + R[8]};
  int k = 0;
  for (int a = 1; a < 4; ++a) if (v[a] > v[k]) k = a;
  const double s = 2 * std::sqrt(v[k]);
  if (k == 0) { q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s; q[3] = s / 4; }
  else if (k == 1) { q[0] = s / 4; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s; q[3] = (R[7] - R[5]) / s; }
  else if (k == 2) { q[0] = (R[1] + R[3]) / s; q[1] = s / 4; q[2] = (R[5] + R[7]) / s; q[3] = (R[2] - R[6]) / s; }
  else { q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = s / 4; q[3] = (R[3] - R[1]) / s; }
  const double nn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double sg = q[3] < 0 ? -1.0 : 1.0;
  for (int a = 0; a < 4; ++a) q[a] = sg * q[a] / nn;
}

// Twc of x_w = G_w^-1(Z(yaw, t) G_c(x_c)): R = Aw^T Z Ac, t = Aw^T (tx, ty, dc - dw)
void reloc_pose(const RelocFrame& w, const RelocFrame& cf, double yaw, double tx, double ty, double Twc[7]) {
  const double c = std::cos(yaw), s = std::sin(yaw);
  const double Z[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
  double ZA[9], R[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) ZA[a * 3 + b] = Z[a * 3] * cf.A[b] + Z[a * 3 + 1] * cf.A[3 + b] + Z[a * 3 + 2] * cf.A[6 + b];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) R[a * 3 + b] = w.A[a] * ZA[b] + w.A[3 + a] * ZA[3 + b] + w.A[6 + a] * ZA[6 + b];
  const double t[3] = {tx, ty, cf.d - w.d};
  for (int a = 0; a < 3; ++a) Twc[a] = w.A[a] * t[0] + w.A[3 + a] * t[1] + w.A[6 + a] * t[2];
  reloc_rot_to_quat(R, Twc + 3);
}

}  // namespace

extern "C" void esl_reloc_params_default(esl_reloc_params* p) {
  if (!p) return;
  // design choices, not values tuned on real data (include/esl.h)
  p->center_tol = 0.25; p->height_tol = 0.25; p->size_ratio = 1.5; p->min_baseline = 0.5;
  p->min_inliers = 3; p->max_candidates = 4096; p->match_labels = 1; p->refine = 1;
}

extern "C" int esl_reloc_set_map(esl_ctx* c, const double* objs, const int32_t* labels, int32_t M, const double ground_world[4]) {
  if (!c || M < 0 || !ground_world || (M > 0 && !labels)) { set_error("esl_reloc_set_map: bad argument"); return ESL_ERR_INVALID; }
  RelocFrame f;
  if (!reloc_frame(ground_world, f)) { set_error("esl_reloc_set_map: the ground plane's normal is shorter than 1e-12"); return ESL_ERR_INVALID; }
  if (const int rc = resident_source_check(c, "esl_reloc_set_map", false, 0, !objs && M > 0, M)) return rc;
  ESL_HIP_TRY(hipSetDevice(c->device));
  RelocState* r = nullptr;
  if (const int rc = reloc_state(c, &r)) return rc;
  r->have_map = false;
  using R = RelocState;
  ScratchSet<R::kBufs>& s = r->set;
  if (const int rc = s.grow(c, R::M_OBJS, (size_t)M * 10 * sizeof(double))) return rc;
  if (const int rc = s.grow(c, R::M_XYH, (size_t)M * 3 * sizeof(double))) return rc;
  if (const int rc = s.grow(c, R::M_AX, (size_t)M * 3 * sizeof(double))) return rc;
  if (const int rc = s.grow(c, R::M_LAB, (size_t)M * sizeof(int))) return rc;
  if (M > 0) {
    double* m_objs = s.at<double>(R::M_OBJS);   // a copy of the map: the resident states may move on, the map stays
    if (objs) ESL_HIP_TRY(hipMemcpyAsync(m_objs, objs, (size_t)M * 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    else ESL_HIP_TRY(hipMemcpyAsync(m_objs, c->objs, (size_t)M * 10 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[R::M_LAB], labels, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_reloc_prep, dim3((M + 255) / 256), dim3(256), 0, c->stream, (const double*)m_objs, (int)M, f, s.at<double>(R::M_XYH),
                       s.at<double>(R::M_AX));
    ESL_HIP_TRY(hipGetLastError());
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's arrays are free again
  }
  r->M = M; r->Gw = f; r->have_map = true;
  return ESL_OK;
}

extern "C" int esl_relocalize(esl_ctx* c, const double* det_objs, const int32_t* det_labels, int32_t D, const double ground_cam[4],
                              const esl_reloc_params* pp, esl_reloc_result* out, int32_t* assoc_out) {
  if (!c || !out || !ground_cam || D < 0 || D > kRelocMaxDet || (D > 0 && (!det_objs || !det_labels))) {
    set_error("esl_relocalize: bad argument (null pointer, D < 0 or D > 64)"); return ESL_ERR_INVALID;
  }
  esl_reloc_params p;
  if (pp) p = *pp; else esl_reloc_params_default(&p);
  const double tolv[4] = {p.center_tol, p.height_tol, p.size_ratio, p.min_baseline};
  for (double v : tolv) if (!std::isfinite(v)) { set_error("esl_relocalize: non-finite tolerance"); return ESL_ERR_INVALID; }
  if (p.center_tol < 0 || p.height_tol < 0 || p.min_baseline < 0 || p.min_inliers < 0 || p.max_candidates < 0 || p.max_candidates > kRelocMaxCand) {
    set_error("esl_relocalize: negative tolerance or count, or max_candidates above 1048576"); return ESL_ERR_INVALID;
  }
  RelocFrame fc;
  if (!reloc_frame(ground_cam, fc)) { set_error("esl_relocalize: the ground plane's normal is shorter than 1e-12"); return ESL_ERR_INVALID; }
  RelocState* r = c->reloc;
  if (!r || !r->have_map) { set_error("esl_relocalize: no map (esl_reloc_set_map)"); return ESL_ERR_STATE; }
  ESL_HIP_TRY(hipSetDevice(c->device));

  std::memset(out, 0, sizeof(*out));
  out->status = 1; out->best_key = -1; out->Twc[6] = 1;
  if (assoc_out) for (int d = 0; d < D; ++d) assoc_out[d] = -1;
  const int M = r->M;
  if (D == 0 || M == 0) return ESL_OK;

  RelocGates g;
  g.center_tol2 = p.center_tol * p.center_tol; g.two_tol = 2 * p.center_tol; g.height_tol = p.height_tol;
  g.size_gate = p.size_ratio > 1; g.log_ratio = g.size_gate ? std::log(p.size_ratio) : 0; g.min_baseline = p.min_baseline;
  g.min_inliers = p.min_inliers; g.match_labels = p.match_labels != 0; g.refine = p.refine != 0;

  using R = RelocState;
  ScratchSet<R::kBufs>& s = r->set;
  double *const d_objs = s.at<double>(R::D_OBJS), *const d_xyh = s.at<double>(R::D_XYH), *const d_ax = s.at<double>(R::D_AX);
  int *const d_lab = s.at<int>(R::D_LAB), *const row = s.at<int>(R::ROW);
  unsigned long long* const counters = s.at<unsigned long long>(R::COUNTERS);
  RelocBest *const part = s.at<RelocBest>(R::PART), *const best = s.at<RelocBest>(R::BEST);

  // detections: staged through the pinned block, prepared on the device
  double* h_objs = (double*)r->host; int32_t* h_lab = (int32_t*)(r->host + kRelocMaxDet * 10 * sizeof(double));
  std::memcpy(h_objs, det_objs, (size_t)D * 10 * sizeof(double));
  std::memcpy(h_lab, det_labels, (size_t)D * sizeof(int32_t));
  ESL_HIP_TRY(hipMemcpyAsync(d_objs, h_objs, (size_t)D * 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(d_lab, h_lab, (size_t)D * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_reloc_prep, dim3(1), dim3(256), 0, c->stream, (const double*)d_objs, (int)D, fc, d_xyh, d_ax);

  // candidates: count per wave, scan, (after the host has seen P) fill
  const int wpd = (M + 63) / 64;
  const size_t nw = (size_t)D * wpd;
  if (const int rc = s.grow(c, R::WAVE_CNT, nw * sizeof(int))) return rc;
  if (const int rc = s.grow(c, R::WAVE_OFF, nw * sizeof(int))) return rc;
  const size_t ccap = (size_t)std::max(p.max_candidates, 2);
  if (const int rc = s.grow(c, R::C_D, ccap * sizeof(int))) return rc;
  if (const int rc = s.grow(c, R::C_M, ccap * sizeof(int))) return rc;
  if (const int rc = s.grow(c, R::C_P, ccap * sizeof(double2))) return rc;
  int *const wave_cnt = s.at<int>(R::WAVE_CNT), *const wave_off = s.at<int>(R::WAVE_OFF);
  int *const c_d = s.at<int>(R::C_D), *const c_m = s.at<int>(R::C_M);
  double2* const c_p = s.at<double2>(R::C_P);
  RelocGateArgs ga;
  ga.m_xyh = s.at<double>(R::M_XYH); ga.m_ax = s.at<double>(R::M_AX); ga.m_lab = s.at<int>(R::M_LAB);
  ga.d_xyh = d_xyh; ga.d_ax = d_ax; ga.d_lab = d_lab;
  ga.M = M; ga.D = D; ga.wpd = wpd; ga.wave_cnt = wave_cnt; ga.wave_off = wave_off;
  // the candidate lists' capacity in entries: the largest max_candidates so far, not this call's (the three lists grow together)
  ga.c_d = c_d; ga.c_m = c_m; ga.c_p = c_p; ga.cand_cap = (int)(s.cap[R::C_D] / sizeof(int)); ga.g = g;
  const dim3 ggrid((M + 255) / 256, D);
  hipLaunchKernelGGL(k_reloc_gate<false>, ggrid, dim3(256), 0, c->stream, ga);
  hipLaunchKernelGGL(k_reloc_scan, dim3(1), dim3(256), 0, c->stream, (const int*)wave_cnt, wave_off, (long long)nw, (int)D, wpd,
                     row, counters, best);
  ESL_HIP_TRY(hipGetLastError());
  unsigned long long* h_cnt = (unsigned long long*)(r->host + 6144);
  ESL_HIP_TRY(hipMemcpyAsync(h_cnt, counters, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  const unsigned long long P = h_cnt[2];
  out->n_candidates = (int32_t)std::min<unsigned long long>(P, 0x7fffffff);
  if (P > (unsigned long long)p.max_candidates) { out->status = 3; return ESL_OK; }
  if (P < 2) return ESL_OK;
  hipLaunchKernelGGL(k_reloc_gate<true>, ggrid, dim3(256), 0, c->stream, ga);

  // hypotheses, slice by slice (ESL_RELOC_SLICE: pairs per slice, for tests; the result does not depend on it)
  uint64_t slice = kRelocSlice;
  if (const char* e = std::getenv("ESL_RELOC_SLICE")) { const long long v = std::atoll(e); if (v >= 64) slice = (uint64_t)v; }
  const uint64_t n_pairs = reloc_pair_count(P);
  slice = std::min<uint64_t>(slice, n_pairs);
  if (const int rc = s.grow(c, R::SURV, (size_t)slice * sizeof(unsigned long long))) return rc;
  unsigned long long* const surv = s.at<unsigned long long>(R::SURV);
  for (uint64_t t0 = 0; t0 < n_pairs; t0 += slice) {
    const uint64_t t1 = std::min<uint64_t>(t0 + slice, n_pairs);
    hipLaunchKernelGGL(k_reloc_hyp_gate, dim3((unsigned)((t1 - t0 + 255) / 256)), dim3(256), 0, c->stream, (const int*)c_d,
                       (const int*)c_m, (const double2*)c_p, (const double*)d_xyh, P, (unsigned long long)t0, (unsigned long long)t1,
                       g.min_baseline, g.two_tol, surv, (unsigned long long)slice, counters);
    const int nb = (int)std::min<uint64_t>((t1 - t0 + 255) / 256, kRelocScoreBlocks);
    hipLaunchKernelGGL(k_reloc_score, dim3(nb), dim3(256), 0, c->stream, (const int*)row, (const int*)c_d, (const double2*)c_p,
                       (const double*)d_xyh, (int)D, P, (const unsigned long long*)surv, (unsigned long long)slice,
                       (const unsigned long long*)counters, g.center_tol2, part);
    hipLaunchKernelGGL(k_reloc_merge, dim3(1), dim3(256), 0, c->stream, (const RelocBest*)part, nb, best, counters,
                       (unsigned long long)slice);
  }
  RelocFinalArgs fa;
  fa.row = row; fa.c_d = c_d; fa.c_m = c_m; fa.c_p = c_p; fa.d_xyh = d_xyh; fa.best = best; fa.counters = counters;
  fa.D = D; fa.g = g; fa.out = s.at<RelocOut>(R::OUT);
  hipLaunchKernelGGL(k_reloc_final, dim3(1), dim3(64), 0, c->stream, fa);
  ESL_HIP_TRY(hipGetLastError());
  RelocOut* ho = (RelocOut*)(r->host + 6144);
  ESL_HIP_TRY(hipMemcpyAsync(ho, fa.out, sizeof(RelocOut), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));

  out->status = ho->status; out->n_candidates = ho->n_candidates; out->n_hypotheses = ho->n_hypotheses;
  out->best_key = ho->best_key; out->n_inliers = ho->n_inliers; out->refined = ho->refined; out->cost = ho->cost;
  if (ho->status == 0) {
    out->yaw = ho->yaw; out->tx = ho->tx; out->ty = ho->ty;
    reloc_pose(r->Gw, fc, ho->yaw, ho->tx, ho->ty, out->Twc);
    if (assoc_out) for (int d = 0; d < D; ++d) assoc_out[d] = ho->assoc[d];
  }
  return ESL_OK;
}
