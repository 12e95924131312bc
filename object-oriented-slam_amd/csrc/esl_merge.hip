// esl_merge.hip — esl_map_overlaps / esl_map_merge: which ellipsoids of a map are the same object, fused, with the edge list rewritten
// (include/esl.h, "map maintenance"; the steps' numbers below are the header's).
//   k_merge_prep      one thread per ellipsoid: validity, R, half-axes, volume; the candidate pass's record (centre, radius; radius < 0 = invalid)
//   k_merge_cand      the gate of step 4 over all pairs i < j: 256 rows per workgroup against tiles of 256 columns staged in LDS, once to
//                     count a row's candidates and, after k_merge_scan, once more to write them -- row by row, ascending j: the list is
//                     in (i, j) order whatever the schedule
//   k_merge_overlap   one wavefront per candidate, both directions in one walk through the lattice's cube: the pair's two affine maps
//                     (lattice integers of one body -> unit-ball coordinates of the other) are set up once in registers, a lane takes
//                     the cells lane, lane + 64, ... (esl_merge_lattice.hpp: no division in the loop), inside lanes are counted with a
//                     ballot and a popcount into integers.  Lane 0 turns the two integers into iou / contain / link.
//   k_merge_rows      esl_map_overlaps: the overlapping pairs of every row, counted, scanned, written (again no atomic append)
//   k_merge_hook / k_merge_jump   connected components of the links: hook the larger root under the smaller (integer atomicMin), then
//                     full path compression, until a round changes nothing; the fixed point (every member -> the smallest index) is unique
//   k_merge_group_*   per group: representative (64-bit atomicMax on an ordered key), weight sum and size (integer atomicAdd), the new
//                     numbering (a scan over the roots), the merged rows copied as bits
//   k_merge_list_*    step 7: a hash table keyed by (frame, group); pass 1 finds the slot and takes the 64-bit atomicMin of the ordered
//                     key (weight, original index), pass 2 the atomicMin of the list position among the winning object's entries, pass 3
//                     writes.  Which slot a key lands in depends on the schedule; what the slot ends up holding does not.
// No floating-point atomics anywhere; every decision is an integer comparison or a total order.
// Everything lives in buffers of its own (esl_ctx::merge) on the context's stream; the resident graph is only read.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "esl_ctx.hpp"
#include "esl_merge_lattice.hpp"

namespace esl {

static_assert(sizeof(esl_merge_params) == 32, "include/esl.h states this size");
static_assert(sizeof(esl_merge_result) == 48, "include/esl.h states this size");

constexpr int kMergeThreads = 256;
constexpr int kMergeOverlapBlocks = 2048;   // 256 CUs x 8 workgroups of four waves; a wave walks the candidate list with the grid's stride

struct MergeObj {
  double R[9];    // row-major, of the normalised quaternion
  double s[3];    // |half-axes|
  double c[3];
  double vol;
};

enum { MS_NVALID, MS_NPAIRS, MS_NLINKS, MS_CHANGED, MS_NMERGED, MS_LARGEST, MS_NCONFLICTS, MS_COUNT = 8 };

enum { MB_OBJS, MB_LAB, MB_W, MB_REC, MB_GATE, MB_ROWCNT, MB_ROWOFF, MB_CAND, MB_RES, MB_MEAS, MB_SCAL, MB_PROWCNT, MB_PROWOFF, MB_OPAIRS,
       MB_OCNT, MB_OIOU, MB_OCON, MB_COMP, MB_REPKEY, MB_WSUM, MB_GSIZE, MB_ROOT, MB_NEWOFF, MB_NEWIDX, MB_MOBJ, MB_MLAB, MB_MW, MB_OCAM,
       MB_OOBJ, MB_OOUT, MB_SLOT, MB_TAB, MB_COUNT };
using MergeSet = ScratchSet<MB_COUNT>;
struct MergeState { MergeSet set; };

// ---- step 1 ---------------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(kMergeThreads) void k_merge_prep(const double* objs, int M, MergeObj* rec, double4* gate,
                                                                      unsigned long long* scal) {
  const int i = blockIdx.x * kMergeThreads + threadIdx.x;
  if (i >= M) return;
  const double* v = objs + (size_t)i * 10;
  bool ok = true;
  for (int k = 0; k < 10; ++k) ok &= isfinite(v[k]);
  const double nrm = sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6]);
  const double s0 = fabs(v[7]), s1 = fabs(v[8]), s2 = fabs(v[9]);
  ok = ok && isfinite(nrm) && nrm > 0 && s0 > 0 && s1 > 0 && s2 > 0;
  MergeObj o = {};
  double4 g = make_double4(0, 0, 0, -1.0);   // radius < 0: in no pair
  if (ok) {
    const double x = v[3] / nrm, y = v[4] / nrm, z = v[5] / nrm, w = v[6] / nrm;
    o.R[0] = 1 - 2 * (y * y + z * z); o.R[1] = 2 * (x * y - z * w);     o.R[2] = 2 * (x * z + y * w);
    o.R[3] = 2 * (x * y + z * w);     o.R[4] = 1 - 2 * (x * x + z * z); o.R[5] = 2 * (y * z - x * w);
    o.R[6] = 2 * (x * z - y * w);     o.R[7] = 2 * (y * z + x * w);     o.R[8] = 1 - 2 * (x * x + y * y);
    o.s[0] = s0; o.s[1] = s1; o.s[2] = s2;
    o.c[0] = v[0]; o.c[1] = v[1]; o.c[2] = v[2];
    o.vol = 4.0 / 3.0 * M_PI * s0 * s1 * s2;
    g = make_double4(v[0], v[1], v[2], fmax(s0, fmax(s1, s2)));
    atomicAdd(&scal[MS_NVALID], 1ull);
  }
  rec[i] = o;
  gate[i] = g;
}

// ---- step 4: the candidates -------------------------------------------------------------------------------------------------------------
// fill == 0: rowcnt[i] = candidates (i, j > i); fill == 1: the same walk writes them from rowoff[i] on.  ONE kernel for both passes, so
// that both evaluate the gate with the same instructions; the write is bounded by the row's end all the same.
static __global__ __launch_bounds__(kMergeThreads) void k_merge_cand(const double4* gate, const int* lab, int M, int match, int fill,
                                                                      int* rowcnt, const long long* rowoff, int2* cand) {
  __shared__ double4 s_g[kMergeThreads];
  __shared__ int s_l[kMergeThreads];
  const int tid = threadIdx.x, i = blockIdx.x * kMergeThreads + tid;
  const double4 gi = i < M ? gate[i] : make_double4(0, 0, 0, -1.0);
  const int li = i < M ? lab[i] : 0;
  const bool valid_i = gi.w > 0;
  long long pos = 0, end = 0;
  if (fill && i < M) { pos = rowoff[i]; end = rowoff[i + 1]; }
  int cnt = 0;
  for (int j0 = blockIdx.x * kMergeThreads; j0 < M; j0 += kMergeThreads) {
    __syncthreads();
    const int jl = j0 + tid;
    s_g[tid] = jl < M ? gate[jl] : make_double4(0, 0, 0, -1.0);
    s_l[tid] = jl < M ? lab[jl] : 0;
    __syncthreads();
    if (!valid_i) continue;
    for (int jj = 0; jj < kMergeThreads; ++jj) {   // every lane reads the same entry: an LDS broadcast
      const int j = j0 + jj;
      const double4 g = s_g[jj];
      if (j <= i || !(g.w > 0) || (match && s_l[jj] != li)) continue;
      const double dx = gi.x - g.x, dy = gi.y - g.y, dz = gi.z - g.z, rr = gi.w + g.w;
      if (dx * dx + dy * dy + dz * dz <= rr * rr * (1.0 + 1e-9)) {
        if (fill && pos < end) cand[pos++] = make_int2(i, j);
        ++cnt;
      }
    }
  }
  if (!fill && i < M) rowcnt[i] = cnt;
}

// exclusive scan of n <= 65536 counts by one workgroup: out[k] = in[0] + .. + in[k - 1], out[n] = the total
static __global__ __launch_bounds__(1024) void k_merge_scan(const int* in, int n, long long* out) {
  __shared__ long long s[1024];
  const int tid = threadIdx.x, chunk = (n + 1023) / 1024;
  const int b = min(n, tid * chunk), e = min(n, b + chunk);
  long long sum = 0;
  for (int k = b; k < e; ++k) sum += in[k];
  s[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int t = 0; t < 1024; ++t) { const long long v = s[t]; s[t] = run; run += v; }
    out[n] = run;
  }
  __syncthreads();
  long long run = s[tid];
  for (int k = b; k < e; ++k) { out[k] = run; run += in[k]; }
}

// ---- steps 2, 3, 5: one wavefront per candidate -------------------------------------------------------------------------------------------
// q of a lattice point of body `a` in body `b`: x = c_a + R_a (s_a o k / n), q = |diag(1 / s_b) R_b^T (x - c_b)|^2 = |T k + d|^2
static __device__ __forceinline__ double merge_q(const double T[9], const double d[3], double kx, double ky, double kz) {
  const double y0 = T[0] * kx + T[1] * ky + T[2] * kz + d[0];
  const double y1 = T[3] * kx + T[4] * ky + T[5] * kz + d[1];
  const double y2 = T[6] * kx + T[7] * ky + T[8] * kz + d[2];
  return y0 * y0 + y1 * y1 + y2 * y2;
}

static __global__ __launch_bounds__(kMergeThreads) void k_merge_overlap(const MergeObj* rec, const int2* cand, long long n_cand, int n,
                                                                         int n_ball, double min_iou, double min_contain, int4* res,
                                                                         double2* meas, unsigned long long* scal) {
  const int lane = threadIdx.x & 63;
  const long long n_waves = (long long)gridDim.x * (kMergeThreads / 64);
  const MergeStep step = merge_step_of(n, 64);
  const MergeCell cell0 = merge_cell_of(n, lane);
  const int rounds = (merge_lattice_cells(n) + 63) / 64;
  const double inv_n = 1.0 / n;
  int my_pairs = 0, my_links = 0;
  for (long long w = (long long)blockIdx.x * (kMergeThreads / 64) + (threadIdx.x >> 6); w < n_cand; w += n_waves) {
    const int2 pr = cand[w];
    const MergeObj& A = rec[pr.x];
    const MergeObj& B = rec[pr.y];
    double P[9], T1[9], d1[3], T2[9], d2[3];   // P = R_B^T R_A
    const double dc[3] = {A.c[0] - B.c[0], A.c[1] - B.c[1], A.c[2] - B.c[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) P[r * 3 + c] = B.R[r] * A.R[c] + B.R[3 + r] * A.R[3 + c] + B.R[6 + r] * A.R[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double ib = 1.0 / B.s[r], ia = 1.0 / A.s[r];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        T1[r * 3 + c] = P[r * 3 + c] * (A.s[c] * inv_n) * ib;   // samples of A in B's unit ball
        T2[r * 3 + c] = P[c * 3 + r] * (B.s[c] * inv_n) * ia;   // samples of B in A's
      }
      d1[r] = (B.R[r] * dc[0] + B.R[3 + r] * dc[1] + B.R[6 + r] * dc[2]) * ib;
      d2[r] = -(A.R[r] * dc[0] + A.R[3 + r] * dc[1] + A.R[6 + r] * dc[2]) * ia;
    }
    int c1 = 0, c2 = 0;
    MergeCell cell = cell0;
    for (int it = 0; it < rounds; ++it) {   // wave-uniform trip count; a lane past the cube's end is outside the ball
      const bool in = merge_cell_in_ball(n, cell);
      int k[3];
      merge_cell_k(n, cell, k);
      const double kx = (double)k[0], ky = (double)k[1], kz = (double)k[2];
      const double q1 = merge_q(T1, d1, kx, ky, kz), q2 = merge_q(T2, d2, kx, ky, kz);
      c1 += __popcll(__ballot(in && q1 <= 1.0));
      c2 += __popcll(__ballot(in && q2 <= 1.0));
      merge_cell_advance(n, step, cell);
    }
    if (lane == 0) {
      const double Vi = A.vol, Vj = B.vol;
      const double inter = 0.5 * ((double)c1 * Vi + (double)c2 * Vj) / (double)n_ball;
      const double iou = inter / (Vi + Vj - inter), contain = fmin(1.0, inter / fmin(Vi, Vj));
      const bool pair = c1 + c2 > 0, link = pair && (iou >= min_iou || contain >= min_contain);
      res[w] = make_int4(c1, c2, link ? 1 : 0, 0);
      meas[w] = make_double2(iou, contain);
      my_pairs += pair ? 1 : 0; my_links += link ? 1 : 0;
    }
  }
  if (lane == 0) {   // one integer atomic pair per wave
    if (my_pairs) atomicAdd(&scal[MS_NPAIRS], (unsigned long long)my_pairs);
    if (my_links) atomicAdd(&scal[MS_NLINKS], (unsigned long long)my_links);
  }
}

// esl_map_overlaps: the overlapping pairs of row i, counted (fill == 0) or written from prowoff[i] on, the first `cap` of the list only
static __global__ __launch_bounds__(kMergeThreads) void k_merge_rows(const int2* cand, const int4* res, const double2* meas,
                                                                      const long long* rowoff, int M, int fill, int* prowcnt,
                                                                      const long long* prowoff, long long cap, int2* o_pairs, int2* o_cnt,
                                                                      double* o_iou, double* o_con) {
  const int i = blockIdx.x * kMergeThreads + threadIdx.x;
  if (i >= M) return;
  long long pos = fill ? prowoff[i] : 0;
  int cnt = 0;
  for (long long e = rowoff[i]; e < rowoff[i + 1]; ++e) {
    const int4 r = res[e];
    if (r.x + r.y <= 0) continue;
    if (fill && pos < cap) {
      o_pairs[pos] = cand[e]; o_cnt[pos] = make_int2(r.x, r.y);
      const double2 m = meas[e];
      o_iou[pos] = m.x; o_con[pos] = m.y;
    }
    ++pos; ++cnt;
  }
  if (!fill) prowcnt[i] = cnt;
}

// ---- step 5: components -----------------------------------------------------------------------------------------------------------------
// invariant: comp[x] <= x and comp[x] is a member of x's component
static __global__ __launch_bounds__(kMergeThreads) void k_merge_iota(int* comp, int M) {
  const int i = blockIdx.x * kMergeThreads + threadIdx.x;
  if (i < M) comp[i] = i;
}
static __global__ __launch_bounds__(kMergeThreads) void k_merge_hook(const int2* cand, const int4* res, long long n_cand, int* comp,
                                                                      unsigned long long* scal) {
  const long long stride = (long long)gridDim.x * kMergeThreads;
  for (long long e = (long long)blockIdx.x * kMergeThreads + threadIdx.x; e < n_cand; e += stride) {
    if (!res[e].z) continue;
    const int2 pr = cand[e];
    const int a = comp[pr.x], b = comp[pr.y];
    if (a != b) {
      atomicMin(&comp[max(a, b)], min(a, b));
      scal[MS_CHANGED] = 1;
    }
  }
}
static __global__ __launch_bounds__(kMergeThreads) void k_merge_jump(int* comp, int M) {
  const int i = blockIdx.x * kMergeThreads + threadIdx.x;
  if (i >= M) return;
  int c = comp[i];
  for (int p = comp[c]; p != c; p = comp[c]) c = p;   // strictly decreasing: ends at a root; roots do not move in this kernel
  comp[i] = c;
}

// ---- step 6: groups -----------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(kMergeThreads) void k_merge_fill(int* w, int M, int v) {
  const int i = blockIdx.x * kMergeThreads + threadIdx.x;
  if (i < M) w[i] = v;
}
static __global__ __launch_bounds__(kMergeThreads) void k_merge_list_count(const int* obj, long long n_obs, int* w) {
  const long long e = (long long)blockIdx.x * kMergeThreads + threadIdx.x;
  if (e < n_obs && obj[e] >= 0) atomicAdd(&w[obj[e]], 1);
}
static __global__ __launch_bounds__(kMergeThreads) void k_merge_group_acc(const int* comp, const int* w, int M, unsigned long long* repkey,
                                                                           int* wsum, int* gsize) {
  const int i = blockIdx.x * kMergeThreads + threadIdx.x;
  if (i >= M) return;
  const int g = comp[i];
  atomicMax(&repkey[g], (unsigned long long)merge_rep_key(w[i], i));
  atomicAdd(&wsum[g], w[i]);
  atomicAdd(&gsize[g], 1);
}
static __global__ __launch_bounds__(kMergeThreads) void k_merge_group_roots(const int* comp, const int* gsize, int M, int* isroot,
                                                                             unsigned long long* scal) {
  const int i = blockIdx.x * kMergeThreads + threadIdx.x;
  if (i >= M) return;
  const int r = comp[i] == i ? 1 : 0;
  isroot[i] = r;
  if (r) {
    if (gsize[i] > 1) atomicAdd(&scal[MS_NMERGED], 1ull);
    atomicMax(&scal[MS_LARGEST], (unsigned long long)gsize[i]);
  }
}
static __global__ __launch_bounds__(kMergeThreads) void k_merge_group_write(const int* comp, const int* isroot, const long long* newoff,
                                                                             const unsigned long long* repkey, const int* wsum,
                                                                             const double* objs, const int* lab, int M, int* newidx,
                                                                             double* mobjs, int* mlab, int* mw) {
  const int i = blockIdx.x * kMergeThreads + threadIdx.x;
  if (i >= M) return;
  newidx[i] = (int)newoff[comp[i]];
  if (!isroot[i]) return;
  const int g = (int)newoff[i], rep = merge_rep_key_index(repkey[i]);
  const unsigned long long* src = (const unsigned long long*)(objs + (size_t)rep * 10);   // as bits: a NaN row stays what it was
  unsigned long long* dst = (unsigned long long*)(mobjs + (size_t)g * 10);
  for (int k = 0; k < 10; ++k) dst[k] = src[k];
  mlab[g] = lab[rep]; mw[g] = wsum[i];
}

// ---- step 7: the edge list ------------------------------------------------------------------------------------------------------------------
constexpr unsigned long long kMergeEmpty = ~0ull;
static __global__ __launch_bounds__(kMergeThreads) void k_merge_list_p1(const int* cam, const int* obj, long long n_obs, const int* comp,
                                                                         const int* w, unsigned long long mask, unsigned long long* keys,
                                                                         unsigned long long* val1, unsigned int* slot_of) {
  const long long e = (long long)blockIdx.x * kMergeThreads + threadIdx.x;
  if (e >= n_obs) return;
  const int o = obj[e];
  if (o < 0) return;
  const unsigned long long key = merge_slot_key(cam[e], comp[o]);
  unsigned long long h = merge_slot_hash(key) & mask;
  for (;;) {   // at most half of the slots are ever taken
    const unsigned long long prev = atomicCAS(&keys[h], kMergeEmpty, key);
    if (prev == kMergeEmpty || prev == key) break;
    h = (h + 1) & mask;
  }
  slot_of[e] = (unsigned int)h;
  atomicMin(&val1[h], (unsigned long long)merge_conflict_key(w[o], o));
}
static __global__ __launch_bounds__(kMergeThreads) void k_merge_list_p2(const int* obj, long long n_obs, const unsigned int* slot_of,
                                                                         const unsigned long long* val1, unsigned long long* val2) {
  const long long e = (long long)blockIdx.x * kMergeThreads + threadIdx.x;
  if (e >= n_obs) return;
  const int o = obj[e];
  if (o < 0) return;
  const unsigned int h = slot_of[e];
  if (merge_conflict_key_index(val1[h]) == o) atomicMin(&val2[h], (unsigned long long)e);
}
static __global__ __launch_bounds__(kMergeThreads) void k_merge_list_p3(const int* obj, long long n_obs, const unsigned int* slot_of,
                                                                         const unsigned long long* val1, const unsigned long long* val2,
                                                                         const int* newidx, int* out, unsigned long long* scal) {
  const long long e = (long long)blockIdx.x * kMergeThreads + threadIdx.x;
  bool lost = false;
  if (e < n_obs) {
    const int o = obj[e];
    int v = -1;
    if (o >= 0) {
      const unsigned int h = slot_of[e];
      if (merge_conflict_key_index(val1[h]) == o && val2[h] == (unsigned long long)e) v = newidx[o];
      else lost = true;
    }
    out[e] = v;
  }
  const unsigned long long m = __ballot(lost);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&scal[MS_NCONFLICTS], (unsigned long long)__popcll(m));
}

void merge_scratch_stats(const esl_ctx* c, int64_t* allocs, int64_t* bytes) {
  if (c->merge) { *allocs = c->merge->set.allocs(); *bytes = (int64_t)c->merge->set.held(); }
}

void merge_release(esl_ctx* c) {   // called by esl_ctx_destroy
  if (c->merge) c->merge->set.release();
  delete c->merge;
  c->merge = nullptr;
}

}  // namespace esl

using namespace esl;

namespace {

unsigned blocks_of(long long n) { return (unsigned)((n + kMergeThreads - 1) / kMergeThreads); }

// what both calls share: parameters, the source of the map
int merge_check(esl_ctx* c, const double* objs, const int32_t* labels, int M, const esl_merge_params* pp, const char* who,
                esl_merge_params& p) {
  const std::string w(who);
  if (!c || M < 0) { set_error(w + ": bad argument (null context or negative count)"); return ESL_ERR_INVALID; }
  if (M > kMergeMaxObjects) { set_error(w + ": M > 65536"); return ESL_ERR_INVALID; }
  if (M > 0 && !labels) { set_error(w + ": null labels"); return ESL_ERR_INVALID; }
  if (pp) p = *pp; else esl_merge_params_default(&p);
  if (p.lattice < kMergeLatticeMin || p.lattice > kMergeLatticeMax) { set_error(w + ": lattice outside 4..32"); return ESL_ERR_INVALID; }
  if (!std::isfinite(p.min_iou) || !(p.min_iou > 0) || p.min_iou > 1) { set_error(w + ": min_iou outside (0, 1]"); return ESL_ERR_INVALID; }
  if (!std::isfinite(p.min_contain) || !(p.min_contain > 0)) { set_error(w + ": min_contain not finite or <= 0"); return ESL_ERR_INVALID; }
  if (p.max_pairs < 0) { set_error(w + ": negative max_pairs"); return ESL_ERR_INVALID; }
  return resident_source_check(c, who, false, 0, !objs && M > 0, M);
}

struct MergeFront {          // what steps 1 - 5 leave on the device
  const double* objs; const int* lab;
  long long n_cand; int n_valid; bool over;   // over: n_cand > max_pairs, nothing after the count has run
  unsigned long long* scal;
};

// steps 1 - 5 up to the candidates' integers and measures.  M > 0.
int merge_front(esl_ctx* c, MergeSet& s, const double* objs, const int32_t* labels, int M, const esl_merge_params& p, MergeFront& f) {
  if (const int rc = source(c, s, MB_OBJS, objs, c->objs, (size_t)M * 10 * sizeof(double), &f.objs)) return rc;
  if (const int rc = upload(c, s, MB_LAB, labels, (size_t)M * sizeof(int32_t), &f.lab)) return rc;
  if (const int rc = s.grow(c, MB_REC, (size_t)M * sizeof(MergeObj))) return rc;
  if (const int rc = s.grow(c, MB_GATE, (size_t)M * sizeof(double4))) return rc;
  if (const int rc = s.grow(c, MB_ROWCNT, (size_t)M * sizeof(int))) return rc;
  if (const int rc = s.grow(c, MB_ROWOFF, (size_t)(M + 1) * sizeof(long long))) return rc;
  if (const int rc = s.grow(c, MB_SCAL, MS_COUNT * sizeof(unsigned long long))) return rc;
  f.scal = s.at<unsigned long long>(MB_SCAL);
  ESL_HIP_TRY(hipMemsetAsync(f.scal, 0, MS_COUNT * sizeof(unsigned long long), c->stream));
  MergeObj* rec = s.at<MergeObj>(MB_REC);
  double4* gate = s.at<double4>(MB_GATE);
  int* rowcnt = s.at<int>(MB_ROWCNT);
  long long* rowoff = s.at<long long>(MB_ROWOFF);
  const unsigned mb = blocks_of(M);
  {
    ProfScope ps(c, 4);
    hipLaunchKernelGGL(k_merge_prep, dim3(mb), dim3(kMergeThreads), 0, c->stream, f.objs, M, rec, gate, f.scal);
    hipLaunchKernelGGL(k_merge_cand, dim3(mb), dim3(kMergeThreads), 0, c->stream, gate, f.lab, M, p.match_labels != 0 ? 1 : 0, 0, rowcnt,
                       rowoff, (int2*)nullptr);
    hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(1024), 0, c->stream, rowcnt, M, rowoff);
  }
  ESL_HIP_TRY(hipGetLastError());
  long long n_cand = 0; unsigned long long n_valid = 0;
  ESL_HIP_TRY(hipMemcpyAsync(&n_cand, rowoff + M, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(&n_valid, f.scal + MS_NVALID, sizeof(n_valid), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  f.n_cand = n_cand; f.n_valid = (int)n_valid; f.over = n_cand > (long long)p.max_pairs;
  if (f.over || n_cand == 0) return ESL_OK;
  if (const int rc = s.grow(c, MB_CAND, (size_t)n_cand * sizeof(int2))) return rc;
  if (const int rc = s.grow(c, MB_RES, (size_t)n_cand * sizeof(int4))) return rc;
  if (const int rc = s.grow(c, MB_MEAS, (size_t)n_cand * sizeof(double2))) return rc;
  const int n = p.lattice;
  const unsigned ob = (unsigned)std::min<long long>((n_cand + 3) / 4, kMergeOverlapBlocks);
  {
    ProfScope ps(c, 4);
    hipLaunchKernelGGL(k_merge_cand, dim3(mb), dim3(kMergeThreads), 0, c->stream, gate, f.lab, M, p.match_labels != 0 ? 1 : 0, 1, rowcnt,
                       rowoff, s.at<int2>(MB_CAND));
    hipLaunchKernelGGL(k_merge_overlap, dim3(ob), dim3(kMergeThreads), 0, c->stream, rec, s.at<const int2>(MB_CAND), n_cand, n,
                       merge_lattice_count(n), p.min_iou, p.min_contain, s.at<int4>(MB_RES), s.at<double2>(MB_MEAS), f.scal);
  }
  ESL_HIP_TRY(hipGetLastError());
  return ESL_OK;
}

}  // namespace

extern "C" void esl_merge_params_default(esl_merge_params* p) {
  if (!p) return;
  p->lattice = 16; p->match_labels = 1; p->min_iou = 0.3; p->min_contain = 0.7; p->max_pairs = 4194304; p->pad = 0;
}

extern "C" int esl_map_overlaps(esl_ctx* c, const double* objs, const int32_t* labels, int32_t M, const esl_merge_params* pp, int64_t cap,
                                int32_t* pairs_out, int32_t* counts_out, double* iou_out, double* contain_out, int64_t* n_pairs,
                                int64_t* n_candidates) {
  esl_merge_params p;
  if (const int rc = merge_check(c, objs, labels, M, pp, "esl_map_overlaps", p)) return rc;
  if (cap < 0 || !n_pairs || !n_candidates || (cap > 0 && (!pairs_out || !counts_out || !iou_out || !contain_out))) {
    set_error("esl_map_overlaps: negative cap or null output");
    return ESL_ERR_INVALID;
  }
  *n_pairs = 0; *n_candidates = 0;
  if (M == 0) return ESL_OK;
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (!c->merge) c->merge = new MergeState();
  MergeSet& s = c->merge->set;
  MergeFront f;
  if (const int rc = merge_front(c, s, objs, labels, M, p, f)) return rc;
  *n_candidates = f.n_cand;
  if (f.over) { *n_pairs = -1; return ESL_OK; }   // more candidates than max_pairs: not computed
  if (f.n_cand == 0) return ESL_OK;
  const long long wcap = std::min<long long>(cap, f.n_cand);
  if (const int rc = s.grow(c, MB_PROWCNT, (size_t)M * sizeof(int))) return rc;
  if (const int rc = s.grow(c, MB_PROWOFF, (size_t)(M + 1) * sizeof(long long))) return rc;
  if (const int rc = s.grow(c, MB_OPAIRS, (size_t)wcap * sizeof(int2))) return rc;
  if (const int rc = s.grow(c, MB_OCNT, (size_t)wcap * sizeof(int2))) return rc;
  if (const int rc = s.grow(c, MB_OIOU, (size_t)wcap * sizeof(double))) return rc;
  if (const int rc = s.grow(c, MB_OCON, (size_t)wcap * sizeof(double))) return rc;
  int* prowcnt = s.at<int>(MB_PROWCNT);
  long long* prowoff = s.at<long long>(MB_PROWOFF);
  const unsigned mb = blocks_of(M);
  {
    ProfScope ps(c, 4);
    for (int fill = 0; fill < 2; ++fill) {
      hipLaunchKernelGGL(k_merge_rows, dim3(mb), dim3(kMergeThreads), 0, c->stream, s.at<const int2>(MB_CAND), s.at<const int4>(MB_RES),
                         s.at<const double2>(MB_MEAS), s.at<const long long>(MB_ROWOFF), M, fill, prowcnt, prowoff, wcap,
                         s.at<int2>(MB_OPAIRS), s.at<int2>(MB_OCNT), s.at<double>(MB_OIOU), s.at<double>(MB_OCON));
      if (!fill) hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(1024), 0, c->stream, prowcnt, M, prowoff);
    }
  }
  ESL_HIP_TRY(hipGetLastError());
  long long np = 0;
  ESL_HIP_TRY(hipMemcpyAsync(&np, prowoff + M, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  *n_pairs = np;
  const size_t nw = (size_t)std::min<long long>(np, wcap);
  if (nw) {
    ESL_HIP_TRY(hipMemcpyAsync(pairs_out, s.buf[MB_OPAIRS], nw * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(counts_out, s.buf[MB_OCNT], nw * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(iou_out, s.buf[MB_OIOU], nw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(contain_out, s.buf[MB_OCON], nw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return ESL_OK;
}

extern "C" int esl_map_merge(esl_ctx* c, const double* objs, const int32_t* labels, const int32_t* weights, int32_t M,
                             const int32_t* obs_cam, const int32_t* obs_obj, int64_t n_obs, const esl_merge_params* pp, int32_t* group_out,
                             int32_t* new_index_out, double* merged_objs_out, int32_t* merged_labels_out, int32_t* merged_weights_out,
                             int32_t* obs_obj_out, esl_merge_result* out) {
  esl_merge_params p;
  if (const int rc = merge_check(c, objs, labels, M, pp, "esl_map_merge", p)) return rc;
  if (!out || n_obs < 0 || (n_obs > 0 && (!obs_cam || !obs_obj)) ||
      (M > 0 && (!group_out || !new_index_out || !merged_objs_out || !merged_labels_out || !merged_weights_out))) {
    set_error("esl_map_merge: null pointer or negative n_obs");
    return ESL_ERR_INVALID;
  }
  if (n_obs >= (1ll << 31)) { set_error("esl_map_merge: n_obs >= 2^31"); return ESL_ERR_INVALID; }
  if (weights) {
    long long tot = 0;
    for (int i = 0; i < M; ++i) {
      if (weights[i] < 0) { set_error("esl_map_merge: negative weight"); return ESL_ERR_INVALID; }
      tot += weights[i];
    }
    if (tot >= (1ll << 31)) { set_error("esl_map_merge: the weights' total is >= 2^31"); return ESL_ERR_INVALID; }
  }
  for (int64_t e = 0; e < n_obs; ++e) {
    if (obs_obj[e] < 0) continue;
    if (obs_obj[e] >= M) { set_error("esl_map_merge: obs_obj >= M"); return ESL_ERR_INVALID; }
    if (obs_cam[e] < 0) { set_error("esl_map_merge: negative obs_cam"); return ESL_ERR_INVALID; }
  }
  std::memset(out, 0, sizeof(*out));
  if (M == 0) {
    if (obs_obj_out) for (int64_t e = 0; e < n_obs; ++e) obs_obj_out[e] = -1;   // only skipped entries can exist
    return ESL_OK;
  }
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (!c->merge) c->merge = new MergeState();
  MergeSet& s = c->merge->set;
  MergeFront f;
  if (const int rc = merge_front(c, s, objs, labels, M, p, f)) return rc;
  out->n_valid = f.n_valid; out->n_candidates = f.n_cand;
  if (f.over) {   // status 3: the map as it came, every object its own group
    out->status = 3; out->n_groups = M; out->largest_group = 1;
    if (objs) std::memcpy(merged_objs_out, objs, (size_t)M * 10 * sizeof(double));
    else {
      ESL_HIP_TRY(hipMemcpyAsync(merged_objs_out, c->objs, (size_t)M * 10 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < M; ++i) {
      group_out[i] = i; new_index_out[i] = i; merged_labels_out[i] = labels[i];
      merged_weights_out[i] = weights ? weights[i] : (n_obs > 0 ? 0 : 1);
    }
    for (int64_t e = 0; e < n_obs; ++e) {
      if (!weights && obs_obj[e] >= 0) ++merged_weights_out[obs_obj[e]];
      if (obs_obj_out) obs_obj_out[e] = obs_obj[e] < 0 ? -1 : obs_obj[e];
    }
    return ESL_OK;
  }
  const unsigned mb = blocks_of(M);
  const size_t mi = (size_t)M * sizeof(int);
  for (int k : {MB_W, MB_COMP, MB_WSUM, MB_GSIZE, MB_ROOT, MB_NEWIDX, MB_MLAB, MB_MW})
    if (const int rc = s.grow(c, k, mi)) return rc;
  if (const int rc = s.grow(c, MB_REPKEY, (size_t)M * sizeof(unsigned long long))) return rc;
  if (const int rc = s.grow(c, MB_NEWOFF, (size_t)(M + 1) * sizeof(long long))) return rc;
  if (const int rc = s.grow(c, MB_MOBJ, (size_t)M * 10 * sizeof(double))) return rc;
  unsigned long long slots = 64;
  if (n_obs > 0) {
    while (slots < 2ull * (unsigned long long)n_obs) slots <<= 1;
    const size_t ob = (size_t)n_obs * sizeof(int);
    for (int k : {MB_OCAM, MB_OOBJ, MB_OOUT, MB_SLOT})
      if (const int rc = s.grow(c, k, ob)) return rc;
    if (const int rc = s.grow(c, MB_TAB, (size_t)slots * 3 * sizeof(unsigned long long))) return rc;
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[MB_OCAM], obs_cam, ob, hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[MB_OOBJ], obs_obj, ob, hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemsetAsync(s.buf[MB_TAB], 0xff, (size_t)slots * 3 * sizeof(unsigned long long), c->stream));
  }
  int* w = s.at<int>(MB_W);
  int* comp = s.at<int>(MB_COMP);
  const int* o_cam = s.at<const int>(MB_OCAM);
  const int* o_obj = s.at<const int>(MB_OOBJ);
  const unsigned eb = blocks_of(n_obs);
  // weights: given, the objects' list entries, or 1
  if (weights) ESL_HIP_TRY(hipMemcpyAsync(w, weights, mi, hipMemcpyHostToDevice, c->stream));
  {
    ProfScope ps(c, 4);
    if (!weights) {
      hipLaunchKernelGGL(k_merge_fill, dim3(mb), dim3(kMergeThreads), 0, c->stream, w, M, n_obs > 0 ? 0 : 1);
      if (n_obs > 0) hipLaunchKernelGGL(k_merge_list_count, dim3(eb), dim3(kMergeThreads), 0, c->stream, o_obj, (long long)n_obs, w);
    }
    hipLaunchKernelGGL(k_merge_iota, dim3(mb), dim3(kMergeThreads), 0, c->stream, comp, M);
  }
  ESL_HIP_TRY(hipGetLastError());
  // components: a round hooks and compresses; the last round finds nothing to hook
  if (f.n_cand > 0) {
    const unsigned hb = (unsigned)std::min<long long>(blocks_of(f.n_cand), 4096);
    for (int round = 0; round <= M; ++round) {
      unsigned long long changed = 0;
      ESL_HIP_TRY(hipMemsetAsync(f.scal + MS_CHANGED, 0, sizeof(unsigned long long), c->stream));
      {
        ProfScope ps(c, 4);
        hipLaunchKernelGGL(k_merge_hook, dim3(hb), dim3(kMergeThreads), 0, c->stream, s.at<const int2>(MB_CAND),
                           s.at<const int4>(MB_RES), f.n_cand, comp, f.scal);
        hipLaunchKernelGGL(k_merge_jump, dim3(mb), dim3(kMergeThreads), 0, c->stream, comp, M);
      }
      ESL_HIP_TRY(hipGetLastError());
      ESL_HIP_TRY(hipMemcpyAsync(&changed, f.scal + MS_CHANGED, sizeof(changed), hipMemcpyDeviceToHost, c->stream));
      ESL_HIP_TRY(hipStreamSynchronize(c->stream));
      if (!changed) break;
    }
  }
  ESL_HIP_TRY(hipMemsetAsync(s.buf[MB_REPKEY], 0, (size_t)M * sizeof(unsigned long long), c->stream));
  ESL_HIP_TRY(hipMemsetAsync(s.buf[MB_WSUM], 0, mi, c->stream));
  ESL_HIP_TRY(hipMemsetAsync(s.buf[MB_GSIZE], 0, mi, c->stream));
  {
    ProfScope ps(c, 4);
    hipLaunchKernelGGL(k_merge_group_acc, dim3(mb), dim3(kMergeThreads), 0, c->stream, comp, w, M, s.at<unsigned long long>(MB_REPKEY),
                       s.at<int>(MB_WSUM), s.at<int>(MB_GSIZE));
    hipLaunchKernelGGL(k_merge_group_roots, dim3(mb), dim3(kMergeThreads), 0, c->stream, comp, s.at<const int>(MB_GSIZE), M,
                       s.at<int>(MB_ROOT), f.scal);
    hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(1024), 0, c->stream, s.at<const int>(MB_ROOT), M, s.at<long long>(MB_NEWOFF));
    hipLaunchKernelGGL(k_merge_group_write, dim3(mb), dim3(kMergeThreads), 0, c->stream, comp, s.at<const int>(MB_ROOT),
                       s.at<const long long>(MB_NEWOFF), s.at<const unsigned long long>(MB_REPKEY), s.at<const int>(MB_WSUM),
                       f.objs, f.lab, M, s.at<int>(MB_NEWIDX), s.at<double>(MB_MOBJ), s.at<int>(MB_MLAB), s.at<int>(MB_MW));
    if (n_obs > 0) {
      unsigned long long* keys = s.at<unsigned long long>(MB_TAB);
      unsigned long long* val1 = keys + slots;
      unsigned long long* val2 = val1 + slots;
      unsigned int* slot_of = s.at<unsigned int>(MB_SLOT);
      hipLaunchKernelGGL(k_merge_list_p1, dim3(eb), dim3(kMergeThreads), 0, c->stream, o_cam, o_obj, (long long)n_obs, comp, w, slots - 1,
                         keys, val1, slot_of);
      hipLaunchKernelGGL(k_merge_list_p2, dim3(eb), dim3(kMergeThreads), 0, c->stream, o_obj, (long long)n_obs, slot_of, val1, val2);
      hipLaunchKernelGGL(k_merge_list_p3, dim3(eb), dim3(kMergeThreads), 0, c->stream, o_obj, (long long)n_obs, slot_of, val1, val2,
                         s.at<const int>(MB_NEWIDX), s.at<int>(MB_OOUT), f.scal);
    }
  }
  ESL_HIP_TRY(hipGetLastError());
  unsigned long long sc[MS_COUNT];
  long long n_groups = 0;
  ESL_HIP_TRY(hipMemcpyAsync(sc, f.scal, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(&n_groups, s.at<long long>(MB_NEWOFF) + M, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(group_out, comp, mi, hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(new_index_out, s.buf[MB_NEWIDX], mi, hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t G = (size_t)n_groups;
  ESL_HIP_TRY(hipMemcpyAsync(merged_objs_out, s.buf[MB_MOBJ], G * 10 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(merged_labels_out, s.buf[MB_MLAB], G * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(merged_weights_out, s.buf[MB_MW], G * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (n_obs > 0 && obs_obj_out)
    ESL_HIP_TRY(hipMemcpyAsync(obs_obj_out, s.buf[MB_OOUT], (size_t)n_obs * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  out->status = 0; out->n_groups = (int32_t)n_groups; out->n_merged_groups = (int32_t)sc[MS_NMERGED];
  out->largest_group = (int32_t)sc[MS_LARGEST]; out->n_conflicts = (int32_t)sc[MS_NCONFLICTS];
  out->n_pairs = (int64_t)sc[MS_NPAIRS]; out->n_links = (int64_t)sc[MS_NLINKS];
  return ESL_OK;
}
