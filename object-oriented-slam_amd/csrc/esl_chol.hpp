// esl_chol.hpp — dense fp64 Cholesky (lower, column-major, in place) + solve for the reduced camera
// system of SLAM mode, written for gfx950: FP64 MFMA (v_mfma_f64_16x16x4_f64) for the panel solve
// and the trailing rank-NB update, LDS for the diagonal block.
//
// Replaces g2o's LinearSolverDense (Thirdparty/g2o/g2o/solvers/linear_solver_dense.h:65-113:
// Eigen::LDLT of the dense matrix, "ok" iff positive) on the Schur-reduced system that
// BlockSolver::solve forms (core/block_solver.hpp:367-486).
//
// Layout: M is (n+1) x n, column-major, leading dimension lda >= n+1.  Rows 0..n-1 hold the lower
// triangle of S; row n holds b^T.  Factoring the augmented matrix leaves y = L^-1 b in row n (the
// forward substitution rides along in the panel solve), so only the backward substitution
// L^T x = y is separate.
//
// Blocked right-looking, NB = 128:
//   k_potrf2  one workgroup: diagonal block -> L11 in registers / LDS, then Linv = L11^-1 (in-place, recursive doubling)
//   k_panel   P <- P * Linv^T           (rows below the diagonal block; MFMA, X*Y^T form)
//   k_update  C <- C - P_i * P_j^T      (lower-triangle tiles of the trailing matrix; MFMA)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "esl_chol_kernels.hpp"
#include "esl_chol_plan.hpp"
#include "esl_chol_persist.hpp"

namespace esl {

// Distributed form (one process per GPU; SURVEY.md section 8 e).  Outer panel o (W x 128 columns) belongs to rank o mod R.
// Every rank holds the full-size matrix, but only the columns of ITS outer panels are kept up to date: the owner factors
// its panel (diagonal blocks, panel solves, inner updates), broadcasts the factored columns (+ the inverses of the diagonal
// blocks for the back-substitution), and every rank applies the rank-(W x 128) update to its own later panels only --
// n^3 / (3 R) flops per rank instead of the replicated n^3 / 3.  After the last panel every rank holds the whole factor,
// so the O(n^2) back-substitution runs replicated and all ranks end with the same x, bit for bit.
struct CholDist {
  int rank = 0, n_ranks = 1;
  void* user = nullptr;
  int (*bcast)(void* user, double* dev, size_t count, int root) = nullptr;   // on the factorisation's stream
  // staging buffer of chol_pack_len(n) doubles: a factored outer panel travels as ONE message holding its rows from the diagonal
  // down (+ the right-hand side's row) and the inverses of its diagonal blocks -- half of the whole-column volume on average.
  // Null: whole columns and the inverses in two messages.
  double* pack = nullptr;
  // OVERLAPPED form (round 3): a second staging buffer and a broadcast that takes the stream to run on.  The messages then travel
  // on their own stream: the owner of panel o + 1 brings it up to date with panel o FIRST, factors and packs it, and its message is
  // on the wire while every rank is still applying panel o to the rest of its panels (the single-GPU look-ahead carried over).
  double* pack2 = nullptr;
  int (*bcast_on)(void* user, double* dev, size_t count, int root, hipStream_t stream) = nullptr;
};
inline int chol_outer_panels(int n);
inline size_t chol_pack_len(int n) { const size_t w = (size_t)chol_outer_panels(n) * kNB; return ((size_t)n + 1) * w + w * kNB; }
inline int chol_outer_panels(int n) { return (n >= 8192) ? 4 : 2; }   // inner 128-panels per outer panel

// ---- the runtime switches of the dense solver: ONE table, filled from the environment once per context ------------------------------
// (chol_set_attributes, i.e. at the context's first factorisation; esl_debug_chol_plan fills a fresh one per call).  Product: changes
// what a user runs.  A/B: selects the other of two forms that must agree (tests and committed scripts compare them).  Debugging:
// tuning and diagnostics.  ESL_CHOL_DIST / ESL_CHOL_DIST_OVERLAP change the collective sequence and are read once per COMMUNICATOR
// (esl_comm.hip, esl_ctx::sw_chol_dist / sw_chol_overlap), not here.
struct CholSwitches {
  int persistent = 2;            // ESL_CHOL_PERSISTENT = 1 / 0: k_chol_persist at every size / never; unset (2): by size.  A/B; 0 is also the fallback after a hand-off timeout
  bool small = true;             // ESL_CHOL_SMALL=0: orders <= 248 on the blocked path too instead of k_chol_small.  A/B
  bool backsub_launches = false; // ESL_CHOL_BACKSUB_LAUNCHES=1: the launch-per-panel back-substitution instead of k_chol_backsub.  A/B; also the fallback
  bool upd_v = true;             // ESL_UPD_V=0: the big rank-K launches on k_chol_update_lds<256, 128> instead of k_chol_update_v (same bits).  A/B
  bool fuse = true;              // ESL_CHOL_FUSE=0: strips under the diagonal block and the next block's update as worker tasks (first form of round 4).  A/B
  int merge = 0;                 // ESL_CHOL_MERGE = 1 .. 16: far updates of a tile per visit; unset (0): 3 from n = 16,384, else 2 (chol_merge_for).  A/B
  bool strips = false;           // ESL_CHOL_STRIPS=1: the strips of a row tile away from the diagonal as one task (measured slower).  A/B
  int special = 2;               // ESL_CHOL_SPECIAL = 1 .. 8: leading column panels of an outer panel with special chain tiles (chol_tile_special).  A/B
  int W = 0;                     // ESL_CHOL_W: outer-panel width of the persistent form; unset (0): chol_outer_panels(n).  Debugging
  int filler = 128;              // ESL_CHOL_FILLER: far-update tasks interleaved per chain-dependent group of the task list.  Debugging
  int timeout_ms = 0;            // ESL_CHOL_TIMEOUT_MS: bound of k_chol_persist's spins; unset (0): 3 s.  Debugging
  bool timing = false;           // ESL_CHOL_TIMING (set at all): the kernels' diagnostics on, the self test prints chol_print_timing.  Debugging
  bool debug = false;            // ESL_CHOL_DEBUG (set at all): the self test creates and destroys a stream while the factorisation runs.  Debugging
  bool upd_v_cap = false;        // ESL_UPD_V_CAP=1: EVERY k_chol_update_v launch with one workgroup per CU (kCholLdsVCap): the update alone at half occupancy.  Debugging
};
inline CholSwitches chol_switches_from_env() {
  CholSwitches s;
  auto clamp = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
  if (const char* e = std::getenv("ESL_CHOL_PERSISTENT")) s.persistent = e[0] == '1' ? 1 : 0;
  if (const char* e = std::getenv("ESL_CHOL_SMALL")) s.small = e[0] != '0';
  if (const char* e = std::getenv("ESL_CHOL_BACKSUB_LAUNCHES")) s.backsub_launches = e[0] == '1';
  if (const char* e = std::getenv("ESL_UPD_V")) s.upd_v = std::atoi(e) != 0;
  if (const char* e = std::getenv("ESL_CHOL_FUSE")) s.fuse = e[0] != '0';
  if (const char* e = std::getenv("ESL_CHOL_MERGE")) s.merge = clamp(std::atoi(e), 1, 16);
  if (const char* e = std::getenv("ESL_CHOL_STRIPS")) s.strips = e[0] == '1';
  if (const char* e = std::getenv("ESL_CHOL_SPECIAL")) s.special = clamp(std::atoi(e), 1, 8);
  if (const char* e = std::getenv("ESL_CHOL_W")) s.W = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("ESL_CHOL_FILLER")) s.filler = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("ESL_CHOL_TIMEOUT_MS")) s.timeout_ms = std::max(1, std::atoi(e));
  s.timing = std::getenv("ESL_CHOL_TIMING") != nullptr;
  s.debug = std::getenv("ESL_CHOL_DEBUG") != nullptr;
  if (const char* e = std::getenv("ESL_UPD_V_CAP")) s.upd_v_cap = e[0] == '1';
  return s;
}

// would chol_launch_update take the k_chol_update_v path for this region?  (The only path that can ASSIGN C = -P P^T instead of updating C.)
inline bool chol_update_v_applies(const CholSwitches& sw, long lda, long rows, long base, long col_limit, bool ext, long ldp) {
  const long nrows = rows - base, nc = col_limit - base;
  if (nrows <= 0 || nc <= 0) return false;
  const bool whole = (nc >= nrows - 1);
  const long big_tiles = ((nrows + 255) / 256) * ((nc + 127) / 128) / (whole ? 2 : 1);
  return big_tiles >= 1024 && sw.upd_v && (lda & 1) == 0 && (base & 1) == 0 && (!ext || (ldp & 1) == 0);
}
// Occupancy cap of k_chol_update_v (`cap` below): the launch asks for more than half of a CU's 160 KB of LDS, so ONE of its four-wave
// workgroups fits a CU instead of two, and half of every SIMD's registers stays free for the waves of a streaming kernel on another
// stream (esl_slam.hip: the segments' products beside the rank-K update).  The kernel's code does not change: it uses the first
// kCholLdsV bytes as before.  Alone, the capped rank-3,744 update of C4 takes 17.75 instead of 16.17 ms.
constexpr size_t kCholLdsVCap = 84 * 1024;
static_assert(2 * kCholLdsVCap > 160 * 1024 && kCholLdsVCap >= kCholLdsV, "one capped workgroup per CU");
// C[base.., base..col_limit) -= P P^T on the lower triangle of the (rows x *) matrix M; P = columns [kcol0, kcol0 + K) of M, or
// Pext (rows x K, leading dimension ldp) when given.  Needs chol_set_attributes() on the current device first.
// part (optional, with Pext and base = 0): workspace of kCholMaxSplit x lda x col_limit doubles -- few tiles and a long K are split
// over K (see the kernel).
// kfirst (optional, with Pext): per group of 64 columns the first row of Pext that can be non-zero there (see the kernel); the array
// covers rows + 256 columns.
inline void chol_launch_update(const CholSwitches& sw, double* M, long lda, long rows, hipStream_t stream, int kcol0, int K, long base, long col_limit,
                               const double* Pext = nullptr, long ldp = 0, double* part = nullptr, const int* kfirst = nullptr, bool assign = false,
                               bool cap = false) {
  // trailing region: rows [base, rows), cols [base, col_limit)
  const long nrows = rows - base, nc = col_limit - base;
  if (nrows <= 0 || nc <= 0) return;
  // the big tile only when it still gives every CU a few workgroups
  const bool whole = (nc >= nrows - 1);
  const long big_tiles = ((nrows + 255) / 256) * ((nc + 127) / 128) / (whole ? 2 : 1);
  if (big_tiles >= 1024) {   // (square 128 x 128 tiles, two workgroups per CU, measured at n = 32,768: 238.7 vs 231.6 ms -- dropped)
    const long ntI = (nrows + 255) / 256, ntJ = (nc + 127) / 128;
    const long nblk = whole ? ntI * (ntI + 1) : ntI * ntJ;   // triangle: sum over ti of (2 ti + 2) tiles
    // round 6: the vendor-shaped 128 x 128 tile, two four-wave workgroups per CU (k_chol_update_v; ESL_UPD_V=0: the 256 x 128 tile).  Same bits.
    // (Four waves of 128 x 64 with the accumulators in AGPRs, k_chol_update_lds<256, 128, 2, 2>, were an experiment of the same round: retired)
    if (chol_update_v_applies(sw, lda, rows, base, col_limit, Pext != nullptr, ldp)) {
      const long vI = (nrows + kVT - 1) / kVT, vJ = (nc + kVT - 1) / kVT;
      const long vblk = whole ? chol_v_grid(vI) : vI * vJ;
      hipLaunchKernelGGL(k_chol_update_v, dim3((unsigned)vblk), dim3(256), (cap || sw.upd_v_cap) ? kCholLdsVCap : kCholLdsV, stream, M, lda, rows, col_limit, kcol0, K, base, (int)vJ, whole ? 0 : 1, Pext, ldp,
                         Pext ? kfirst : nullptr, assign ? 1 : 0);
      return;
    }
    hipLaunchKernelGGL((k_chol_update_lds<256, 128>), dim3((unsigned)nblk), dim3(512), kCholLdsBig, stream, M, lda, rows, col_limit, kcol0, K,
                       base, (int)ntJ, whole ? 0 : 1, Pext, ldp, (double*)nullptr, 0, Pext ? kfirst : nullptr);
  } else {
    const long ntI = (nrows + 127) / 128, ntJ = (nc + 63) / 64;
    const long nblk = whole ? ntI * (ntI + 1) : ntI * ntJ;
    int nsplit = 1, kper = K;
    if (part && Pext && base == 0 && nblk < 128 && K >= 16 * kKC) {
      nsplit = (int)std::min<long>(kCholMaxSplit, std::max<long>(1, 512 / nblk));
      kper = ((K + nsplit - 1) / nsplit + kKC - 1) / kKC * kKC;
      nsplit = (K + kper - 1) / kper;
    }
    if (nsplit > 1) {
      hipLaunchKernelGGL((k_chol_update_lds<128, 64>), dim3((unsigned)nblk, (unsigned)nsplit), dim3(512), kCholLdsSmall, stream, M, lda, rows, col_limit,
                         kcol0, K, base, (int)ntJ, whole ? 0 : 1, Pext, ldp, part, kper);
      hipLaunchKernelGGL(k_chol_splitk_reduce, dim3((unsigned)((rows * col_limit + 255) / 256)), dim3(256), 0, stream, M, lda, rows, col_limit, part, nsplit);
    } else {
      hipLaunchKernelGGL((k_chol_update_lds<128, 64>), dim3((unsigned)nblk), dim3(512), kCholLdsSmall, stream, M, lda, rows, col_limit, kcol0, K,
                         base, (int)ntJ, whole ? 0 : 1, Pext, ldp, (double*)nullptr, 0, Pext ? kfirst : nullptr);
    }
  }
}

// Per-context state of the host driver: the switches; the look-ahead stream and its events, which live on the CONTEXT's device and are used
// by one context only (two contexts sharing them could wait on each other's records); and hipFuncSetAttribute is per device.
struct CholRuntime {
  hipStream_t side = nullptr;
  std::vector<hipEvent_t> ev_panel, ev_trail;
  hipStream_t comm = nullptr;                               // the distributed factorisation's message stream
  hipEvent_t ev_begin = nullptr;                            // everything the caller's stream held when the factorisation began
  std::vector<hipEvent_t> ev_packed, ev_recv, ev_unpacked;  // per outer panel: message staged / received / copied out of its staging buffer
  bool attr_set = false;
  int* bs_flags = nullptr; int bs_flags_cap = 0;            // one "x_p published" word per 128-panel of k_chol_backsub
  // persistent factorisation: the task list / strip counts of the last (n, W) on the device, the sync words, begin / done events
  CholPlan plan;
  CholTask* d_tasks = nullptr; int* d_ns = nullptr; int* d_sync = nullptr;
  size_t d_tasks_cap = 0, d_ns_cap = 0, d_sync_cap = 0;
  CholSwitches sw;                                          // filled from the environment when chol_set_attributes first runs for this context
  int n_cu = 0;                                             // hipDeviceProp_t::multiProcessorCount of the context's device (grids of the one-launch forms)
  int fallbacks = 0;                                        // trials redone launch-per-step after a device-side hand-off timed out (esl_slam.hip)
  // optional event bracket around the FACTORISATION alone (not the back-substitution): mark(user, 1) before, mark(user, 0) after
  void (*prof_mark)(void* user, int begin) = nullptr;
  void* prof_user = nullptr;
  // camera-first elimination (esl_slam.hip): the separators' chain runs here beside the interior rows' pipeline, then the segments'
  // products beside the separators' forward recurrence and the rank-K update.  cf_ev_a: the separators' system is assembled (main
  // stream); cf_ev_s: their chain's blocks are written (side); cf_ev_x: the slabs are complete (main); cf_ev_p: the products are (side);
  // cf_ev_c: the segments' chains are factored (main); cf_ev_t: the sweep's per-slot matrices are written (side; esl_cf_sweep.hpp)
  hipStream_t cf_side = nullptr;
  hipEvent_t cf_ev_x = nullptr, cf_ev_p = nullptr, cf_ev_a = nullptr, cf_ev_s = nullptr, cf_ev_c = nullptr, cf_ev_t = nullptr;
  hipError_t cf_overlap_init() {
    if (cf_side && cf_ev_x && cf_ev_p && cf_ev_a && cf_ev_s && cf_ev_c && cf_ev_t) return hipSuccess;
    if (cf_side) return hipErrorNotReady;   // (an earlier attempt failed half way: the serial order)
    // (a plain second stream.  Two full-size grids on two streams do not run side by side -- the second kernel's workgroups are placed
    //  when the first one's are all dispatched -- and with the side stream confined to every 2nd / 4th / 8th CU of every XCD
    //  (hipExtStreamCreateWithCUMask) the products simply ran later AND slower: the bracket around T's build 29.3 -> 32.9 / 40.7 / 57.2 ms.
    //  What the second stream does give: the products fill the update's last, partly empty round of tiles: 30.0 -> 29.3 ms.)
    hipError_t e = hipStreamCreateWithFlags(&cf_side, hipStreamNonBlocking); if (e != hipSuccess) return e;
    for (hipEvent_t* ev : {&cf_ev_x, &cf_ev_p, &cf_ev_a, &cf_ev_s, &cf_ev_c, &cf_ev_t}) {
      e = hipEventCreateWithFlags(ev, hipEventDisableTiming); if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  void release() {
    if (cf_side) { (void)hipStreamSynchronize(cf_side); (void)hipStreamDestroy(cf_side); cf_side = nullptr; }
    for (hipEvent_t* ev : {&cf_ev_x, &cf_ev_p, &cf_ev_a, &cf_ev_s, &cf_ev_c, &cf_ev_t})
      if (*ev) { (void)hipEventDestroy(*ev); *ev = nullptr; }
    if (bs_flags) { (void)hipFree(bs_flags); bs_flags = nullptr; bs_flags_cap = 0; }
    if (d_tasks) { (void)hipFree(d_tasks); d_tasks = nullptr; d_tasks_cap = 0; }
    if (d_ns) { (void)hipFree(d_ns); d_ns = nullptr; d_ns_cap = 0; }
    if (d_sync) { (void)hipFree(d_sync); d_sync = nullptr; d_sync_cap = 0; }
    plan = CholPlan();
    for (std::vector<hipEvent_t>* v : {&ev_panel, &ev_trail, &ev_packed, &ev_recv, &ev_unpacked}) {
      for (hipEvent_t e : *v) (void)hipEventDestroy(e);
      v->clear();
    }
    if (side) { (void)hipStreamDestroy(side); side = nullptr; }
    if (comm) { (void)hipStreamDestroy(comm); comm = nullptr; }
    if (ev_begin) { (void)hipEventDestroy(ev_begin); ev_begin = nullptr; }
    attr_set = false;
  }
};

// dynamic-LDS limits of the big kernels, the switches and what they set on the device: once per context (= per device)
inline hipError_t chol_set_attributes(CholRuntime& rt) {
  if (rt.attr_set) return hipSuccess;
  rt.sw = chol_switches_from_env();
  hipError_t e = hipFuncSetAttribute((const void*)k_chol_potrf2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kP2Lds); if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_chol_update_lds<256, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCholLdsBig); if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_chol_update_v, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCholLdsVCap); if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_chol_backsub, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBsLds); if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_chol_persist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPwLds); if (e != hipSuccess) return e;
  const int on = rt.sw.timing ? 1 : 0;
  e = hipMemcpyToSymbol(HIP_SYMBOL(g_chol_stats_on), &on, sizeof(on)); if (e != hipSuccess) return e;
  if (rt.sw.timeout_ms > 0) {
    const long long ticks = 100000LL * rt.sw.timeout_ms;
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_chol_timeout_ticks), &ticks, sizeof(ticks)); if (e != hipSuccess) return e;
  }
  int dev = 0;
  hipDeviceProp_t prop;
  e = hipGetDevice(&dev); if (e != hipSuccess) return e;
  e = hipGetDeviceProperties(&prop, dev); if (e != hipSuccess) return e;
  rt.n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : kPwGrid;
  rt.attr_set = true;
  return hipSuccess;
}

// Far updates of a tile per visit (chol_plan_build).  Measured on MI355X (round 6, scripts/chol_bench.py).  With ONE grid of group
// boundaries for all tiles (1 / 2 / 4 / 8 outer panels per visit): n = 8,192 7.22 / 7.53 / 7.76 / 8.65 ms, 18,000 39.5 / 39.1 / 38.9 / 40.4 -- the
// time in task bodies falls as predicted (36.5 -> 34.1 ms) but the far work arrives in bursts and the waiting grows (2.7 -> 3.8 ms).
// With the boundaries STAGGERED by tile (1 / 2 / 3 / 4 / 6 per visit): n = 4,096 2.97 / 2.93 / 2.98, 8,192 7.35 / 7.12 / 7.18 / 7.70, 12,000
// 15.35 / 14.85 / 15.64 / 16.7, 18,000 39.38 / 37.94 / 37.67 / 38.0 / 39.2, 24,000 87.7 / 83.9 / 83.5 / 84.7 / 86.3.
// Default: 3 from n = 16,384, else 2; ESL_CHOL_MERGE overrides (1 = the round 4-5 list).
// The strips of a row tile away from the diagonal as ONE task (ESL_CHOL_STRIPS=1): measured and NOT the default -- n = 4,096 2.95 -> 3.57 ms,
// 8,192 7.00 -> 8.31, 12,000 15.0 -> 17.2, 18,000 37.7 -> 38.9, 24,000 83.4 -> 84.7: four workgroups finish a row tile's solve sooner than
// one, and every trailing update of that row tile waits for it.
inline int chol_merge_for(const CholSwitches& sw, int n) { return sw.merge > 0 ? sw.merge : (n >= 16384 ? 3 : 2); }
// the task list the switches select for an order-n system with outer panels of W inner panels (chol_factor_persistent, esl_debug_chol_plan)
inline void chol_plan_from_switches(const CholSwitches& sw, int n, int W, int filler, CholPlan& pl) {
  chol_plan_build(n, W, filler, pl, sw.fuse, chol_merge_for(sw, n), sw.strips, std::min(sw.special, W));
}
// the persistent kernel on the caller's stream (one launch; the sync words are cleared in front of it)
inline hipError_t chol_factor_persistent(double* M, long lda, int n, double* Linv_ws, int* info, hipStream_t st, CholRuntime& rt) {
  const CholSwitches& sw = rt.sw;
  const int W = sw.W > 0 ? sw.W : chol_outer_panels(n);
  const int merge = chol_merge_for(sw, n), spc = std::min(sw.special, W);
  if (rt.plan.n != n || rt.plan.W != W || rt.plan.fuse != (sw.fuse ? 1 : 0) || rt.plan.merge != merge || rt.plan.strip_merge != (sw.strips ? 1 : 0) || rt.plan.sp != spc) {
    { hipError_t e0 = hipStreamSynchronize(st); if (e0 != hipSuccess) return e0; }   // the old list / sync words may still be in use
    chol_plan_from_switches(sw, n, W, sw.filler, rt.plan);
    auto grow = [](void** p, size_t* cap, size_t need) -> hipError_t {
      if (*cap >= need) return hipSuccess;
      if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
      hipError_t e = hipMalloc(p, need); if (e == hipSuccess) *cap = need;
      return e;
    };
    hipError_t e = grow((void**)&rt.d_tasks, &rt.d_tasks_cap, std::max<size_t>(rt.plan.tasks.size(), 1) * sizeof(CholTask)); if (e != hipSuccess) return e;
    e = grow((void**)&rt.d_ns, &rt.d_ns_cap, std::max<size_t>(rt.plan.ns.size(), 1) * sizeof(int)); if (e != hipSuccess) return e;
    {
      const size_t need = chol_sync_words(rt.plan.np, rt.plan.nR) * sizeof(int);
      if (rt.d_sync_cap < need) {
        if (rt.d_sync) { (void)hipFree(rt.d_sync); rt.d_sync = nullptr; rt.d_sync_cap = 0; }
        e = hipMalloc((void**)&rt.d_sync, need); if (e != hipSuccess) return e;   // (polled words: read through chol_peek only)
        rt.d_sync_cap = need;
      }
    }
    // once per system size.  The stream is NON-BLOCKING (no implicit ordering with the null stream's copies): wait for whatever still
    // reads the old list, then ship the new one ON the stream, in front of the launch that reads it.  The source is
    // rt.plan (lives as long as the runtime); a pageable source is staged by the runtime before hipMemcpyAsync returns.
    // (The buffers above were re-allocated after the same wait would have been due: nothing of this context runs during a plan
    // change -- the previous factorisation's caller has read its info word, i.e. synchronised -- but the wait makes it a fact.)
    e = hipStreamSynchronize(st); if (e != hipSuccess) return e;
    if (!rt.plan.tasks.empty()) { e = hipMemcpyAsync(rt.d_tasks, rt.plan.tasks.data(), rt.plan.tasks.size() * sizeof(CholTask), hipMemcpyHostToDevice, st); if (e != hipSuccess) return e; }
    e = hipMemcpyAsync(rt.d_ns, rt.plan.ns.data(), rt.plan.ns.size() * sizeof(int), hipMemcpyHostToDevice, st); if (e != hipSuccess) return e;
  }
  const CholPlan& pl = rt.plan;
  hipError_t e = hipMemsetAsync(rt.d_sync, 0, chol_sync_words(pl.np, pl.nR) * sizeof(int), st); if (e != hipSuccess) return e;
  // one workgroup per CU of THIS device (the kernel is correct for any grid >= 2: the first arrival is the chain, the others pull tasks)
  const int grid = std::max(2, std::min(rt.n_cu > 0 ? rt.n_cu : kPwGrid, kPwGrid));
  hipLaunchKernelGGL(k_chol_persist, dim3((unsigned)grid), dim3(kPwThreads), kPwLds, st, M, lda, n, pl.np, pl.W, pl.nR, Linv_ws, (const CholTask*)rt.d_tasks,
                     (int)pl.tasks.size(), (const int*)rt.d_ns, rt.d_sync, info, pl.fuse, pl.sp);
  return hipGetLastError();
}

// ---- host driver: the forms of the factorisation, each on its own, and the dispatcher -------------------------------------------------
// Outer panels of W inner panels (W x 128 columns): the inner panels are factored one after the other on the caller's
// stream, each followed by a rank-128 update of the rest of the outer panel; the trailing matrix then gets ONE rank-(W x 128)
// update (W = 2 halves, W = 4 quarters the read-modify-write traffic on C and the per-tile prologue / epilogue per flop).
// Geometry of outer panel o: inner panels [p0, p1), columns [c_begin, c_end); as a message, h rows from the diagonal down (the
// right-hand side's row among them) x w columns, then the n_inv doubles of its diagonal blocks' inverses.
struct CholOuter { int p0, p1, c_begin, c_end; long h, w; size_t n_inv; };
inline CholOuter chol_outer_geo(int n, int o) {
  const int W = chol_outer_panels(n), np = (n + kNB - 1) / kNB;
  CholOuter g;
  g.p0 = o * W; g.p1 = (g.p0 + W < np) ? g.p0 + W : np;
  g.c_begin = g.p0 * kNB; g.c_end = (g.p1 * kNB < n) ? g.p1 * kNB : n;
  g.h = (long)n + 1 - g.c_begin; g.w = g.c_end - g.c_begin; g.n_inv = (size_t)(g.p1 - g.p0) * kNB * kNB;
  return g;
}
inline int chol_n_outer(int n) { const int W = chol_outer_panels(n); return ((n + kNB - 1) / kNB + W - 1) / W; }
// factor outer panel g on `st`: per inner panel the diagonal block, the panel solve, and the rank-nb update that brings the rest of the
// outer panel's columns up to date
inline void chol_factor_outer(const CholSwitches& sw, double* M, long lda, int n, double* Linv_ws, int* info, hipStream_t st, const CholOuter& g) {
  const long rows = (long)n + 1;
  for (int p = g.p0; p < g.p1; ++p) {
    const int k0 = p * kNB, nb = (n - k0 < kNB) ? (n - k0) : kNB;
    double* Linv = Linv_ws + (size_t)p * kNB * kNB;
    hipLaunchKernelGGL(k_chol_potrf2, dim3(1), dim3(kP2Threads), kP2Lds, st, M, lda, k0, nb, Linv, info);
    const long below = rows - (k0 + nb);
    if (below > 0) hipLaunchKernelGGL(k_chol_panel, dim3((unsigned)((below + 63) / 64)), dim3(512), 0, st, M, lda, rows, k0, nb, Linv);
    if (p + 1 < g.p1) chol_launch_update(sw, M, lda, rows, st, k0, nb, (long)k0 + nb, (long)g.c_end);
  }
}
// a factored outer panel as ONE message in buf (the panel from its diagonal down, then the diagonal blocks' inverses), and back out of it
inline hipError_t chol_stage_panel(double* M, long lda, int n, double* Linv_ws, hipStream_t st, const CholOuter& g, double* buf) {
  hipLaunchKernelGGL(k_chol_pack, dim3((unsigned)((g.h + 255) / 256), (unsigned)g.w), dim3(256), 0, st, M, lda, (long)n + 1, (long)g.c_begin, (long)g.c_begin, buf, 0);
  return hipMemcpyAsync(buf + (size_t)g.h * g.w, Linv_ws + (size_t)g.p0 * kNB * kNB, g.n_inv * sizeof(double), hipMemcpyDeviceToDevice, st);
}
inline hipError_t chol_unpack_panel(double* M, long lda, int n, double* Linv_ws, hipStream_t st, const CholOuter& g, double* buf) {
  hipLaunchKernelGGL(k_chol_pack, dim3((unsigned)((g.h + 255) / 256), (unsigned)g.w), dim3(256), 0, st, M, lda, (long)n + 1, (long)g.c_begin, (long)g.c_begin, buf, 1);
  return hipMemcpyAsync(Linv_ws + (size_t)g.p0 * kNB * kNB, buf + (size_t)g.h * g.w, g.n_inv * sizeof(double), hipMemcpyDeviceToDevice, st);
}
inline hipError_t chol_grow_events(std::vector<hipEvent_t>& v, int count) {
  while ((int)v.size() < count) {
    hipEvent_t ev;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming); if (e != hipSuccess) return e;
    v.push_back(ev);
  }
  return hipSuccess;
}

// small systems on one GPU: one workgroup, one launch, substitutions included (k_chol_small)
inline hipError_t chol_solve_small(const double* M, long lda, int n, double* x, int* info, hipStream_t st) {
  hipLaunchKernelGGL(k_chol_small, dim3(1), dim3(kCsThreads), 0, st, M, lda, n, x, info);
  return hipGetLastError();
}

// ---- distributed, messages overlapped with the trailing updates --------------------------------------------------------------
// Streams: st (the caller's: all arithmetic), rt.comm (the broadcasts, in panel order -- the same order on every rank).
// Buffers: panel o travels in pack (o even) / pack2 (o odd).  Events per panel o: ev_packed (owner: factored + staged, on st),
// ev_recv (message complete, on comm), ev_unpacked (non-owners: copied out into M / Linv_ws, on st).  Ordering that keeps the two
// buffers safe: the broadcast of panel o waits for ev_packed[o] on the owner and for ev_unpacked[o - 2] on the others (the last
// reader of that buffer); the owner stages panel o on st after st has waited for ev_recv[o - 1], and comm runs in order, so the
// broadcast of panel o - 2 (the last sender from that buffer) is over by then.
// Every panel still receives the updates of panels 0, 1, 2, .. in that order: same bits as chol_factor_dist.
inline hipError_t chol_factor_dist_overlap(double* M, long lda, int n, double* Linv_ws, int* info, hipStream_t st, CholRuntime& rt, const CholDist& dist) {
  const long rows = (long)n + 1;
  const int n_outer = chol_n_outer(n), R = dist.n_ranks, me = dist.rank;
  if (!rt.comm) { hipError_t e = hipStreamCreateWithFlags(&rt.comm, hipStreamNonBlocking); if (e != hipSuccess) return e; }
  if (!rt.ev_begin) { hipError_t e = hipEventCreateWithFlags(&rt.ev_begin, hipEventDisableTiming); if (e != hipSuccess) return e; }
  {   // the message stream starts behind everything the caller's stream already holds (its earlier collectives on this communicator
      // among it: two collectives of one communicator must not run side by side)
    hipError_t e = hipEventRecord(rt.ev_begin, st); if (e != hipSuccess) return e;
    e = hipStreamWaitEvent(rt.comm, rt.ev_begin, 0); if (e != hipSuccess) return e;
  }
  for (std::vector<hipEvent_t>* v : {&rt.ev_packed, &rt.ev_recv, &rt.ev_unpacked}) { hipError_t e = chol_grow_events(*v, n_outer); if (e != hipSuccess) return e; }
  auto buf_of = [&](int o) { return (o & 1) ? dist.pack2 : dist.pack; };
  auto factor_and_stage = [&](int o) -> hipError_t {   // this rank owns panel o; everything on st
    const CholOuter g = chol_outer_geo(n, o);
    chol_factor_outer(rt.sw, M, lda, n, Linv_ws, info, st, g);
    hipError_t e = chol_stage_panel(M, lda, n, Linv_ws, st, g, buf_of(o)); if (e != hipSuccess) return e;
    e = hipGetLastError(); if (e != hipSuccess) return e;
    return hipEventRecord(rt.ev_packed[o], st);
  };
  auto update_with = [&](int o, int o2) {   // panel o2 -= (its rows of panel o) (panel o's rows of panel o2's columns)^T
    const CholOuter g = chol_outer_geo(n, o), q = chol_outer_geo(n, o2);
    chol_launch_update(rt.sw, M, lda, rows, st, g.c_begin, g.c_end - g.c_begin, (long)q.c_begin, (long)q.c_end);
  };
  if (0 % R == me) { hipError_t e = factor_and_stage(0); if (e != hipSuccess) return e; }
  for (int o = 0; o < n_outer; ++o) {
    const int owner = o % R;
    const CholOuter g = chol_outer_geo(n, o);
    hipError_t e;
    if (owner == me) e = hipStreamWaitEvent(rt.comm, rt.ev_packed[o], 0);
    else e = (o >= 2) ? hipStreamWaitEvent(rt.comm, rt.ev_unpacked[o - 2], 0) : hipSuccess;
    if (e != hipSuccess) return e;
    if (dist.bcast_on(dist.user, buf_of(o), (size_t)g.h * g.w + g.n_inv, owner, rt.comm)) return hipErrorUnknown;
    e = hipEventRecord(rt.ev_recv[o], rt.comm); if (e != hipSuccess) return e;
    e = hipStreamWaitEvent(st, rt.ev_recv[o], 0); if (e != hipSuccess) return e;
    if (owner != me) { e = chol_unpack_panel(M, lda, n, Linv_ws, st, g, buf_of(o)); if (e != hipSuccess) return e; }
    e = hipEventRecord(rt.ev_unpacked[o], st); if (e != hipSuccess) return e;
    // look-ahead: the next panel, if it is this rank's, before anything else
    const bool next_mine = o + 1 < n_outer && (o + 1) % R == me;
    if (next_mine) {
      update_with(o, o + 1);
      e = factor_and_stage(o + 1); if (e != hipSuccess) return e;
    }
    for (int o2 = o + 1 + (next_mine ? 1 : 0); o2 < n_outer; ++o2)
      if (o2 % R == me) update_with(o, o2);
  }
  return hipSuccess;
}

// ---- distributed, the messages on the caller's stream one after the other (ESL_CHOL_DIST_OVERLAP=0, or no second buffer / stream-taking broadcast)
inline hipError_t chol_factor_dist(double* M, long lda, int n, double* Linv_ws, int* info, hipStream_t st, CholRuntime& rt, const CholDist& dist) {
  const long rows = (long)n + 1;
  const int n_outer = chol_n_outer(n);
  for (int o = 0; o < n_outer; ++o) {
    const int owner = o % dist.n_ranks;
    const CholOuter g = chol_outer_geo(n, o);
    if (owner == dist.rank) {
      chol_factor_outer(rt.sw, M, lda, n, Linv_ws, info, st, g);
      hipError_t e = hipGetLastError(); if (e != hipSuccess) return e;
    }
    if (dist.pack) {   // one message: the panel from its diagonal down, then the diagonal blocks' inverses
      if (owner == dist.rank) { hipError_t e = chol_stage_panel(M, lda, n, Linv_ws, st, g, dist.pack); if (e != hipSuccess) return e; }
      if (dist.bcast(dist.user, dist.pack, (size_t)g.h * g.w + g.n_inv, owner)) return hipErrorUnknown;
      if (owner != dist.rank) { hipError_t e = chol_unpack_panel(M, lda, n, Linv_ws, st, g, dist.pack); if (e != hipSuccess) return e; }
    } else {
      // the factored columns (whole columns: the rows above the diagonal travel along, unused) and the diagonal blocks' inverses
      if (dist.bcast(dist.user, M + (size_t)g.c_begin * lda, (size_t)lda * (size_t)(g.c_end - g.c_begin), owner)) return hipErrorUnknown;
      if (dist.bcast(dist.user, Linv_ws + (size_t)g.p0 * kNB * kNB, g.n_inv, owner)) return hipErrorUnknown;
    }
    // this rank's later outer panels
    for (int o2 = o + 1; o2 < n_outer; ++o2) {
      if (o2 % dist.n_ranks != dist.rank) continue;
      const CholOuter q = chol_outer_geo(n, o2);
      chol_launch_update(rt.sw, M, lda, rows, st, g.c_begin, g.c_end - g.c_begin, (long)q.c_begin, (long)q.c_end);
    }
  }
  return hipSuccess;
}

// ---- launch per step with look-ahead ------------------------------------------------------------------------------------------
// The trailing update of an outer panel is split -- the columns of the NEXT outer panel are updated on the caller's stream, the rest
// on a second stream, so the next outer panel's potrf / panel solves (single-workgroup and short kernels that leave the chip
// empty) run underneath the big update instead of in front of it.
inline hipError_t chol_factor_lookahead(double* M, long lda, int n, double* Linv_ws, int* info, hipStream_t st, CholRuntime& rt) {
  const long rows = (long)n + 1;
  const int n_outer = chol_n_outer(n);
  // below ~8k unknowns the chain of single-workgroup potrf launches is the critical path whatever runs beside it (measured:
  // n = 2994 4.55 ms without, 4.75 ms with look-ahead), from 16k on it buys 12-15 %
  const bool lookahead = n >= 8192;
  bool trail_pending = false;   // rt.ev_trail[o - 1] has been recorded and not yet waited for
  for (int o = 0; o < n_outer; ++o) {
    const CholOuter g = chol_outer_geo(n, o);
    chol_factor_outer(rt.sw, M, lda, n, Linv_ws, info, st, g);
    if (g.c_end >= n) break;
    const int K = g.c_end - g.c_begin;
    const int next_end = chol_outer_geo(n, o + 1).c_end;                   // end of the next outer panel's columns
    if (!lookahead || next_end >= n) {
      if (trail_pending) { hipError_t e = hipStreamWaitEvent(st, rt.ev_trail[o - 1], 0); if (e != hipSuccess) return e; trail_pending = false; }
      chol_launch_update(rt.sw, M, lda, rows, st, g.c_begin, K, (long)g.c_end, (long)n);
      continue;
    }
    hipError_t e = hipEventRecord(rt.ev_panel[o], st); if (e != hipSuccess) return e;
    // the next outer panel's columns: written by the previous side-stream update as well -> wait for it first
    if (trail_pending) { e = hipStreamWaitEvent(st, rt.ev_trail[o - 1], 0); if (e != hipSuccess) return e; trail_pending = false; }
    chol_launch_update(rt.sw, M, lda, rows, st, g.c_begin, K, (long)g.c_end, (long)next_end);
    // everything to the right of them, underneath the next outer panel's factorisation
    e = hipStreamWaitEvent(rt.side, rt.ev_panel[o], 0); if (e != hipSuccess) return e;
    chol_launch_update(rt.sw, M, lda, rows, rt.side, g.c_begin, K, (long)next_end, (long)n);
    e = hipEventRecord(rt.ev_trail[o], rt.side); if (e != hipSuccess) return e;
    trail_pending = true;
  }
  if (trail_pending) { hipError_t e = hipStreamWaitEvent(st, rt.ev_trail[n_outer - 2], 0); if (e != hipSuccess) return e; }
  return hipSuccess;
}

// ---- backward substitution L^T x = y: one launch (k_chol_backsub), or two launches per panel (ESL_CHOL_BACKSUB_LAUNCHES=1: the A/B
// form, and the fallback where the one-launch form cannot read the factor as 16-byte pairs: odd leading dimension, unaligned base)
inline hipError_t chol_back_substitute(const double* M, long lda, int n, const double* Linv_ws, double* z_ws, double* x, int* info, hipStream_t st, CholRuntime& rt) {
  const int np = (n + kNB - 1) / kNB;
  if (!rt.sw.backsub_launches && (lda & 1) == 0 && ((uintptr_t)M & 15) == 0 && ((uintptr_t)Linv_ws & 15) == 0) {
    if (rt.bs_flags_cap < np + 1) {   // np panel flags + the arrival-ticket word
      if (rt.bs_flags) { (void)hipFree(rt.bs_flags); rt.bs_flags = nullptr; rt.bs_flags_cap = 0; }
      const int cap = std::max(np + 1, 512);
      hipError_t e = hipMalloc((void**)&rt.bs_flags, (size_t)cap * sizeof(int)); if (e != hipSuccess) return e;   // (polled words: read through chol_peek only)
      rt.bs_flags_cap = cap;
    }
    hipError_t e = hipMemsetAsync(rt.bs_flags, 0, (size_t)(np + 1) * sizeof(int), st); if (e != hipSuccess) return e;
    const int bs_grid = std::min(np, std::min(rt.n_cu > 0 ? rt.n_cu : kBsMaxGrid, kBsMaxGrid));
    hipLaunchKernelGGL(k_chol_backsub, dim3((unsigned)bs_grid), dim3(kBsThreads), kBsLds, st, M, lda, n, np, Linv_ws, x, rt.bs_flags, info);
    return hipGetLastError();
  }
  for (int p = np - 1; p >= 0; --p) {
    const int k0 = p * kNB, nb = (n - k0 < kNB) ? (n - k0) : kNB;
    hipLaunchKernelGGL(k_chol_backdot, dim3(nb), dim3(256), 0, st, M, lda, n, k0, nb, (const double*)x, z_ws);
    hipLaunchKernelGGL(k_chol_backsolve, dim3((nb + 3) / 4), dim3(256), 0, st, Linv_ws + (size_t)p * kNB * kNB, k0, nb, (const double*)z_ws, x);
  }
  return hipGetLastError();
}

// the optional event bracket around the FACTORISATION alone: closes on EVERY way out of it, error returns included (an
// early return used to leave the scope open, and later brackets were skipped or mis-paired)
struct CholProfBracket {
  CholRuntime& r; bool open;
  explicit CholProfBracket(CholRuntime& rr) : r(rr), open(rr.prof_mark != nullptr) { if (open) r.prof_mark(r.prof_user, 1); }
  void close() { if (open) { r.prof_mark(r.prof_user, 0); open = false; } }
  ~CholProfBracket() { close(); }
};

// Host driver.  M: (n+1) x n col-major (lda), Linv_ws: ceil(n/NB) * NB*NB doubles, z_ws: NB doubles,
// x: n doubles (output), info: device int (bit 0 set on a non-positive pivot).  The current device must be the one `rt` and
// `st` belong to.
inline hipError_t chol_factor_solve(double* M, long lda, int n, double* Linv_ws, double* z_ws, double* x, int* info,
                                    hipStream_t st, CholRuntime& rt, const CholDist* dist = nullptr) {
  { hipError_t e = chol_set_attributes(rt); if (e != hipSuccess) return e; }
  const CholSwitches& sw = rt.sw;
  CholProfBracket bracket(rt);
  const bool multi = dist && dist->n_ranks > 1;
  // small systems on one GPU: k_chol_small substitutes by itself.  (ESL_CHOL_SMALL=0 keeps the blocked path: A/B and the tests that
  // compare the two; ESL_CHOL_PERSISTENT=1 asks for that kernel at every size: the tests of its chain)
  if (!multi && chol_small_fits(n) && sw.small && sw.persistent != 1) return chol_solve_small(M, lda, n, x, info, st);
  // the look-ahead stream and its events, per context
  if (!rt.side) { hipError_t e = hipStreamCreateWithFlags(&rt.side, hipStreamNonBlocking); if (e != hipSuccess) return e; }
  for (std::vector<hipEvent_t>* v : {&rt.ev_panel, &rt.ev_trail}) { hipError_t e = chol_grow_events(*v, chol_n_outer(n)); if (e != hipSuccess) return e; }
  hipError_t e;
  if (multi && dist->pack && dist->pack2 && dist->bcast_on) e = chol_factor_dist_overlap(M, lda, n, Linv_ws, info, st, rt, *dist);
  else if (multi) e = chol_factor_dist(M, lda, n, Linv_ws, info, st, rt, *dist);
  // one launch or launch per step, by size, measured on MI355X (profiles/r4_cholesky_microbench.txt), one launch vs launch per step:
  // n = 2,994 2.43 vs 2.24 ms, 4,096 3.23 vs 3.24, 6,000 4.88 vs 5.75, 8,192 7.94 vs 8.95, 12,000 15.9 vs 17.9, 18,000 40.3 vs 43.9,
  // 24,000 88.0 vs 91.8, 32,768 214.4 vs 214.5 (a draw: the launch path is kept there, it is the form that has run the
  // order-59,994 reduced camera system since round 1)
  else if (sw.persistent == 1 || (sw.persistent == 2 && n >= 4096 && n < 30000)) e = chol_factor_persistent(M, lda, n, Linv_ws, info, st, rt);
  else e = chol_factor_lookahead(M, lda, n, Linv_ws, info, st, rt);
  if (e != hipSuccess) return e;
  bracket.close();
  return chol_back_substitute(M, lda, n, Linv_ws, z_ws, x, info, st, rt);
}

// ---- ESL_CHOL_TIMING: what the kernels' diagnostics recorded during their last launches, to stderr (esl_selftest_cholesky) -----------
inline void chol_print_timing(int n) {
  std::vector<long long> ps((size_t)kPwGrid * 5, 0);
  if (hipMemcpyFromSymbol(ps.data(), HIP_SYMBOL(g_chol_stats), ps.size() * sizeof(long long)) == hipSuccess && ps[2] > 0) {
    // persistent kernel, last launch: workgroup 0 = the chain of diagonal blocks, the others pull tasks off the list
    long long t_first = ps[3], t_last = ps[4];
    double w_wait = 0, w_body = 0, w_tasks = 0, w_span = 0, w_wait_max = 0, w_end_min = 1e300, w_end_max = 0; int nw = 0;
    for (int b = 1; b < kPwGrid; ++b) {
      const long long* q = &ps[(size_t)b * 5];
      if (q[4] == 0) continue;
      t_first = std::min(t_first, q[3]); t_last = std::max(t_last, q[4]);
    }
    for (int b = 1; b < kPwGrid; ++b) {
      const long long* q = &ps[(size_t)b * 5];
      if (q[4] == 0) continue;
      ++nw; w_wait += (double)q[0]; w_body += (double)q[1]; w_tasks += (double)q[2]; w_span += (double)(q[4] - q[3]);
      w_wait_max = std::max(w_wait_max, (double)q[0]);
      w_end_min = std::min(w_end_min, (double)(q[4] - t_first)); w_end_max = std::max(w_end_max, (double)(q[4] - t_first));
    }
    fprintf(stderr, "[k_chol_persist, last launch] span %.2f ms | chain: %lld blocks, waiting %.2f ms, factoring %.2f ms | %d workers: mean waiting %.2f ms (max %.2f), "
                    "in task bodies %.2f ms, %.0f tasks each, alive %.2f ms, first / last exit at %.2f / %.2f ms\n",
            (double)(t_last - t_first) * 1e-5, ps[2], (double)ps[0] * 1e-5, (double)ps[1] * 1e-5, nw, nw ? w_wait / nw * 1e-5 : 0.0, w_wait_max * 1e-5,
            nw ? w_body / nw * 1e-5 : 0.0, nw ? w_tasks / nw : 0.0, nw ? w_span / nw * 1e-5 : 0.0, w_end_min * 1e-5, w_end_max * 1e-5);
  }
  {
    std::vector<long long> cl(2048, 0);
    const int npl = std::min(1024, (n + kNB - 1) / kNB);
    if (ps[2] > 0 && hipMemcpyFromSymbol(cl.data(), HIP_SYMBOL(g_chol_chain_log), cl.size() * sizeof(long long)) == hipSuccess && npl > 8) {
      // the chain's timeline, averaged over eighths of the panels: factor time and the gap between one factor published and the next tile final
      long long ft[4] = {0, 0, 0, 0};
      if (hipMemcpyFromSymbol(ft, HIP_SYMBOL(g_chol_fuse_ticks), sizeof(ft)) == hipSuccess && (ft[1] | ft[2]))
        fprintf(stderr, "[k_chol_persist chain, fused stage, us per panel] waits %.1f  rows under the block %.1f  next block's update %.1f  drain %.1f\n",
                (double)ft[0] * 0.01 / npl, (double)ft[1] * 0.01 / npl, (double)ft[2] * 0.01 / npl, (double)ft[3] * 0.01 / npl);
      fprintf(stderr, "[k_chol_persist chain, us per panel by eighth of the matrix: potrf / gap to the next block]");
      for (int e = 0; e < 8; ++e) {
        const int k0 = e * npl / 8, k1 = std::min(npl - 1, (e + 1) * npl / 8);
        double f = 0, g = 0; int c = 0;
        for (int k = k0; k < k1; ++k) { f += (double)(cl[2 * k + 1] - cl[2 * k]); g += (double)(cl[2 * k + 2] - cl[2 * k + 1]); ++c; }
        if (c) fprintf(stderr, " %.0f/%.0f", f / c * 0.01, g / c * 0.01);
      }
      fprintf(stderr, "\n");
      {   // the same over the last three eighths (where the chain sets the pace), by the panel's position in its outer panel
        const int Wp = chol_outer_panels(n);
        std::vector<double> f(Wp, 0), g(Wp, 0); std::vector<int> cn(Wp, 0);
        for (int k = 5 * npl / 8; k < npl - 1; ++k) { f[k % Wp] += (double)(cl[2 * k + 1] - cl[2 * k]); g[k % Wp] += (double)(cl[2 * k + 2] - cl[2 * k + 1]); ++cn[k % Wp]; }
        fprintf(stderr, "[k_chol_persist chain, last 3/8 of the panels, us by k mod W: potrf / gap]");
        for (int q = 0; q < Wp; ++q) if (cn[q]) fprintf(stderr, " %.0f/%.0f", f[q] / cn[q] * 0.01, g[q] / cn[q] * 0.01);
        fprintf(stderr, "\n");
      }
    }
  }
  {
    long long uc[4] = {0, 0, 0, 0};
    if (hipMemcpyFromSymbol(uc, HIP_SYMBOL(g_upd_clk), sizeof(uc)) == hipSuccess && uc[1] > 0)
      fprintf(stderr, "[k_chol_update_lds, one %lld-row tile of the last launch, K = %lld] %.1f us at a shader clock of %.0f MHz -> MFMA peak at that clock %.1f TFLOP/s\n",
              uc[3], uc[2], (double)uc[1] * 0.01, (double)uc[0] / (double)uc[1] * 100.0, 78.6 * ((double)uc[0] / (double)uc[1] * 100.0) / 2400.0);
  }
  long long clk[16];
  if (hipMemcpyFromSymbol(clk, HIP_SYMBOL(g_potrf_clk), sizeof(clk)) == hipSuccess) {
    static const char* names[9] = {"load", "rank-4 steps", "-", "-", "-", "store L", "-", "inverse", "store Linv"};
    fprintf(stderr, "[k_chol_potrf2, last launch, us into the rank-4 loop at step 1 / 8 / 16 / 24: %.1f %.1f %.1f %.1f]\n", (double)(clk[10] - clk[1]) * 0.01,
            (double)(clk[11] - clk[1]) * 0.01, (double)(clk[12] - clk[1]) * 0.01, (double)(clk[13] - clk[1]) * 0.01);
    fprintf(stderr, "[k_chol_potrf2, last launch, triangular inverse: levels 4 + 8 %.1f us, level 16 %.1f us, levels 32 + 64 %.1f us]\n", (double)(clk[14] - clk[7]) * 0.01,
            (double)(clk[15] - clk[14]) * 0.01, (double)(clk[8] - clk[15]) * 0.01);
    fprintf(stderr, "[k_chol_potrf2, last launch, us]");
    for (int k = 0; k < 9; ++k) fprintf(stderr, " %s=%.1f", names[k], (double)(clk[k + 1] - clk[k]) * 0.01);
    fprintf(stderr, "\n");
  }
}

}  // namespace esl
