// esl_chol_persist.hpp — the persistent (one-launch) dense factorisation: the bounded wait on a dependency word, the fused steps of the
// chain of diagonal blocks, and k_chol_persist itself.  Task list: esl_chol_plan.hpp; host driver: chol_factor_persistent (esl_chol.hpp).
#pragma once
#include "esl_chol_kernels.hpp"
#include "esl_chol_plan.hpp"

namespace esl {

// ---- persistent factorisation (round 4) -----------------------------------------------------------------------------------------
// The launch-per-step form (esl_chol_kernels.hpp) leaves the chain of diagonal blocks exposed wherever the trailing matrix is too small to hide it
// (the last ~8,000 rows of an order-18,000 system, ~8 of its 44 ms) and its small kernels queue behind 110 us update tiles for a
// free CU.  Here ONE kernel, k_chol_persist, runs the whole factorisation: 256 workgroups of 512 threads, every one the only
// tenant of its CU (157 KB of LDS).  Workgroup 0 is the CHAIN: it walks the diagonal blocks (the potrf2 body).  The other 255 pull
// TASKS from a static list with one atomic counter.  Tasks, on the absolute tile grid (row tiles of 256, column tiles = the
// 128-wide panels):
//   S(k, i)     strip i (64 rows) of the panel solve of panel k                            (k_chol_panel's body)
//   u(k, R, J)  tile (R, J) -= X(R, k) X(J, k)^T, rank 128, J in the rest of k's outer panel (k_chol_update_lds's body); the
//               DIAGONAL tile of a panel takes these in quarters (task type 3, below)
//   U(o, R, J)  tile (R, J) -= X(R, o) X(J, o)^T, rank W x 128, J beyond outer panel o
// Dependencies are words in device memory (zeroed by a memset in front of the launch): pdone[k] (chain: L_kk, Linv_k published),
// sdone[k][R] (strips of row tile R solved for panel k; complete at ns[k][R]), ver[R][J] (updates applied to tile (R, J): every
// update carries its sequence number, waits for ver == seq and leaves ver = seq + 1 -- read-modify-write order and "tile final"
// in one word).  The list is in an order in which every task's prerequisites come earlier (or are the chain's), so a workgroup
// that spins on a word waits for work another RESIDENT workgroup already holds: no deadlock whatever the dispatch order; the
// next outer panel's chain-dependent tasks sit between batches of the previous outer panel's far updates (look-ahead without
// streams or events).  tests/test_chol_plan.py replays the list on the CPU.  Hand-offs follow the guide's recipe R1: payload
// stored write-through (sc1), every storing wave drains, one lane publishes the word; the consumer polls from one lane, ONE
// agent-scope acquire, plain loads.  Every spin is bounded (bit 1 of info + an abort word that stops all other spins).
// What the first versions taught (all measured on MI355X, round 4):
//   * TWO kernels (chain / workers) on two streams are co-resident only until something else touches the queues: a stream created
//     or destroyed anywhere in the process while they run gets them TIME-SLICED against each other, and a spinning consumer whose
//     producer is switched out turns a 40 ms factorisation into seconds.  One kernel cannot be split that way.
//   * a polled word must be read with a WRITING atomic (chol_peek: an atomic add of zero).  Agent-scope loads, fetch_or(0) (the
//     compiler folds it into a load) and failing compare-and-swaps are all served from the polling XCD's L2, which another XCD's
//     write-through store does not update: once every workgroup of an XCD waits, nothing evicts the line and the stale value is
//     read forever.  Pollers back to back saturate the atomic units (255 of them slowed the whole kernel 100x): workers sleep
//     ~2.7 us between polls, the chain ~0.1 us; a plain agent-scope load goes first (the words only grow: stale can under-report).
//   * where the time goes at n = 18,000 (ESL_CHOL_TIMING=1 prints it): workers spend 35.5 of 40 ms inside task bodies (the
//     rank-512 tiles run at ~73 % of a CU's MFMA peak) and 3.5 ms waiting; the chain is idle 31 ms -- and sets the pace over the
//     last three eighths of the panels, where a step costs potrf 62 us + 40 us (strips under the diagonal block -> the quarters of
//     the next diagonal tile -> the next block) against 3 - 70 us of trailing work.  Two schedule changes got it there from
//     62 + 68 us: the diagonal tile's rank-128 updates in four quarters (42 us for one workgroup), and the first diagonal tile of
//     the NEXT outer panel fed rank-128 updates panel by panel instead of waiting for its rank-512 tile (chol_tile_special).
//   * the chain then stopped waiting for other workgroups between two blocks: it solves the 128 rows under its block against the
//     inverse that is still in its LDS and applies the rank-128 update to the next diagonal block itself (chol_chain_solve_rows /
//     chol_chain_update_next; strips 0, 1 and the diagonal half of the quarters leave the task list; ESL_CHOL_FUSE=0 is the
//     form before).  Its own 25 us (14 + 10 + drain) replace 40 us of hand-offs: the step is 66 + 36 us, n = 18,000 40.5 -> 40.0 ms.
//     The chain's own arithmetic is now what the last eighths of the panels cost; the next lever is the 66 us of potrf2.
// sync words: [0] task counter, [1] abort, [2] arrival tickets (0 = the chain), [4 ..) pdone[np], sdone[np][nR], ver[nR][np], quarters done [nR][np]
inline size_t chol_sync_words(int np, int nR) { return 4 + (size_t)np + 3 * (size_t)np * nR; }
__device__ long long g_chol_timeout_ticks = 300000000LL;   // 3 s at 100 MHz (ESL_CHOL_TIMEOUT_MS overrides it: debugging)
// Spin until *word >= want (ONE lane; bounded).  Every poll is a chol_peek -- a device-scope atomic -- so the pollers are RATE
// LIMITED: 255 workgroups polling back to back saturate the atomic units (~90 atomics per us on one word) and every other atomic
// of the launch -- the chain's own polls, the task counter, the publishes -- queues behind them: measured, the first 30 panels of an
// order-8,192 system then take 300 ms instead of 4.  SLEEP = argument of s_sleep (64 cycles each): workers wait ~2.7 us between
// polls (at most ~95 polls per us from all of them together), the chain -- one poller -- ~0.1 us.
template <int SLEEP>
__device__ __forceinline__ bool chol_wait_ge(int* word, int want, int* abortw, int* info) {
  // fast path: a plain agent-scope load.  The words only ever grow, so a stale copy can under-report but never over-report; most
  // waits of tasks deep in the list were satisfied long ago and this XCD has either never fetched the line or fetched it late enough
  if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) return true;
  if (chol_peek(word) >= want) return true;
  const long long t0 = (long long)wall_clock64();
  for (unsigned spins = 1;; ++spins) {
    __builtin_amdgcn_s_sleep(SLEEP);
    if (chol_peek(word) >= want) return true;
    if ((spins & 15u) == 0) {
      // (abort: a plain agent-scope load is enough -- a poller that keeps seeing a stale 0 runs into its own timeout)
      if (__hip_atomic_load(abortw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
      if ((long long)wall_clock64() - t0 > g_chol_timeout_ticks) {
        atomicOr(info, 2);
        __hip_atomic_store(abortw, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
      }
    }
  }
}

// ---- the chain's own step to the next diagonal block (round 4, "fused chain") -------------------------------------------------
// After chol_potrf2_body the LDS array L holds Linv_k.  The next diagonal block waits for two things that other workgroups used to
// deliver: the solve of the 128 rows under block k (strips 0, 1 of panel k) and the rank-128 update of block k + 1 with them --
// 40 us of task bodies, drains and polls per panel against ~8 us of arithmetic.  Here the chain does both itself:
//   stage B   X = A[r0 .. r0 + 128, panel k] Linv_k^T   (rows < `rows`: the right-hand side's row rides along), Linv from LDS, A from
//             global memory; X goes to global memory (it IS L's rows) and, once every wave has finished with Linv, into the LDS array
//   stage C   A[r0 + i, c1 + j] -= sum_c X(i, c) X(j, c),  i >= j: the lower triangle of the next diagonal block (and the
//             right-hand side's row when it lies in these rows), X from LDS
// Both products are formed transposed (lane & 15 = the matrix ROW), so every global access is 128 contiguous bytes per 16 lanes.
// 512 threads = 8 waves.  The caller provides the waits (stage B: the tile of these rows final for panel k; stage C: every earlier
// update of the next diagonal tile applied) and the publish afterwards.
template <bool WT>
__device__ __forceinline__ void chol_chain_solve_rows(double* __restrict__ sm, double* __restrict__ M, long lda, long rows, int k0) {
  double* L = sm;
#define LL(i, j) L[(i) + (j) * kLdsPad]
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 15, kq = lane >> 4;
  const long r0 = (long)k0 + kNB;
  const long row = r0 + 16 * wave + r;
  const bool rv = row < rows;
  const double* ap = M + (rv ? row : rows - 1) + (long)(k0 + kq) * lda;
  double a[32];
#pragma unroll
  for (int s2 = 0; s2 < 32; ++s2) a[s2] = ap[(long)(4 * s2) * lda];
  double4_t acc[8];
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) acc[jb] = double4_t{0, 0, 0, 0};
#pragma unroll
  for (int s2 = 0; s2 < 32; ++s2) {
    const double av = rv ? a[s2] : 0.0;
    const int k = 4 * s2 + kq;
#pragma unroll
    for (int jb = 0; jb < 8; ++jb)
      if (4 * s2 < 16 * jb + 16) {   // Linv(c, k) = 0 for k > c (compile-time after unrolling)
        const int c = 16 * jb + r;
        const double lv = (k <= c) ? LL(c, k) : 0.0;
        acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(lv, av, acc[jb], 0, 0, 0);   // D[c = 4 g + kq][row = r]
      }
  }
  // X -> global memory: lane r = row, 16 lanes store 128 contiguous bytes of a column
  if constexpr (WT) {
#pragma unroll
    for (int jb = 0; jb < 8; jb += 2)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        chol_store_wt_pair(&M[row + (long)(k0 + 16 * jb + 4 * g + kq) * lda], &M[row + (long)(k0 + 16 * (jb + 1) + 4 * g + kq) * lda], acc[jb][g], acc[jb + 1][g], rv,
                           ((lda | (r0 + 16 * wave)) & 1) == 0);
  } else if (rv) {
#pragma unroll
    for (int jb = 0; jb < 8; ++jb)
#pragma unroll
      for (int g = 0; g < 4; ++g) chol_store<WT>(&M[row + (long)(k0 + 16 * jb + 4 * g + kq) * lda], acc[jb][g]);
  }
  __syncthreads();   // every wave has read Linv: the array now holds X (rows past the matrix as zeros)
#pragma unroll
  for (int jb = 0; jb < 8; ++jb)
#pragma unroll
    for (int g = 0; g < 4; ++g) LL(16 * wave + r, 16 * jb + 4 * g + kq) = rv ? acc[jb][g] : 0.0;
  __syncthreads();
#undef LL
}
// tiles (ib >= jb) of the next diagonal block owned by wave w: w, w + 8, ... of the 36, at most 5
__device__ __forceinline__ void chol_chain_tile(int tl, int& ib, int& jb) {
  ib = 0; int off = 0;
  while (off + ib + 1 <= tl) { off += ib + 1; ++ib; }
  jb = tl - off;
}
// the current values of the wave's entries of the next diagonal block, requested BEFORE the solve of the rows (every earlier update
// of that tile has been waited for by then): fetched one tile at a time in front of its own products, each was ~2 us of exposed
// latency, five in a row
struct CholChainC { double v[5][4]; };
__device__ __forceinline__ void chol_chain_prefetch_next(const double* __restrict__ M, long lda, long rows, int n, int k0, CholChainC& c) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
  const long c1 = (long)k0 + kNB;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int tl = wave + 8 * q;
    int ib, jb;
    chol_chain_tile(tl < 36 ? tl : 35, ib, jb);
    const long row = c1 + 16 * ib + r;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const long col = c1 + 16 * jb + 4 * g + kq;
      c.v[q][g] = M[(row < rows ? row : rows - 1) + (col < n ? col : (long)n - 1) * lda];
    }
  }
}
template <bool WT>
__device__ __forceinline__ void chol_chain_update_next(double* __restrict__ sm, double* __restrict__ M, long lda, long rows, int n, int k0,
                                                       const CholChainC& c) {
  double* L = sm;
#define LL(i, j) L[(i) + (j) * kLdsPad]
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 15, kq = lane >> 4;
  const long c1 = (long)k0 + kNB;   // first row AND first column of the next diagonal block
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int tl = wave + 8 * q;
    if (tl >= 36) break;
    int ib, jb;
    chol_chain_tile(tl, ib, jb);
    double4_t acc = {0, 0, 0, 0};
#pragma unroll 8
    for (int kk = 0; kk < kNB; kk += 4) {
      const double xj = LL(16 * jb + r, kk + kq), xi = LL(16 * ib + r, kk + kq);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xj, xi, acc, 0, 0, 0);   // D[j = 4 g + kq][i = r]
    }
    const long row = c1 + 16 * ib + r;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const long col = c1 + 16 * jb + 4 * g + kq;
      if (row < rows && col < n && row >= col) chol_store<WT>(&M[row + col * lda], c.v[q][g] - acc[g]);
    }
  }
#undef LL
}
static_assert(kP2Lds >= kCholLdsBig, "the persistent kernel's LDS is sized by the diagonal-block role");
constexpr int kPwThreads = 512, kPwGrid = 256;
// diagnostics of the persistent kernel (ESL_CHOL_TIMING=1 in the self test): per workgroup {ticks waiting on dependency words, ticks
// inside task bodies, tasks, first tick, last tick} of the last launch, wall_clock64 ticks (100 MHz)
__device__ long long g_chol_stats[kPwGrid * 5];
__device__ long long g_chol_chain_log[2 * 1024];
__device__ long long g_chol_fuse_ticks[4];   // fused chain stage, totals of the last launch: waits, row solve, next-block update, drain + publish   // per diagonal block: tick its tile was final, tick its factor was published
constexpr size_t kPwLds = kP2Lds + 64 + 256;   // + the task slot words and the diagnostics accumulators + the two halves' barrier counters (slot[16], slot[48])
static_assert(2 * kCholLdsV <= kP2Lds, "two halves' staging buffers");
// ONE kernel, two roles (round 4, second form): workgroup 0 is the chain, workgroups 1..255 the workers.  (The first form ran the two
// roles as two kernels on two streams: correct and as fast -- but whether two queues of one process run side by side or in turns
// is the scheduler's business: creating or destroying any stream while the pair ran made it time-slice them, each role then only
// moved during its own quantum, and an order-18,000 factorisation went from 42 ms to its 3 s spin limit.)  The 157 KB of LDS the
// diagonal-block role needs make every workgroup the only tenant of its CU -- which the 104 KB of the update role did anyway.
static __global__ __launch_bounds__(kPwThreads) void k_chol_persist(double* __restrict__ M, long lda, int n, int np, int W, int nR,
                                                                   double* __restrict__ Linv_ws, const CholTask* __restrict__ tasks,
                                                                   int n_tasks, const int* __restrict__ ns, int* sync, int* info, int fuse, int SP) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  int* slot = reinterpret_cast<int*>(sm + kP2Lds / sizeof(double));   // (behind the roles' LDS: no static __shared__, guide G17)
  long long* lstat = reinterpret_cast<long long*>(slot + 4);           // diagnostics accumulate in LDS, not in registers (see below)
  const bool stats = g_chol_stats_on != 0;
  if (stats && threadIdx.x == 0) { lstat[0] = lstat[1] = lstat[2] = 0; lstat[3] = (long long)wall_clock64(); if (blockIdx.x == 0) { g_chol_fuse_ticks[0] = g_chol_fuse_ticks[1] = g_chol_fuse_ticks[2] = g_chol_fuse_ticks[3] = 0; } }
  int* pdone = sync + 4;
  int* sdone = pdone + np;
  int* ver = sdone + (size_t)np * nR;
  int* qdone = ver + (size_t)np * nR;
  const int t = threadIdx.x;
  const long rows = (long)n + 1;
  // the chain is whichever workgroup gets here FIRST (a ticket in sync[2]), not blockIdx 0: the workers' waits end only if the chain
  // is resident, and nothing guarantees that the dispatcher starts with block 0 (guide G16: no dispatch-order assumption)
  if (t == 0) { slot[2] = __hip_atomic_fetch_add(sync + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); slot[14] = 0; slot[15] = 0; }
  __syncthreads();
  const bool is_chain = slot[2] == 0;
  if (is_chain) {   // ---- the chain: diagonal blocks in order
    bool have_next = false;   // fused: block k already carries every update (the previous step applied the last one itself)
    for (int k = 0; k < np; ++k) {
      const int k0 = k * kNB, nb = (n - k0 < kNB) ? (n - k0) : kNB;
      if (t == 0) {
        const long long tw = stats ? (long long)wall_clock64() : 0;
        const bool ok = have_next || chol_wait_ge<2>(&ver[(size_t)(k / 2) * np + k], chol_tile_final(k / 2, k, W, SP), sync + 1, info);   // every update of the diagonal block's tile is in
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        slot[0] = ok ? 1 : 0;
        if (stats) { const long long now = (long long)wall_clock64(); lstat[0] += now - tw; lstat[4] = now; if (k < 1024) g_chol_chain_log[2 * k] = now; }
      }
      __syncthreads();
      if (!slot[0]) return;
      chol_potrf2_body<true, kPwThreads>(sm, M, lda, k0, nb, Linv_ws + (size_t)k * kNB * kNB, info);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its write-through stores ...
      __syncthreads();
      if (t == 0) {
        __hip_atomic_store(&pdone[k], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... then ONE lane publishes
        if (stats) { const long long now = (long long)wall_clock64(); lstat[1] += now - lstat[4]; lstat[2] += 1; if (k < 1024) g_chol_chain_log[2 * k + 1] = now; }
      }
      have_next = false;
      const long below = rows - ((long)k0 + nb);
      if (fuse && below > 0) {
        // the rows under the block (strips 0, 1 of panel k: a full panel -- only the last one is short, and it has just the
        // right-hand side's row under it, which the same code handles) and the next diagonal block: chol_chain_solve_rows / _update_next
        const int R1 = (int)(((long)k0 + nb) / 256);
        const int nstr = below > 64 ? 2 : 1;
        const bool next = k + 1 < np;
        if (t == 0) {
          const long long tw = stats ? (long long)wall_clock64() : 0;
          bool ok = chol_wait_ge<2>(&ver[(size_t)R1 * np + k], chol_tile_final(R1, k, W, SP), sync + 1, info);
          if (ok && next) ok = chol_wait_ge<2>(&ver[(size_t)((k + 1) / 2) * np + k + 1], chol_tile_seq((k + 1) / 2, k + 1, W, SP, k), sync + 1, info);
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          slot[0] = ok ? 1 : 0;
          if (stats) { const long long now = (long long)wall_clock64(); lstat[0] += now - tw; g_chol_fuse_ticks[0] += now - tw; lstat[4] = now; }
        }
        __syncthreads();
        if (!slot[0]) return;
        CholChainC cnext;
        if (next) chol_chain_prefetch_next(M, lda, rows, n, k0, cnext);
        if (nb == kNB) chol_chain_solve_rows<true>(sm, M, lda, rows, k0);
        else {   // the short last panel: one row (the right-hand side's) against a partial inverse -- the strip body
          chol_panel_body<true>(M, lda, rows, k0, nb, Linv_ws + (size_t)k * kNB * kNB, 0L);
        }
        if (stats && t == 0) { const long long now = (long long)wall_clock64(); g_chol_fuse_ticks[1] += now - lstat[4]; lstat[4] = now; }
        if (next) chol_chain_update_next<true>(sm, M, lda, rows, n, k0, cnext);
        if (stats && t == 0) { const long long now = (long long)wall_clock64(); g_chol_fuse_ticks[2] += now - lstat[4]; lstat[4] = now; }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
          if (stats) { const long long now = (long long)wall_clock64(); g_chol_fuse_ticks[3] += now - lstat[4]; }
          __hip_atomic_fetch_add(&sdone[(size_t)k * nR + R1], nstr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (next) {
            // panel k's update of tile ((k + 1) / 2, k + 1): the workers' quarters (the half that is not the diagonal block) move the
            // sequence number on when they are done; when there are none (k + 1 odd: the other half lies above the diagonal) the chain does
            const int J = k + 1, R = J / 2;
            int mine = 0;
            for (int q = 0; q < 4; ++q) if ((q & 1) != (J & 1) && chol_quarter_live(R, J, q & 1, q >> 1, rows, n)) ++mine;
            if (mine == 0) __hip_atomic_store(&ver[(size_t)R * np + J], chol_tile_seq(R, J, W, SP, k) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        have_next = next;
      }
    }
    if (stats && t == 0) { for (int q = 0; q < 4; ++q) g_chol_stats[q] = lstat[q]; g_chol_stats[4] = (long long)wall_clock64(); }
    return;
  }
  for (;;) {               // ---- a worker: the next task of the list
    // (nothing but the kernel arguments is live across a task body: the task is re-read from the list afterwards -- with the
    //  descriptor, the publish address and the diagnostics kept in registers the update tile's 212 spilled 60 B per lane)
    if (t == 0) {
      if (slot[14] > 0) { slot[14] -= 1; slot[15] += 1; }   // the next strip of the task in hand: no new task, no waits, no publish in between
      else { slot[0] = __hip_atomic_fetch_add(sync, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); slot[15] = 0; }
    }
    __syncthreads();
    if (slot[0] >= n_tasks) {
      if (stats && t == 0) { const int me = slot[2] < kPwGrid ? slot[2] : kPwGrid - 1; for (int q = 0; q < 4; ++q) g_chol_stats[5 * me + q] = lstat[q]; g_chol_stats[5 * me + 4] = (long long)wall_clock64(); }
      return;
    }
    if (t == 0 && slot[15] == 0) {
      const CholTask tk = tasks[slot[0]];
      bool ok = true;
      const long long tw = stats ? (long long)wall_clock64() : 0;
      slot[14] = (tk.type == 0 && tk.c > 1) ? tk.c - 1 : 0;   // strips of this task after the first
      if (tk.type == 0) {
        const int k = tk.a, k0 = k * kNB, nb = (n - k0 < kNB) ? (n - k0) : kNB;
        const int R = (int)(((long)k0 + nb + 64L * tk.b) / 256);
        ok = chol_wait_ge<100>(&pdone[k], 1, sync + 1, info) && chol_wait_ge<100>(&ver[(size_t)R * np + k], chol_tile_final(R, k, W, SP), sync + 1, info);
      } else {
        const int R = tk.b, J = tk.c & 0xffff;
        const int cnt = (tk.type == 2) ? (tk.c >> 16) : 1;   // type 2: outer panels [a, a + cnt) in one visit
        const int ke = (tk.type != 2) ? tk.a + 1 : (((tk.a + cnt) * W < np) ? (tk.a + cnt) * W : np);
        // the LAST panel's strips of a row tile are solved only after every earlier panel of the same outer panel has solved its own
        // there and updated them (S waits for its tile to be final): one pair of words stands for all W panels
        // the three words are fetched TOGETHER first (agent-scope loads go to the fabric, ~1.5 us each one after the other; most
        // tasks find all three satisfied) and only the unsatisfied ones enter the polling wait
        int* w0 = &sdone[(size_t)(ke - 1) * nR + R];
        int* w1 = &sdone[(size_t)(ke - 1) * nR + J / 2];
        int* w2 = &ver[(size_t)R * np + J];
        const int want0 = ns[(size_t)(ke - 1) * nR + R], want1 = ns[(size_t)(ke - 1) * nR + J / 2];
        const int seq = (tk.type != 2) ? chol_tile_seq(R, J, W, SP, tk.a) : tk.a;
        const int v0 = __hip_atomic_load(w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), v1 = __hip_atomic_load(w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                  v2 = __hip_atomic_load(w2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = (v0 >= want0 || chol_wait_ge<100>(w0, want0, sync + 1, info)) && (v1 >= want1 || chol_wait_ge<100>(w1, want1, sync + 1, info)) &&
             (v2 >= seq || chol_wait_ge<100>(w2, seq, sync + 1, info));
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      slot[1] = ok ? 1 : 0;
      slot[16] = 0; slot[48] = 0;   // the halves' barrier counters (chol_update_tile_v<.., 1>): every wave of the previous task is behind its last barrier
      if (stats) { const long long now = (long long)wall_clock64(); lstat[0] += now - tw; lstat[4] = now; }
    }
    __syncthreads();
    if (!slot[1]) return;
    {
      const CholTask tk = tasks[slot[0]];
      if (tk.type == 0) {
        const int k = tk.a, k0 = k * kNB, nb = (n - k0 < kNB) ? (n - k0) : kNB;
        // (a task of several strips -- tk.c, one row tile's -- comes back here once per strip without leaving the task: slot[15] = the strip
        //  it is at.  A loop around this body cost the merged kernel 540 B of scratch per lane, K loops included: 37.7 -> 46.7 ms.)
        chol_panel_body<true>(M, lda, rows, k0, nb, Linv_ws + (size_t)k * kNB * kNB, (long)(tk.b + slot[15]));
      } else {
        const int cnt = (tk.type == 2) ? (tk.c >> 16) : 1;
        const int kb = (tk.type != 2) ? tk.a : tk.a * W, ke = (tk.type != 2) ? tk.a + 1 : (((tk.a + cnt) * W < np) ? (tk.a + cnt) * W : np);
        const long c0 = (long)kb * kNB;
        const int K = (int)(((long)ke * kNB < n ? (long)ke * kNB : (long)n) - c0);
        if (tk.type == 3)
          chol_update_tile<128, 64, 4, 2, true>(sm, M, lda, rows, (long)n, M + c0 * lda, lda, K, 256L * tk.b + 128L * ((tk.c >> 16) & 1),
                                                128L * (tk.c & 0xffff) + 64L * ((tk.c >> 17) & 1), false);
        else {
          {
          // round 6: the two halves of the workgroup take the tile's upper and lower 128 rows independently (chol_update_tile_v, HV = 1;
          // the eight-wave chol_update_tile<256, 128> in its place, a compile-time A/B until DESIGN 4.17: 86.4 against 89.7 % of the MFMA peak in the probe)
          const int hv = chol_uniform(t >> 8), Ku = chol_uniform(K);
          const long ih = 256L * chol_uniform(tk.b) + 128L * hv, jh = 128L * chol_uniform(tk.c & 0xffff), c0u = chol_uniform(c0);
          if (ih < rows && jh <= ih + 127)   // (a half under the matrix or above the diagonal has nothing to do)
            chol_update_tile_v<true, 1>(sm + hv * (2 * kKC * kVLd), M, lda, rows, (long)n, M + c0u * lda, lda, Ku, ih, jh, false, slot + 16 + 32 * hv);
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its write-through stores ...
    __syncthreads();
    if (t == 0 && slot[14] == 0) {                        // ... then ONE lane publishes (a task of several strips: after its last)
      const CholTask tk = tasks[slot[0]];
      if (tk.type == 0) {
        const int k = tk.a, k0 = k * kNB, nb = (n - k0 < kNB) ? (n - k0) : kNB;
        __hip_atomic_fetch_add(&sdone[(size_t)k * nR + (size_t)(((long)k0 + nb + 64L * tk.b) / 256)], tk.c > 1 ? tk.c : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else if (tk.type == 3) {
        // quarters of ONE update run side by side; the one that completes the set moves the tile's sequence number on.  (The counter
        // only grows: panel a is the (a % W + 1)-th rank-128 update of this tile, which belongs to a's own outer panel.)
        const int J = tk.c & 0xffff, mine = (tk.c >> 18) & 7, full = (tk.c >> 21) & 7;
        const int old = __hip_atomic_fetch_add(&qdone[(size_t)tk.b * np + J], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1 == full * chol_tile_ridx(tk.b, J, W, SP, tk.a) + mine)
          __hip_atomic_store(&ver[(size_t)tk.b * np + J], chol_tile_seq(tk.b, J, W, SP, tk.a) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        const int J = tk.c & 0xffff;
        __hip_atomic_store(&ver[(size_t)tk.b * np + J], (tk.type == 1) ? chol_tile_seq(tk.b, J, W, SP, tk.a) + 1 : tk.a + (tk.c >> 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (stats) { lstat[1] += (long long)wall_clock64() - lstat[4]; lstat[2] += 1; }
    }
    __syncthreads();                                      // (slot[0] is free for the next task)
  }
}

}  // namespace esl
