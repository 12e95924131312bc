// esl_chol_kernels.hpp — device code of the launch-per-step dense Cholesky (see esl_chol.hpp for the method and the layout):
// diagonal block (k_chol_potrf2), panel solve (k_chol_panel), the two rank-K update tiles (k_chol_update_lds, k_chol_update_v), the
// one-workgroup solve of small systems (k_chol_small), the back-substitution kernels, and the pack / split-K helpers.  The bodies
// (chol_potrf2_body, chol_panel_body, chol_update_tile, chol_update_tile_v) are shared with k_chol_persist (esl_chol_persist.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace esl {

constexpr int kNB = 128;       // panel width
constexpr int kLdsPad = 129;   // column stride of the LDS copy of the diagonal block (bank-conflict pad)

typedef double double4_t __attribute__((ext_vector_type(4)));

// ---- diagonal block -----------------------------------------------------------------------------------------
// info[0] |= 1 when a pivot is not positive (g2o: LDLT not positive => solve fails => step rejected).
constexpr int kSB = 32;   // (LDS sizing only: the 96 x 32 temporary of the triangular inverse)
// diagnostic: wall_clock64() marks (100 MHz) of the last k_chol_potrf2 launch, read by esl_selftest_cholesky when
// ESL_CHOL_TIMING is set
__device__ long long g_potrf_clk[16];
#define POTRF_MARK(k) do { if (t == 0) g_potrf_clk[k] = (long long)wall_clock64(); } while (0)
// ---- k_chol_potrf2: right-looking over the WHOLE 128 x 128 block in rank-4 steps ------------------------------------------------
// 528 threads each OWN a 4 x 4 block of the lower triangle in 16 registers for the whole factorisation; only the current block
// column (4 x 128 doubles) and the inverse of its diagonal block (10 doubles) travel through LDS.  32 steps of two barriers each
// (see the loop).  History of this kernel, n = 2,994 factor + solve: blocked form of round 1 (k_chol_potrf: 32 x 32 sub-blocks
// factored by one wave with v_readlane broadcasts) 4.5 ms; one column per step with one barrier (590 ns per column, all of it
// latency of LDS write -> 10-wave barrier -> LDS read) 4.0 ms; rank-4 steps (column loop 76 -> 28 us, kernel 118 -> 72 us) 2.86 ms.  Around the loop: every thread
// fetches its own block (load 10 -> 2 us) and writes its part of L back from registers; the triangular inverse is computed in
// place by recursive doubling from the 4 x 4 inverses the factorisation produces anyway (see below).
// (Also measured: round 1's blocked loop moved into this kernel's frame on eight waves with the sub-block inverses
// overlapped -- slower, 4.9 ms: at two waves per SIMD and 244 registers the wave-synchronous column steps went 12 -> 17 us.
// Round 1's kernel itself was deleted in round 3 after its equivalence runs.)
constexpr int kP2Threads = 640;
// WT: L and Linv leave with write-through (sc1) stores -- the persistent factorisation hands them to other workgroups inside the launch
template <bool WT>
__device__ __forceinline__ void chol_store(double* p, double v) {
  if constexpr (WT) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else *p = v;
}
// Write-through stores in PAIRS (round 6).  An 8-byte sc1 store costs 2.7 x a 16-byte one per byte (the guide's store table), and in the
// product layouts of this file a lane holds ONE row: 16 lanes = 16 consecutive rows of a column.  Two values of the lane's row that belong
// to two different columns (x -> column a, y -> column b) are exchanged with the neighbouring lane (lane ^ 1: rows 2 m, 2 m + 1) so that
// the even lane stores rows {2 m, 2 m + 1} of column a and the odd lane the same rows of column b, 16 bytes each: half the store
// instructions, all of them wide.  `pa`, `pb`: this lane's own addresses of (row, a) and (row, b); `ok`: the lane's row is inside the
// matrix; `wide`: 16-byte alignment holds (even leading dimension and even first row).  A pair whose second row is outside falls
// back to 8-byte stores.  The inline-assembly store carries the wait states of the wide-store data hazard (see chol_update_tile_v).
// (Against the 8-byte form, a compile-time A/B until DESIGN 4.17: k_chol_persist 36.4 -> 35.7 - 35.8 ms in the bench, together with the update tile's.)
__device__ __forceinline__ double chol_xchg_lane1(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0xB1, 0xF, 0xF, true), hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0xB1, 0xF, 0xF, true);   // quad_perm [1, 0, 3, 2]
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void chol_store_wt_pair(double* pa, double* pb, double x, double y, bool ok, bool wide) {
  typedef double double2_t __attribute__((ext_vector_type(2)));
  const bool odd = (threadIdx.x & 1) != 0;
  const double got = chol_xchg_lane1(odd ? x : y);
  const bool nb_ok = __builtin_amdgcn_mov_dpp((int)ok, 0xB1, 0xF, 0xF, true) != 0;
  if (wide && ok && nb_ok) {
    double* p = odd ? pb - 1 : pa;
    const double2_t v = odd ? double2_t{got, y} : double2_t{x, got};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
  } else if (ok) {
    chol_store<true>(pa, x);
    chol_store<true>(pb, y);
  }
}
// ---- the triangular inverse of the factored diagonal block, in place in the LDS copy (see chol_potrf2_body) -------------------------------
// A function of its own, NOT inlined (round 6): inlined into k_chol_persist its register pressure (two tile columns of double4 accumulators)
// moved the merged kernel's allocation and the chain's fused row solve picked up spills -- 15.5 -> 24.7 us per panel, which ate the
// 8 us the inverse had gained.  The LDS copy is reached through the kernel's one dynamic-LDS symbol (offset 0), not through a pointer
// argument (that would decay to flat addressing).
template <int NT>
static __device__ __attribute__((noinline)) void chol_inv_levels() {
  extern __shared__ __attribute__((aligned(16))) double sm_inv[];
  double* L = sm_inv;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#define LL(i, j) L[(i) + (j) * kLdsPad]
  // ---- Linv = L^-1 IN PLACE by recursive doubling: the inverse of [A 0; C D] is [A^-1 0; -D^-1 C A^-1  D^-1].  Level b merges
  // pairs of adjacent b x b diagonal inverses; C (original L) is overwritten by its block of the inverse, which no later level
  // reads as L.  Rounds 3-5: b = 4, 8 one thread per output entry; b = 16, 32, 64 two MFMA products, the intermediate T = C A^-1 parked
  // in the (unused) block above the diagonal that mirrors C; 8 barriers in all, against the 32-step triangular inverses of
  // the four 32 x 32 sub-blocks + 3 dependent block columns of the blocked form (25.6 -> 16.4 us; n = 2,994 2.86 -> 2.60 ms).
  // Round 6: every level on the matrix cores, and no intermediate through LDS.  In the f64 MFMA layout the D fragment of the first product
  // (T = C A^-1: lane (r, kq), register g = T[kq + 4 g][r]) IS the B fragment of k-step g of the second (X = D^-1 T wants T[4 g + kq][r]):
  // a wave that computes a tile column of T keeps it in registers and goes straight on to the same tile column of X.
  //   levels 4, 8   wave s < 8 owns the 16 x 16 diagonal super-block s; the level's C / A^-1 / D^-1 positions are selected by index masks
  //                 and the two products are 4 + 4 MFMAs on the whole super-block (block-diagonal operands), wave-local: no barrier
  //                 between the two levels (LDS operations of one wave complete in order)
  //   level 16      four groups, one wave each: 4 + 4 MFMAs
  //   levels 32, 64 (group, tile column) per wave: the column's tiles of T, then of X, all in registers; one barrier before C is overwritten
  // 16.4 -> ~6 us (the one-entry-per-thread loops of levels 4, 8 were 5.1 us, the per-MFMA LDS round trips of the others 10.9).
  {
    const int r = lane & 15, kq = lane >> 4;
    if (wave < 8) {
      const int s0 = 16 * wave;
#pragma unroll
      for (int b = 4; b <= 8; b *= 2) {
        // position classes of the level inside the super-block: same 2b-group, (upper | lower) half of it
        auto grp = [b](int i) { return i / (2 * b); };
        auto low = [b](int i) { return (i / b) & 1; };
        double4_t tt = {0, 0, 0, 0}, xx = {0, 0, 0, 0};
        double av[4], bv[4], dv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int k = 4 * g + kq;
          const bool cpos = grp(r) == grp(k) && low(r) == 1 && low(k) == 0;             // C(i = r, k)
          const bool apos = grp(k) == grp(r) && low(k) == 0 && low(r) == 0 && k >= r;   // A^-1(k, j = r), lower
          const bool dpos = grp(r) == grp(k) && low(r) == 1 && low(k) == 1 && k <= r;   // D^-1(i = r, m = k), lower
          const double vc = LL(s0 + r, s0 + k), va = LL(s0 + k, s0 + r);
          av[g] = cpos ? vc : 0.0; bv[g] = apos ? va : 0.0; dv[g] = dpos ? vc : 0.0;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) tt = __builtin_amdgcn_mfma_f64_16x16x4f64(av[g], bv[g], tt, 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) xx = __builtin_amdgcn_mfma_f64_16x16x4f64(dv[g], tt[g], xx, 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int i = kq + 4 * g;
          if (grp(i) == grp(r) && low(i) == 1 && low(r) == 0) LL(s0 + i, s0 + r) = -xx[g];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the wave's own writes, before its own reads of the next level)
        __builtin_amdgcn_wave_barrier();
      }
    }
    __syncthreads();
    if (t == 0) g_potrf_clk[14] = (long long)wall_clock64();   // (diagnostic: end of levels 4, 8)
    if (wave < 4) {   // level 16: group `wave`, rows / columns [32 wave, 32 wave + 32)
      const int r0 = 32 * wave;
      double4_t tt = {0, 0, 0, 0}, xx = {0, 0, 0, 0};
      double av[4], bv[4], dv[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k = 4 * g + kq;
        av[g] = LL(r0 + 16 + r, r0 + k);
        const double va = LL(r0 + k, r0 + r), vd = LL(r0 + 16 + r, r0 + 16 + k);
        bv[g] = (k >= r) ? va : 0.0; dv[g] = (k <= r) ? vd : 0.0;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) tt = __builtin_amdgcn_mfma_f64_16x16x4f64(av[g], bv[g], tt, 0, 0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) xx = __builtin_amdgcn_mfma_f64_16x16x4f64(dv[g], tt[g], xx, 0, 0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) LL(r0 + 16 + kq + 4 * g, r0 + r) = -xx[g];   // (C's own wave: nobody else reads this group)
    }
    __syncthreads();
    if (t == 0) g_potrf_clk[15] = (long long)wall_clock64();   // (diagnostic: end of level 16)
    auto level_cols = [&](auto bc) {
      constexpr int B = decltype(bc)::value, NTL = B / 16;   // (kNB / (2 B)) x NTL = 4 wave tasks at both levels
      double4_t X[NTL];
      const int mg = wave / NTL, jb = wave % NTL, r0 = mg * 2 * B;
      if (wave < 4) {
        double4_t Tc[NTL];
#pragma unroll
        for (int m = 0; m < NTL; ++m) { Tc[m] = double4_t{0, 0, 0, 0}; X[m] = double4_t{0, 0, 0, 0}; }
        const int j = jb * 16 + r;
        // T(:, jb) = C(:, k) A^-1(k, jb), k from the column's own tile on (A^-1 is lower); operands of step kk + 4 in flight under step kk
        double an[NTL], bn, ac[NTL], bc2;
        {
          const int k = jb * 16 + kq;
          const double va = LL(r0 + k, r0 + j);
          bc2 = (k >= j) ? va : 0.0;
#pragma unroll
          for (int m = 0; m < NTL; ++m) ac[m] = LL(r0 + B + m * 16 + r, r0 + k);
        }
        for (int kk = jb * 16; kk < B; kk += 4) {
          const int k = (kk + 4 < B ? kk + 4 : kk) + kq;
          const double va = LL(r0 + k, r0 + j);
          bn = (k >= j) ? va : 0.0;
#pragma unroll
          for (int m = 0; m < NTL; ++m) an[m] = LL(r0 + B + m * 16 + r, r0 + k);
#pragma unroll
          for (int m = 0; m < NTL; ++m) Tc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[m], bc2, Tc[m], 0, 0, 0);
          bc2 = bn;
#pragma unroll
          for (int m = 0; m < NTL; ++m) ac[m] = an[m];
        }
        // X(ib, jb) = D^-1(ib, m) T(m, jb), m <= ib
#pragma unroll
        for (int ib = 0; ib < NTL; ++ib) {
          const int i = ib * 16 + r;
#pragma unroll
          for (int m = 0; m <= ib; ++m) {
            double dv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int mm = m * 16 + 4 * g + kq;
              const double vd = LL(r0 + B + i, r0 + B + mm);
              dv[g] = (mm <= i) ? vd : 0.0;
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) X[ib] = __builtin_amdgcn_mfma_f64_16x16x4f64(dv[g], Tc[m][g], X[ib], 0, 0, 0);
          }
        }
      }
      __syncthreads();   // every column's reads of C are done
      if (wave < 4) {
#pragma unroll
        for (int ib = 0; ib < NTL; ++ib)
#pragma unroll
          for (int g = 0; g < 4; ++g) LL(r0 + B + ib * 16 + kq + 4 * g, r0 + jb * 16 + r) = -X[ib][g];
      }
      __syncthreads();
    };
    level_cols(std::integral_constant<int, 32>{});
    level_cols(std::integral_constant<int, 64>{});
  }
#undef LL
}
// NT = 640: every one of the 528 blocks has its own thread (the stand-alone kernel).  NT = 512 (the persistent kernel's workgroup
// shape): threads 0..15 own TWO blocks one after the other -- their first one lies in block column 0 and is final after step 0, so
// they store it there and then (global memory + the LDS copy) and take over blocks 512..527 (block columns 26..31, which only see
// work at the very end) in time for step 0's rank-4 update.
template <bool WT, int NT = kP2Threads>
__device__ __forceinline__ void chol_potrf2_body(double* __restrict__ sm, double* __restrict__ M, long lda, int k0, int nb,
                                                 double* __restrict__ Linv /* kNB x kNB col-major */, int* __restrict__ info) {
  static_assert(NT == 640 || NT == 512, "potrf2: 640 or 512 threads");
  double* L = sm;                          // kNB x kNB, column stride kLdsPad: the factor, later its inverse
  double* T = sm + kNB * kLdsPad;          // 96 x 32 temporary of the inverse; the column buffers of the factorisation before that
  double* dinv = T + 96 * kSB;             // kNB reciprocals of the diagonal
  const int t = threadIdx.x;
#define LL(i, j) L[(i) + (j) * kLdsPad]
  POTRF_MARK(0);
  // the thread's 4 x 4 block (bi >= bj) of the 32 x 32 grid of blocks, enumerated column by column: the blocks of the first
  // block columns are finished first, so whole waves drop out of the update as the factorisation moves right
  const bool own = t < 528;
  int bi = 0, bj = 0;
  auto block_of = [](int idx, int& obi, int& obj) {
    int off = 0; obj = 0;
    while (off + (32 - obj) <= idx) { off += 32 - obj; ++obj; }
    obi = obj + (idx - off);
  };
  if (own) block_of(t, bi, bj);
  double a[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * bi + r, j = 4 * bj + c;
      a[r][c] = (own && i < nb && j < nb && i >= j) ? M[(long)(k0 + i) + (long)(k0 + j) * lda] : ((i == j) ? 1.0 : 0.0);   // identity padding
    }
  // NT = 512: the second block of threads 0..15 is fetched NOW, with everything else (fetched at the hand-over inside step 0 it was a
  // global round trip on the critical path of the whole workgroup: 4 - 6 us of the chain's every step)
  double a2[4][4];
  int bi2 = 0, bj2 = 0;
  if constexpr (NT == 512) {
    if (t < 16) block_of(512 + t, bi2, bj2);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * bi2 + r, j = 4 * bj2 + c;
        a2[r][c] = (t < 16 && i < nb && j < nb && i >= j) ? M[(long)(k0 + i) + (long)(k0 + j) * lda] : ((i == j) ? 1.0 : 0.0);
      }
  }
  // Rank-4 steps: block column J = the four columns of the 4 x 4 blocks (., J).  Per step, two barriers instead of four:
  //   (a) the owner of the diagonal block (J, J) factors it in registers (four dependent rsqrt chains) and publishes its
  //       inverse (10 numbers)                                                                       -> barrier A
  //   (b) the blocks below it solve X = A L_JJ^-T with that inverse, keep X (their part of L) and publish its four columns
  //                                                                                                   -> barrier B
  //   (c) every block to the right subtracts the rank-4 product of its rows' and its columns' entries; the owner of the NEXT
  //       diagonal block goes straight on to (a), so barrier A of step J + 1 is the barrier that ends step J.
  double* colbuf = T;                      // [4][kNB]: the four columns of the current block column (rows below the diagonal block)
  double* dblk = T + 4 * kNB;              // [10]: inverse of the current diagonal block, packed rows (0,0) (1,0) (1,1) (2,0) ...
  double xd[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};   // diagonal-block owners: the inverse of their factored block
  // 4 x 4 Cholesky of the thread's own block (lower triangle), in place; returns the inverse of the factor, publishes 1 / L(c,c)
  auto factor_diag = [&](int J) {
    double is[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double d = a[c][c];
#pragma unroll
      for (int k = 0; k < c; ++k) d -= a[c][k] * a[c][k];
      if (!(d > 0)) atomicOr(info, 1);
      double r = __builtin_amdgcn_rsq(d);   // 1/sqrt(d): hardware estimate + two Newton steps (no fp64 sqrt, no divide)
      r = r * (1.5 - 0.5 * d * r * r);
      r = r * (1.5 - 0.5 * d * r * r);
      is[c] = r;
      a[c][c] = d * r;
#pragma unroll
      for (int rr = c + 1; rr < 4; ++rr) {
        double v = a[rr][c];
#pragma unroll
        for (int k = 0; k < c; ++k) v -= a[rr][k] * a[c][k];
        a[rr][c] = v * r;
      }
      dinv[4 * J + c] = r;
    }
    // X = L^-1 (lower): X(c,c) = 1 / L(c,c), X(r,c) = -(sum_{k=c}^{r-1} L(r,k) X(k,c)) / L(r,r)
    double x[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      x[c][c] = is[c];
#pragma unroll
      for (int rr = c + 1; rr < 4; ++rr) {
        double v = 0;
#pragma unroll
        for (int k = c; k < rr; ++k) v += a[rr][k] * x[k][c];
        x[rr][c] = -v * is[rr];
      }
    }
    int q = 0;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
      for (int c = 0; c <= rr; ++c) { dblk[q++] = x[rr][c]; xd[rr][c] = x[rr][c]; }
  };
  if (own && bi == 0 && bj == 0) factor_diag(0);
  __syncthreads();                                      // barrier A of step 0
  POTRF_MARK(1);
  for (int J = 0; J < kNB / 4; ++J) {
    if (t == 0 && (J == 1 || J == 8 || J == 16 || J == 24)) g_potrf_clk[10 + (J + 7) / 8 - (J == 1 ? 1 : 0)] = (long long)wall_clock64();   // (diagnostic: 10 = J 1, 11 = J 8, 12 = J 16, 13 = J 24)
    if (own && bj == J && bi > J) {                     // (b) X = A L_JJ^-T: X(r,c) = sum_{k <= c} A(r,k) Linv(c,k)
      double li[10];
#pragma unroll
      for (int q = 0; q < 10; ++q) li[q] = dblk[q];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double a0 = a[r][0], a1 = a[r][1], a2 = a[r][2], a3 = a[r][3];
        a[r][0] = a0 * li[0];
        a[r][1] = a0 * li[1] + a1 * li[2];
        a[r][2] = a0 * li[3] + a1 * li[4] + a2 * li[5];
        a[r][3] = a0 * li[6] + a1 * li[7] + a2 * li[8] + a3 * li[9];
      }
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) colbuf[c * kNB + 4 * bi + r] = a[r][c];
    }
    __syncthreads();                                    // barrier B
    if constexpr (NT == 512) {
      if (J == 0 && t < 16) {   // first block (t, 0) is final: store it, take over block 512 + t (original values; step 0's update follows)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 4 * bi + r, j = c;
            if (i >= j) {
              if (i < nb && j < nb) chol_store<WT>(&M[(long)(k0 + i) + (long)(k0 + j) * lda], a[r][c]);
              LL(i, j) = (bi == 0) ? xd[r][c] : a[r][c];
            }
          }
        bi = bi2; bj = bj2;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) a[r][c] = a2[r][c];
      }
    }
    if (own && bj > J) {                                // (c) rank-4 update
      double rv[4][4], cv[4][4];                        // [k][r]: entries of column k of the block column in this block's rows / columns
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) { rv[k][r] = colbuf[k * kNB + 4 * bi + r]; cv[k][r] = colbuf[k * kNB + 4 * bj + r]; }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double v = a[r][c];
#pragma unroll
          for (int k = 0; k < 4; ++k) v -= rv[k][r] * cv[k][c];
          a[r][c] = v;
        }
      if (bi == bj && bj == J + 1) factor_diag(J + 1);  // (a) of the next step
    }
    __syncthreads();                                    // barrier A of step J + 1
  }
  POTRF_MARK(2); POTRF_MARK(3); POTRF_MARK(4);   // (marks 2..4 of the blocked form collapse: the whole column loop is "factor32[0]")
  // L11 back to memory straight from the owners' registers (the factor itself is part of the result), and into LDS for the
  // inverse: off-diagonal 4 x 4 blocks as they are, diagonal blocks as their INVERSES (computed during the factorisation)
  if (own) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * bi + r, j = 4 * bj + c;
        if (i >= j) {
          if constexpr (WT) {
            // write-through: the block's rows (2 p, 2 p + 1) of a column as one 16-byte store where both are stored (see chol_store_wt_pair)
            const bool pair = (r & 1) == 0 ? (i + 1 < nb && j < nb && (lda & 1) == 0) : (i - 1 >= j && i < nb && j < nb && (lda & 1) == 0);
            if (pair) {
              if ((r & 1) == 0) {
                typedef double double2_t __attribute__((ext_vector_type(2)));
                const double2_t v = double2_t{a[r][c], a[r | 1][c]};
                asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(&M[(long)(k0 + i) + (long)(k0 + j) * lda]), "v"(v) : "memory");
              }
            } else if (i < nb && j < nb) chol_store<WT>(&M[(long)(k0 + i) + (long)(k0 + j) * lda], a[r][c]);
          } else if (i < nb && j < nb) chol_store<WT>(&M[(long)(k0 + i) + (long)(k0 + j) * lda], a[r][c]);
          LL(i, j) = (bi == bj) ? xd[r][c] : a[r][c];
        }
      }
  }
  __syncthreads();
  POTRF_MARK(5); POTRF_MARK(6); POTRF_MARK(7);
  chol_inv_levels<NT>();
  POTRF_MARK(8);
  if constexpr (WT) {   // (write-through: 16-byte stores, see chol_store_wt_pair; the workspace is 16-byte aligned, kNB is even)
    typedef double double2_t __attribute__((ext_vector_type(2)));
    for (int idx = 2 * t; idx < kNB * kNB; idx += 2 * NT) {
      const int i = idx % kNB, j = idx / kNB;
      const double2_t v = double2_t{(i < nb && j < nb && i >= j) ? LL(i, j) : 0.0, (i + 1 < nb && j < nb && i + 1 >= j) ? LL(i + 1, j) : 0.0};
      asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(&Linv[idx]), "v"(v) : "memory");
    }
  } else
  for (int idx = t; idx < kNB * kNB; idx += NT) {
    const int i = idx % kNB, j = idx / kNB;
    chol_store<WT>(&Linv[idx], (i < nb && j < nb && i >= j) ? LL(i, j) : 0.0);
  }
  POTRF_MARK(9);
#undef LL
}
constexpr size_t kP2Lds = (size_t)(kNB * kLdsPad + 96 * kSB + kNB) * sizeof(double);
static __global__ __launch_bounds__(kP2Threads) void k_chol_potrf2(double* __restrict__ M, long lda, int k0, int nb,
                                                            double* __restrict__ Linv /* kNB x kNB col-major */,
                                                            int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  chol_potrf2_body<false, kP2Threads>(sm, M, lda, k0, nb, Linv, info);
}

// ---- panel solve: P <- P * Linv^T for rows [r0, rows) of columns [k0, k0+nb) -------------------------------
// One WORKGROUP owns 64 rows x all kNB columns; its 8 waves take 32 x 32 sub-tiles (2 row groups x 4 column groups), so a
// wave's dependent chain is 128 MFMAs, not the 1,024 of the first version (one wave per 64 rows x 128 columns: 86 us per
// launch whatever the height of the panel).  The rows are updated in place: every wave reads all K input columns of its
// rows, the barrier makes sure all of the workgroup's reads are done before anybody writes.
template <bool WT>
__device__ __forceinline__ void chol_panel_body(double* __restrict__ M, long lda, long rows, int k0, int nb,
                                                const double* __restrict__ Linv, long strip) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, kq = lane >> 4;
  const long r0 = (long)k0 + nb + strip * 64 + (wave >> 2) * 32;
  const int cg = (wave & 3) * 32;
  const double* P = M + (long)k0 * lda;
  double4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = double4_t{0, 0, 0, 0};
  const double* xp[2];
  const double* yp[2];
  bool xv[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const long xr = r0 + m * 16 + r;
    xv[m] = xr < rows;
    xp[m] = P + (xv[m] ? xr : 0) + (long)kq * lda;
    yp[m] = Linv + (cg + m * 16 + r) + (long)kq * kNB;
  }
  if (nb == kNB) {   // (rows past the end read row 0 -- xp[] is clamped -- and are dropped at the store: one straggling wave on the
                     //  two-deep path below used to set the duration of the whole launch, 22 us whatever the rest did)
    // full panel, rows inside: 16 k-steps of operands in flight at a time (a slot is reloaded with step s + 16 right after step s
    // used it).  Two steps deep, the loop waited for a global load per step: 25 us per launch whatever the panel height.
    double ra[16][2], rb[16][2];
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2)
#pragma unroll
      for (int m = 0; m < 2; ++m) { ra[s2][m] = xp[m][(long)(4 * s2) * lda]; rb[s2][m] = yp[m][(long)(4 * s2) * kNB]; }
    __builtin_amdgcn_sched_barrier(0);   // all 64 loads are issued HERE (left alone, the scheduler sinks them to three steps ahead of their use)
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int nj = 0; nj < 2; ++nj) acc[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(rb[s2][nj], ra[s2][mi], acc[mi][nj], 0, 0, 0);
        if (half == 0) {
#pragma unroll
          for (int m = 0; m < 2; ++m) { ra[s2][m] = xp[m][(long)(4 * (s2 + 16)) * lda]; rb[s2][m] = yp[m][(long)(4 * (s2 + 16)) * kNB]; }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
  } else {
  // software pipeline, two k-steps deep
  double a[2], b[2], an[2], bn[2];
  {
    const bool kv = kq < nb;
#pragma unroll
    for (int m = 0; m < 2; ++m) { a[m] = (xv[m] && kv) ? xp[m][0] : 0.0; b[m] = kv ? yp[m][0] : 0.0; }
  }
  for (int kk = 0; kk < nb; kk += 4) {
    const int kn = kk + 4;
    const bool kv = (kn + kq) < nb;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      an[m] = (xv[m] && kv) ? xp[m][(long)kn * lda] : 0.0;
      bn[m] = kv ? yp[m][(long)kn * kNB] : 0.0;
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int nj = 0; nj < 2; ++nj) acc[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[nj], a[mi], acc[mi][nj], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < 2; ++m) { a[m] = an[m]; b[m] = bn[m]; }
  }
  }
  __syncthreads();   // every wave of the workgroup has read its input rows
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        // the product is formed TRANSPOSED (Linv fragment as the MFMA A operand): D's lane & 15 is then the panel ROW, so 16 lanes
        // store 128 contiguous bytes of a column (row-major-in-lanes stores touched 64 different cache lines per instruction)
        const long row = r0 + mi * 16 + r;
        const int col = cg + nj * 16 + kq + 4 * g;
        if constexpr (WT) {
          if (nb == kNB) {   // write-through, full panel: the lane's two column blocks leave as one 16-byte store per lane pair
            if (nj == 0)
              chol_store_wt_pair(&M[row + (long)(k0 + col) * lda], &M[row + (long)(k0 + col + 16) * lda], acc[mi][0][g], acc[mi][1][g], row < rows,
                                 ((lda | (r0 + mi * 16)) & 1) == 0);
            continue;
          }
        }
        if (row < rows && col < nb) chol_store<WT>(&M[row + (long)(k0 + col) * lda], acc[mi][nj][g]);
      }
}
static __global__ __launch_bounds__(512) void k_chol_panel(double* __restrict__ M, long lda, long rows, int k0, int nb,
                                                    const double* __restrict__ Linv) {
  chol_panel_body<false>(M, lda, rows, k0, nb, Linv, (long)blockIdx.x);
}

// ---- trailing update, LDS-staged: C[base.., base..) -= P P^T with P = columns [kcol0, kcol0 + K) -------------------
// Workgroup tile 256 (rows) x 128 (cols), 8 waves as 4 x 2 sub-tiles of 64 x 64; the K dimension is streamed
// through LDS in chunks of 16 (double-buffered: global -> registers while the MFMAs of the previous chunk issue,
// registers -> LDS, one barrier per chunk).  Operand traffic per tile is (256 + 128) x K doubles instead of the
// 4 x (64 + 64) x K each wave used to pull on its own, and K itself is 256 (two 128-wide inner panels per
// trailing update), which halves the read-modify-write traffic on C per flop.
// The product is formed TRANSPOSED (B-fragment as the MFMA A operand): in the f64 D layout lane & 15 is then the
// row index of C, so 16 lanes touch 128 contiguous bytes of the column-major matrix.
// Small trailing matrices (the reduced system of a C3-sized graph, n ~ 3k) use a 128 x 64 tile (32 x 32 per wave): the
// chain of one wave is then 4 MFMAs per k-step instead of 16 and a trailing matrix of 1,500 rows still spreads over ~140
// workgroups; with the big tile it occupied 20 CUs for 86 us whatever its size.
constexpr int kKC = 16;
__device__ int g_chol_stats_on;     // ESL_CHOL_TIMING (esl_selftest_cholesky): diagnostics of the solver's kernels on
__device__ long long g_upd_clk[4];  // k_chol_update_lds, one tile of the last launch: shader clock ticks, 100 MHz ticks, K, tile rows
// One tile of C -= P P^T: rows [i0, i0 + BM) x columns [j0, j0 + BN) of M (lower triangle only), P = (rows x K) column-major with
// leading dimension ldp; `assign`: C = -P P^T (split-K slices).  WT: C leaves with write-through stores (persistent factorisation).
template <int BM, int BN, int WM, int WN, bool WT>
__device__ __forceinline__ void chol_update_tile(double* __restrict__ sm, double* __restrict__ M, long lda, long rows, long ncols,
                                                 const double* __restrict__ P, long ldp, int K, long i0, long j0, bool assign) {
  constexpr int NT = 64 * WM * WN;                // threads per workgroup
  constexpr int kLdA = BM + 16, kLdB = BN + 16;   // +16: the 4 k-groups of a fragment read land in different banks
  constexpr int SM = BM / WM, SN = BN / WN;       // rows x columns of one wave's sub-tile
  constexpr int MI = SM / 16, NJ = SN / 16;
  constexpr int QA = BM * kKC / 2 / NT, QB = BN * kKC / 2 / NT;   // double2 per thread per chunk
  static_assert(QA >= 1 && QB >= 1, "chunk smaller than the workgroup");
  double* As = sm;                               // [2][kKC][kLdA]
  double* Bs = sm + 2 * kKC * kLdA;              // [2][kKC][kLdB]
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int wi = wave / WN, wj = wave % WN;
  // global -> register staging: A chunk = BM x 16 doubles, B chunk = BN x 16 doubles, as double2
  typedef double double2_t __attribute__((ext_vector_type(2)));
  double2_t ra[QA], rb[QB];
  auto gload = [&](int kc) {
#pragma unroll
    for (int q = 0; q < QA; ++q) {
      const int e = t + NT * q, pr = e % (BM / 2), k = e / (BM / 2);
      const long row = i0 + 2 * pr;
      const bool kv = (kc + k) < K;
      // edge tiles: clamped addresses + selects, no branches (a branchy load per element made the edge workgroups the stragglers)
      const long kcl = kv ? (long)(kc + k) : (long)(K - 1);
      const double v0 = P[(row < rows ? row : rows - 1) + kcl * ldp], v1 = P[(row + 1 < rows ? row + 1 : rows - 1) + kcl * ldp];
      ra[q] = double2_t{(kv && row < rows) ? v0 : 0.0, (kv && row + 1 < rows) ? v1 : 0.0};
    }
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      const int e = t + NT * q, pr = e % (BN / 2), k = e / (BN / 2);
      const long row = j0 + 2 * pr;
      const bool kv = (kc + k) < K;
      const long kcl = kv ? (long)(kc + k) : (long)(K - 1);
      const double v0 = P[(row < rows ? row : rows - 1) + kcl * ldp], v1 = P[(row + 1 < rows ? row + 1 : rows - 1) + kcl * ldp];
      rb[q] = double2_t{(kv && row < rows) ? v0 : 0.0, (kv && row + 1 < rows) ? v1 : 0.0};
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int q = 0; q < QA; ++q) {
      const int e = t + NT * q, pr = e % (BM / 2), k = e / (BM / 2);
      *reinterpret_cast<double2_t*>(As + (buf * kKC + k) * kLdA + 2 * pr) = ra[q];
    }
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      const int e = t + NT * q, pr = e % (BN / 2), k = e / (BN / 2);
      *reinterpret_cast<double2_t*>(Bs + (buf * kKC + k) * kLdB + 2 * pr) = rb[q];
    }
  };
  double4_t acc[NJ][MI];   // acc[nj][mi]: rows = j (tile columns), cols = i (tile rows)
#pragma unroll
  for (int x = 0; x < NJ; ++x)
#pragma unroll
    for (int y = 0; y < MI; ++y) acc[x][y] = double4_t{0, 0, 0, 0};
  const bool skip = (j0 + wj * SN) > (i0 + wi * SM + SM - 1) || (i0 + wi * SM) >= rows || (j0 + wj * SN) >= ncols;  // sub-tile above the diagonal / outside
  const int r = lane & 15, kq = lane >> 4;
  // interior tiles (all rows of the tile inside the matrix, K a multiple of the chunk): the same staging without a single
  // guard -- the guarded form costs ~250 instructions and 22 branches per 64 MFMAs, in phase on all 8 waves after each barrier
  const bool interior = (i0 + BM <= rows) && (K % kKC == 0);
  const double* pA[QA];
  const double* pB[QB];
#pragma unroll
  for (int q = 0; q < QA; ++q) { const int e = t + NT * q; pA[q] = P + i0 + 2 * (e % (BM / 2)) + (long)(e / (BM / 2)) * ldp; }
#pragma unroll
  for (int q = 0; q < QB; ++q) { const int e = t + NT * q; pB[q] = P + j0 + 2 * (e % (BN / 2)) + (long)(e / (BN / 2)) * ldp; }
  auto gload_fast = [&](int kc) {
#pragma unroll
    for (int q = 0; q < QA; ++q) ra[q] = *reinterpret_cast<const double2_t*>(pA[q] + (long)kc * ldp);
#pragma unroll
    for (int q = 0; q < QB; ++q) rb[q] = *reinterpret_cast<const double2_t*>(pB[q] + (long)kc * ldp);
  };
  // Round 6, persistent kernel only: the C tile's lines are requested (one dword per line and lane group, into a register nobody
  // reads) under the LAST chunk's MFMAs.  The tile was written write-through by whichever CU visited it last, usually on another
  // XCD: the epilogue's NJ dependent load groups each paid a fabric round trip (~2 us) in a task visited 216 times per worker at
  // n = 18,000.  The loads are older than the epilogue's, and loads complete in order, so the dummy register is dead by the time the
  // first real C value arrives (it is kept allocated until then).
  int c_dummy = 0;
  auto c_prefetch = [&]() {
    const long iw0 = i0 + wi * SM, jw0 = j0 + wj * SN;
    const bool full_sub = !assign && (iw0 + SM <= rows) && (jw0 + SN <= ncols) && (jw0 + SN - 1 <= iw0);
    if (full_sub) {
      // ONE pointer walks the sub-tile's column groups (column jw0 + kq + 4 c, c = 0 .. 4 NJ - 1), the MI row groups are immediate
      // offsets: 64 separately formed addresses took the merged kernel's scratch from 144 to 656 B
      const double* pc = &M[(iw0 + r) + (jw0 + kq) * lda];
#pragma unroll 1
      for (int c2 = 0; c2 < 4 * NJ; ++c2) {
        if constexpr (MI == 4)
          asm volatile("global_load_dword %0, %1, off\n\tglobal_load_dword %0, %1, off offset:128\n\tglobal_load_dword %0, %1, off offset:256\n\t"
                       "global_load_dword %0, %1, off offset:384" : "+v"(c_dummy) : "v"(pc) : "memory");
        else if constexpr (MI == 2)
          asm volatile("global_load_dword %0, %1, off\n\tglobal_load_dword %0, %1, off offset:128" : "+v"(c_dummy) : "v"(pc) : "memory");
        pc += 4 * lda;
      }
    }
  };
  auto mainloop = [&](auto fast) {
    if constexpr (decltype(fast)::value) gload_fast(0); else gload(0);
    sstore(0);
    __syncthreads();
    int buf = 0;
    for (int kc = 0; kc < K; kc += kKC) {
      const bool more = kc + kKC < K;
      if (more) { if constexpr (decltype(fast)::value) gload_fast(kc + kKC); else gload(kc + kKC); }
      else if constexpr (WT) c_prefetch();   // (the last chunk has no operands to fetch: its MFMAs cover the C tile's way into this XCD's L2)
      if (!skip) {
        const double* Ab = As + buf * kKC * kLdA + wi * SM + r;
        const double* Bb = Bs + buf * kKC * kLdB + wj * SN + r;
#pragma unroll
        for (int kk = 0; kk < kKC; kk += 4) {
          double a[MI], bq[NJ];
#pragma unroll
          for (int m = 0; m < MI; ++m) a[m] = Ab[(kk + kq) * kLdA + m * 16];
#pragma unroll
          for (int m = 0; m < NJ; ++m) bq[m] = Bb[(kk + kq) * kLdB + m * 16];
#pragma unroll
          for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) acc[nj][mi] = __builtin_amdgcn_mfma_f64_16x16x4f64(bq[nj], a[mi], acc[nj][mi], 0, 0, 0);
        }
      }
      if (more) sstore(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  };
  if (interior) mainloop(std::true_type{}); else mainloop(std::false_type{});
  if (skip) return;
  const long iw = i0 + wi * SM, jw = j0 + wj * SN;
  const int rq = lane >> 4;
  // C -= acc.  Sub-tiles that lie entirely inside the matrix and strictly below the diagonal (all but a sliver) take the
  // unguarded form: 4 MI independent loads in flight per column group, then the subtracts and stores.  The guarded form
  // compiled to load / wait / subtract / store one element at a time -- 64 exposed memory round trips per lane, which
  // cost more than the whole K loop of the tile.
  const bool full = (iw + SM <= rows) && (jw + SN <= ncols) && (jw + SN - 1 <= iw);
  if (full) {
    // Round 6: the loads of column group nj + 1 are issued BEFORE the stores of group nj (two register sets).  Written as "load 16,
    // store 16" per group the compiler keeps every group's loads behind the previous group's stores (same array), i.e. NJ exposed
    // round trips to a tile another CU wrote last -- ~2 us each, in a task that is visited 216 times per worker at n = 18,000.
    // Launch-path kernels only (n = 32,768: 215.9 -> 213.6 ms): the persistent kernel owns all 256 registers of its two waves per SIMD
    // and the second register set went to scratch there (128 -> 224 B, task bodies 33.6 -> 34.3 ms) -- it keeps the one-set form.
    if constexpr (WT && NJ == 2 && MI == 2) {
      // the persistent kernel's quarter tiles (32 x 32 per wave): both column groups' C values first, then the lane's two columns of a
      // row leave with its neighbour's as 16-byte write-through stores (chol_store_wt_pair)
      double c2[2][MI][4];
#pragma unroll
      for (int nj = 0; nj < 2; ++nj)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int g = 0; g < 4; ++g) c2[nj][mi][g] = assign ? 0.0 : M[(iw + mi * 16 + r) + (jw + nj * 16 + rq + 4 * g) * lda];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          chol_store_wt_pair(&M[(iw + mi * 16 + r) + (jw + rq + 4 * g) * lda], &M[(iw + mi * 16 + r) + (jw + 16 + rq + 4 * g) * lda], c2[0][mi][g] - acc[0][mi][g],
                             c2[1][mi][g] - acc[1][mi][g], true, ((lda | iw) & 1) == 0);
      asm volatile("" :: "v"(c_dummy));
      return;
    }
    constexpr int NSET = WT ? 1 : 2;
    double cv[NSET][MI][4];
    auto load_group = [&](int nj, double (&dst)[MI][4]) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int g = 0; g < 4; ++g) dst[mi][g] = assign ? 0.0 : M[(iw + mi * 16 + r) + (jw + nj * 16 + rq + 4 * g) * lda];
    };
    if constexpr (NSET == 2) load_group(0, cv[0]);
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
      if constexpr (NSET == 2) { if (nj + 1 < NJ) load_group(nj + 1, cv[(nj + 1) & 1]); }
      else load_group(nj, cv[0]);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int g = 0; g < 4; ++g) chol_store<WT>(&M[(iw + mi * 16 + r) + (jw + nj * 16 + rq + 4 * g) * lda], cv[nj & (NSET - 1)][mi][g] - acc[nj][mi][g]);
      if (nj == 0) asm volatile("" :: "v"(c_dummy));   // (the prefetch's destination register: allocated until the first real C values are in)
    }
    return;
  }
  // edge and diagonal sub-tiles: the same batching with clamped addresses and predicated stores (an `if` around the whole
  // read-modify-write compiles to one exposed memory round trip per element, and the workgroup doing that is the last to finish)
#pragma unroll
  for (int nj = 0; nj < NJ; ++nj) {
    double cv[MI][4];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const long col = jw + nj * 16 + rq + 4 * g;   // D row  -> j
        const long row = iw + mi * 16 + r;            // D col  -> i (contiguous across lanes)
        cv[mi][g] = assign ? 0.0 : M[(row < rows ? row : rows - 1) + (col < ncols ? col : ncols - 1) * lda];
      }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const long col = jw + nj * 16 + rq + 4 * g;
        const long row = iw + mi * 16 + r;
        if (row < rows && col < ncols && row >= col) chol_store<WT>(&M[row + col * lda], cv[mi][g] - acc[nj][mi][g]);
      }
  }
}

template <int BM, int BN, int WM = 4, int WN = 2>
static __global__ __launch_bounds__(64 * WM * WN, 2) void k_chol_update_lds(double* __restrict__ M, long lda, long rows, long ncols,
                                                                           int kcol0, int K, long base, int ntJ, int rect,
                                                                           const double* __restrict__ Pext, long ldp,
                                                                           double* __restrict__ part, int kper,
                                                                           const int* __restrict__ kfirst = nullptr) {
  static_assert((BM == 2 * BN || BM == BN) && BM % 64 == 0, "tile shape");
  constexpr int RT = BM / BN;                     // tile row ti of the lower triangle holds RT (ti + 1) tiles
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const long b = blockIdx.x;
  long ti, tj;
  if (rect) {                                    // a few tile columns of a tall region: ntJ tiles per tile row
    ti = b / ntJ; tj = b - ti * ntJ;
    if (tj > RT * ti + RT - 1) return;           // above the diagonal
  } else {                                       // the whole lower triangle: rows 0 .. ti-1 hold RT ti (ti + 1) / 2 tiles
    ti = (long)((sqrt(1.0 + 8.0 * (double)b / RT) - 1.0) * 0.5);
    while (RT * ti * (ti + 1) / 2 > b) --ti;
    while (RT * (ti + 1) * (ti + 2) / 2 <= b) ++ti;
    tj = b - RT * ti * (ti + 1) / 2;             // 0 .. RT (ti + 1) - 1
    if (tj >= ntJ) return;
  }
  const long i0 = base + ti * BM, j0 = base + tj * BN;
  if (i0 >= rows || j0 >= ncols) return;
  // the rank-K factor: columns [kcol0, kcol0 + K) of M itself (Cholesky trailing update), or an external (rows x K) column-major
  // matrix Pext with leading dimension ldp (C -= Pext Pext^T: the reduced ellipsoid system of the camera-first elimination, esl_cf.hpp)
  const double* P = Pext ? Pext : M + (long)kcol0 * lda;
  if (!Pext) ldp = lda;
  // split-K (gridDim.y > 1; small outputs with a long K: a 450 x 450 system has 20 tiles): slice blockIdx.y takes K range
  // [y kper, (y + 1) kper) and writes -acc into ITS copy of the output (part + y lda ncols; no read-modify-write); a reduction
  // kernel adds the slices to C in slice order -- deterministic, unlike atomics
  if (part) {
    const int kbeg = (int)blockIdx.y * kper;
    P += (long)kbeg * ldp;
    K = (K - kbeg < kper) ? K - kbeg : kper;
    M = part + (size_t)blockIdx.y * (size_t)lda * (size_t)ncols;
    if (K <= 0) return;
  }
  // kfirst (external factor only, round 5): kfirst[g] = the first row of Pext that can be non-zero in any of the columns
  // [64 g, 64 g + 64) -- esl_cf.hpp orders T's ellipsoids by first camera, so the separators' rows of X are structurally zero above a
  // staircase.  A product term (row r, column c) needs both factors non-zero: the tile starts at the later of its two earliest
  // rows, rounded down to a chunk.  Only exact zeros are skipped: the result has the same bits.
  if (kfirst) {
    int ka = K, kb = K;
    for (long g = i0 / 64; g < (i0 + BM) / 64; ++g) ka = kfirst[g] < ka ? kfirst[g] : ka;
    for (long g = j0 / 64; g < (j0 + BN) / 64; ++g) kb = kfirst[g] < kb ? kfirst[g] : kb;
    int ks = ka > kb ? ka : kb;
    ks = (ks < K ? ks : K) & ~(kKC - 1);
    P += (long)ks * ldp;
    K -= ks;
    if (K <= 0) return;
  }
  // (diagnostic, ESL_CHOL_TIMING: shader clock ticks against 100 MHz wall-clock ticks over one tile of the last launch -- is the
  //  K loop's distance from the MFMA peak a matter of the clock the part sustains under this load?)
  const bool clk_on = BM == 256 && K >= 512 && gridDim.x >= 2048 && g_chol_stats_on != 0 && blockIdx.x == gridDim.x / 2 && threadIdx.x == 0;   // (a tile in the middle of a launch that fills the chip)
  long long c0 = 0, w0 = 0;
  if (clk_on) { c0 = (long long)clock64(); w0 = (long long)wall_clock64(); }
  chol_update_tile<BM, BN, WM, WN, false>(sm, M, lda, rows, ncols, P, ldp, K, i0, j0, part != nullptr);
  if (clk_on) { g_upd_clk[0] = (long long)clock64() - c0; g_upd_clk[1] = (long long)wall_clock64() - w0; g_upd_clk[2] = K; g_upd_clk[3] = BM; }
}
// dynamic LDS of the two k_chol_update_lds shapes, and the most K slices of a split-K launch (chol_launch_update, esl_chol.hpp)
constexpr size_t kCholLdsBig = (size_t)(2 * kKC * (256 + 16 + 128 + 16)) * sizeof(double);
constexpr size_t kCholLdsSmall = (size_t)(2 * kKC * (128 + 16 + 64 + 16)) * sizeof(double);
constexpr int kCholMaxSplit = 16;

// ---- round 6: the update tile in the shape the part's own DGEMM library runs (scripts/debug/rocblas_dgemm_probe.py) ------------------
// The vendor DGEMM reaches 89 - 96 % of the FP64-MFMA peak at these sizes where the 256 x 128 tile above reaches 79 %.  Its kernels
// (the dispatched symbols name the shape: MT128x128x16, four waves of 32 x 128, one operand "direct to VGPR") differ in two ways that
// matter here: (1) a workgroup is FOUR waves, one per SIMD, and TWO workgroups share a CU -- when one of them sits in its barrier the
// other one's wave on the same SIMD owns the matrix core, where the eight waves of the big tile all wait together; (2) the operand
// no other wave needs (this wave's 32 rows) never touches LDS: every lane loads its own MFMA fragment from global memory (a lane's
// fragment of the f64 16x16x4 MFMA is ONE element: row r = lane & 15, k = lane >> 4), only the 128-column operand the four waves share
// is staged.  Half the LDS stores and half the LDS fragment reads per MFMA.
// Tile: rows [i0, i0 + 128) x columns [j0, j0 + 128); wave w owns rows i0 + 32 w .. + 31, interleaved in pairs -- lane r holds rows
// 2 r and 2 r + 1 (one 16-byte load per k-step, and the C tile's read-modify-write is 16-byte accesses too).  Same product
// orientation as above (D rows = tile columns, D columns = tile rows), the same k order inside and across MFMAs: the same bits.
constexpr int kVT = 128, kVLd = kVT + 16;
// a value every lane holds alike, as the compiler cannot know (it came through LDS or a vector load): into scalar registers
__device__ __forceinline__ int chol_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long chol_uniform(long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v & 0xffffffffL)), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long)v >> 32));
  return (long)(((unsigned long)hi << 32) | lo);
}
constexpr size_t kCholLdsV = (size_t)(2 * kKC * kVLd) * sizeof(double);
// HV = 1 (the persistent factorisation, one 512-thread workgroup per CU): the workgroup's two halves -- waves 0-3 and 4-7, one wave per
// SIMD each (measured: the eight waves of a workgroup sit on SIMDs 3 0 2 1 3 0 2 1) -- run this function side by side on the upper and
// the lower 128 rows of a 256 x 128 tile, each with its own LDS buffers and its own barrier: a counter in LDS (`bar`, zeroed by the
// caller behind a workgroup barrier) that the four waves of a half bump and poll.  The piecewise probe (scripts/debug/tile_probe_v.hip):
// 86.4 % of the FP64-MFMA peak for the eight-wave 256 x 128 loop, 92.3 % for two four-wave workgroups, 89.7 % for two halves of one
// workgroup behind the LDS-counter barrier.
template <bool WT, int HV = 0>
__device__ __forceinline__ void chol_update_tile_v(double* __restrict__ sm, double* __restrict__ M, long lda, long rows, long ncols,
                                                   const double* __restrict__ P, long ldp, int K, long i0, long j0, bool assign, int* bar = nullptr) {
  typedef double double2_t __attribute__((ext_vector_type(2)));
  constexpr int NT = 256, NJ = kVT / 16, QB = kVT * kKC / 2 / NT;   // 8 column blocks; 4 double2 of the shared operand per thread and chunk
  const int t = HV ? (int)(threadIdx.x & 255) : (int)threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 15, kq = lane >> 4;
  const long iw = i0 + wave * 32;
  // The unguarded loop only needs the tile's 128 rows of P to be READABLE: rows [rows, ldp) of a column-major array are padding inside
  // the allocation, and what they hold cannot matter -- row r of either operand only enters row / column r of the product, and rows and
  // columns >= `rows` of C are never stored.  With a leading dimension that is a multiple of 128 (esl_slam.hip pads its own) the
  // LAST tile row takes the unguarded loop like every other: as the guarded form it ran 2 - 3 x longer, 141 tiles of it at the very
  // end of the launch -- a fixed ~2 ms on the rank-3,744 update.
  const bool interior = (i0 + kVT <= ldp) && (K % (2 * kKC) == 0);
  const bool skipw = (j0 > iw + 31) || iw >= rows;   // this wave's rows lie above the diagonal / under the matrix: staging and barriers only
  int phase = 0;
  auto sync = [&]() {
    if constexpr (HV == 0) __syncthreads();
    else {
      phase += 4;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_fetch_add(bar, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < phase) __builtin_amdgcn_s_sleep(0);
      asm volatile("" ::: "memory");
    }
  };
  // the shared operand: thread t stages rows j0 + 2 (e % 64), k = e / 64 (e = t + 256 q), i.e. k = t / 64 + 4 q; this lane's own
  // fragments: rows iw + 2 r, iw + 2 r + 1 at k = kc + 4 s + kq.  Addresses = a wave-uniform base (scalar registers) + ONE 32-bit
  // per-lane byte offset each (eight 64-bit pointers per lane went to scratch in the persistent kernel)
  const char* PBu = reinterpret_cast<const char*>(P + j0);
  const char* PAu = reinterpret_cast<const char*>(P + i0);
  const unsigned offB = (unsigned)((2 * (t % (kVT / 2)) + (long)(t / (kVT / 2)) * ldp) * (long)sizeof(double));
  const unsigned offA = (unsigned)((wave * 32 + 2 * r + (long)kq * ldp) * (long)sizeof(double));
  double2_t rb[QB];
  auto gload_b = [&](int kc, auto fast) {
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      if constexpr (decltype(fast)::value) rb[q] = *reinterpret_cast<const double2_t*>(PBu + (long)(kc + 4 * q) * ldp * (long)sizeof(double) + offB);
      else {
        const int e = t + NT * q, k = e / (kVT / 2);
        const long row = j0 + 2 * (e % (kVT / 2));
        const bool kv = (kc + k) < K;
        const long kcl = kv ? (long)(kc + k) : (long)(K - 1);
        const double v0 = P[(row < rows ? row : rows - 1) + kcl * ldp], v1 = P[(row + 1 < rows ? row + 1 : rows - 1) + kcl * ldp];
        rb[q] = double2_t{(kv && row < rows) ? v0 : 0.0, (kv && row + 1 < rows) ? v1 : 0.0};
      }
    }
  };
  auto gload_a = [&](double2_t (&a)[4], int kc, auto fast) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if constexpr (decltype(fast)::value) a[s] = *reinterpret_cast<const double2_t*>(PAu + (long)(kc + 4 * s) * ldp * (long)sizeof(double) + offA);
      else {
        const long row = iw + 2 * r;
        const int k = kc + 4 * s + kq;
        const bool kv = k < K;
        const long kcl = kv ? (long)k : (long)(K - 1);
        const double v0 = P[(row < rows ? row : rows - 1) + kcl * ldp], v1 = P[(row + 1 < rows ? row + 1 : rows - 1) + kcl * ldp];
        a[s] = double2_t{(kv && row < rows) ? v0 : 0.0, (kv && row + 1 < rows) ? v1 : 0.0};
      }
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      const int e = t + NT * q;
      *reinterpret_cast<double2_t*>(sm + (buf * kKC + e / (kVT / 2)) * kVLd + 2 * (e % (kVT / 2))) = rb[q];
    }
  };
  double4_t acc[NJ][2];
#pragma unroll
  for (int x = 0; x < NJ; ++x) { acc[x][0] = double4_t{0, 0, 0, 0}; acc[x][1] = double4_t{0, 0, 0, 0}; }
  const bool full = !skipw && (iw + 32 <= rows) && (j0 + kVT <= ncols) && (j0 + kVT - 1 <= iw) && ((lda & 1) == 0) && (((iw & 1) == 0));
  // persistent kernel: the C sub-tile's lines requested under the LAST chunk's MFMAs (see chol_update_tile: the tile was written
  // write-through by another CU, usually on another XCD; one dword per 128-byte line and lane group into a register nobody reads)
  int c_dummy = 0;
  auto c_prefetch = [&]() {
    if (full && !assign) {
      const double* pc = &M[(iw + 2 * r) + (j0 + kq) * lda];
#pragma unroll 1
      for (int c2 = 0; c2 < 4 * NJ; ++c2) {
        asm volatile("global_load_dword %0, %1, off" : "+v"(c_dummy) : "v"(pc) : "memory");
        pc += 4 * lda;
      }
    }
  };
  // one chunk: MFMAs on a_cur and LDS buffer `buf`; the operands of chunk `kn` (the next one; the last chunk names itself) are
  // requested first and the shared one goes into the other LDS buffer behind the MFMAs.  No branch around the loads or the stores:
  // with `if (more)` the compiler's wait-count pass joins the two paths at the first MFMA and waits for the loads it has just issued
  // (vmcnt(3) with twelve in flight: one exposed memory round trip per chunk).
  auto chunk = [&](double2_t (&a_cur)[4], double2_t (&a_nxt)[4], int kn, int buf, auto fast) {
    gload_b(kn, fast);
    gload_a(a_nxt, kn, fast);
    if (!skipw) {
      const double* Bb = sm + buf * kKC * kVLd + r;
      double bq[2][NJ];
#pragma unroll
      for (int m = 0; m < NJ; ++m) bq[0][m] = Bb[kq * kVLd + m * 16];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (s + 1 < 4) {
#pragma unroll
          for (int m = 0; m < NJ; ++m) bq[(s + 1) & 1][m] = Bb[(4 * (s + 1) + kq) * kVLd + m * 16];
        }
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) {
          acc[nj][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(bq[s & 1][nj], a_cur[s].x, acc[nj][0], 0, 0, 0);
          acc[nj][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(bq[s & 1][nj], a_cur[s].y, acc[nj][1], 0, 0, 0);
        }
      }
    }
    // (the stores stay behind the MFMAs: hoisted to the middle of the chunk, as the scheduler likes to, they wait for loads that are
    //  half a chunk old -- 19.1 vs 18.7 ms on the rank-3,744 update)
    __builtin_amdgcn_sched_barrier(0);
    sstore(buf ^ 1);
    sync();
  };
  auto mainloop = [&](auto fast) {
    double2_t a0[4], a1[4];
    gload_b(0, fast); gload_a(a0, 0, fast);
    sstore(0);
    sync();
    if constexpr (decltype(fast)::value) {
      // an even number of whole chunks: ONE copy of the chunk pair (separate copies for the last chunks cost the persistent kernel
      // 80 scratch stores + 35 reloads per visit around them); the last chunk fetches nothing new -- its own operands again
      for (int kc = 0; kc < K; kc += 2 * kKC) {
        const bool last = kc + 2 * kKC >= K;
        if constexpr (WT) { if (last) c_prefetch(); }
        chunk(a0, a1, kc + kKC, 0, fast);
        chunk(a1, a0, last ? kc + kKC : kc + 2 * kKC, 1, fast);
      }
    } else {
      const int klast = ((K + kKC - 1) / kKC - 1) * kKC;   // first k of the last chunk
      int kc = 0;
      for (; kc + kKC <= klast; kc += 2 * kKC) {
        chunk(a0, a1, kc + kKC, 0, fast);
        chunk(a1, a0, kc + 2 * kKC <= klast ? kc + 2 * kKC : klast, 1, fast);
      }
      if (kc <= klast) chunk(a0, a1, klast, 0, fast);   // (an odd number of chunks)
    }
  };
  if (interior) mainloop(std::true_type{}); else mainloop(std::false_type{});
  if (skipw || j0 >= ncols) return;
  // C -= acc: acc[nj][mi][g] is row iw + 2 r + mi, column j0 + 16 nj + kq + 4 g
  if (full) {
    double2_t cv[2][4];
    auto load_group = [&](int nj, double2_t (&dst)[4]) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        dst[g] = assign ? double2_t{0.0, 0.0} : *reinterpret_cast<const double2_t*>(&M[(iw + 2 * r) + (j0 + nj * 16 + kq + 4 * g) * lda]);
    };
    load_group(0, cv[0]);
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
      if (nj + 1 < NJ) load_group(nj + 1, cv[(nj + 1) & 1]);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        double* p = &M[(iw + 2 * r) + (j0 + nj * 16 + kq + 4 * g) * lda];
        const double2_t v = double2_t{cv[nj & 1][g].x - acc[nj][0][g], cv[nj & 1][g].y - acc[nj][1][g]};
        // write-through as ONE 16-byte sc1 store: 8-byte sc1 stores cost 2.7 x per byte (the guide's store table; n = 18,000 37.25 ->
        // 36.37 ms, 24,000 80.7 -> 79.4 against two 8-byte atomic stores).  Inline assembly, so the compiler sees neither the store's
        // place in the vmcnt queue nor its hazard: a VALU write to the data registers of a store wider than 8 bytes needs wait states
        // behind it (the hazard recognizer pads its own stores; without the s_nop the next address computation landed in the stored data)
        if constexpr (WT) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
        else *reinterpret_cast<double2_t*>(p) = v;
      }
      if (nj == 0) asm volatile("" :: "v"(c_dummy));   // (the prefetch's destination register: allocated until the first real C values are in)
    }
    return;
  }
#pragma unroll
  for (int nj = 0; nj < NJ; ++nj) {
    double cv[2][4];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const long col = j0 + nj * 16 + kq + 4 * g, row = iw + 2 * r + mi;
        cv[mi][g] = assign ? 0.0 : M[(row < rows ? row : rows - 1) + (col < ncols ? col : ncols - 1) * lda];
      }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const long col = j0 + nj * 16 + kq + 4 * g, row = iw + 2 * r + mi;
        if (row < rows && col < ncols && row >= col) chol_store<WT>(&M[row + col * lda], cv[mi][g] - acc[nj][mi][g]);
      }
  }
}
// the launch: same arguments and tile enumeration as k_chol_update_lds<128, 128> (square tiles: tile row ti holds ti + 1 tiles)
// Tile order: row-major over the triangle.  (Workgroups are dealt to the eight XCDs round-robin, each with an L2 of its own; ids dealt so
// that an XCD works on an 8 x 8 block of tiles took a quarter of the L2 misses away and changed nothing, 18.9 vs 19.1 ms: retired)
__host__ __device__ inline long chol_v_grid(long ntI) { return ntI * (ntI + 1) / 2; }
static __global__ __launch_bounds__(256, 2) void k_chol_update_v(double* __restrict__ M, long lda, long rows, long ncols, int kcol0, int K, long base, int ntJ,
                                                                 int rect, const double* __restrict__ Pext, long ldp,
                                                                 const int* __restrict__ kfirst = nullptr, int assign = 0) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const long b = blockIdx.x;
  long ti, tj;
  if (rect) {
    ti = b / ntJ; tj = b - ti * ntJ;
    if (tj > ti) return;
  } else {
    ti = (long)((sqrt(1.0 + 8.0 * (double)b) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > b) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= b) ++ti;
    tj = b - ti * (ti + 1) / 2;
    if (tj >= ntJ) return;
  }
  const long i0 = base + ti * kVT, j0 = base + tj * kVT;
  if (i0 >= rows || j0 >= ncols) return;
  const double* P = Pext ? Pext : M + (long)kcol0 * lda;
  if (!Pext) ldp = lda;
  if (kfirst) {   // (the staircase of esl_cf.hpp, as in k_chol_update_lds)
    int ka = K, kb = K;
    for (long g = i0 / 64; g < (i0 + kVT) / 64; ++g) ka = kfirst[g] < ka ? kfirst[g] : ka;
    for (long g = j0 / 64; g < (j0 + kVT) / 64; ++g) kb = kfirst[g] < kb ? kfirst[g] : kb;
    int ks = ka > kb ? ka : kb;
    ks = (ks < K ? ks : K) & ~(kKC - 1);
    if (((K - ks) & kKC) != 0 && ks >= kKC) ks -= kKC;   // (the tile's unguarded loop takes chunks in pairs: an odd count sent half the tiles down the guarded path)
    P += (long)ks * ldp;
    K -= ks;
    if (K <= 0) {
      if (assign)   // C = -P P^T: a tile the staircase skips altogether still has to leave zeros
        for (int e = threadIdx.x; e < kVT * kVT; e += 256) {
          const long row = i0 + e % kVT, col = j0 + e / kVT;
          if (row < rows && col < ncols && row >= col) M[row + col * lda] = 0.0;
        }
      return;
    }
  }
  chol_update_tile_v<false>(sm, M, lda, rows, ncols, P, ldp, K, i0, j0, assign != 0);
}

// ---- small systems: factor + both substitutions in ONE workgroup, the whole lower triangle in registers (round 6) ---------------
// An order-180 system (20 ellipsoids: BASELINE configs[4] in SLAM mode) is two diagonal blocks of the blocked path: 2 x potrf2 + 2 panel
// solves + 1 update + the back-substitution = 6 dependent launches, ~170 us, with fewer than 1e7 flops in them.  Here 1024 threads own
// the 4 x 4 blocks of the lower triangle (and of the right-hand side's row, a block row of its own under the padded matrix) for the
// whole solve -- up to two blocks per thread, enumerated column by column, so n <= 248 -- and run the rank-4 steps of k_chol_potrf2
// over ALL block columns: (a) the diagonal block's owner factors it and publishes the inverse of its factor, (b) the blocks under it
// become X = A L_JJ^-T and publish their four columns, (c) every block to the right subtracts its rank-4 product.  y = L^-1 b rides
// along as the last block row.  L^T x = y runs on the same registers, block row by block row from the last: the diagonal owner forms
// x_J = L_JJ^-T z_J, the blocks (J, j < J) subtract L(J, j)^T x_J from z_j (one writer per entry and step: no atomics, fixed order).
// Only x leaves the kernel (nobody reads the factor of these systems afterwards; the panels' inverses are not formed at all).
constexpr int kCsThreads = 1024, kCsKB = 2, kCsMaxRows = 256;
__host__ __device__ inline int chol_small_blocks(int n) { const int nbc = (n + 3) / 4; return nbc * (nbc + 1) / 2 + nbc; }
inline bool chol_small_fits(int n) { return n >= 1 && chol_small_blocks(n) <= kCsThreads * kCsKB && 4 * ((n + 3) / 4 + 1) <= kCsMaxRows; }
static __global__ __launch_bounds__(kCsThreads) void k_chol_small(const double* __restrict__ M, long lda, int n, double* __restrict__ x,
                                                                  int* __restrict__ info) {
  __shared__ double colbuf[4 * kCsMaxRows];   // [k][4 bi + r]: the four columns of the current block column
  __shared__ double dblk[12];                 // inverse of the current diagonal block's factor, packed rows
  __shared__ double zs[kCsMaxRows];           // back-substitution: what is left of y
  __shared__ double xs[4];
  const int t = threadIdx.x;
  const int NBC = (n + 3) / 4, NBR = NBC + 1, total = chol_small_blocks(n);
  int bi[kCsKB], bj[kCsKB];
  bool own[kCsKB];
  double a[kCsKB][4][4];
#pragma unroll
  for (int q = 0; q < kCsKB; ++q) {
    const int idx = t + q * kCsThreads;
    own[q] = idx < total;
    int off = 0, c = 0;
    if (own[q]) while (off + (NBR - c) <= idx) { off += NBR - c; ++c; }
    bj[q] = c; bi[q] = own[q] ? c + (idx - off) : 0;
    const bool rhs = bi[q] == NBC;              // the right-hand side's row: local row 0 of the last block row
#pragma unroll
    for (int c2 = 0; c2 < 4; ++c2)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * bi[q] + r, j = 4 * bj[q] + c2;
        const bool valid = own[q] && j < n && (rhs ? r == 0 : (i < n && i >= j));
        const long row = rhs ? (long)n : (long)i;
        const double v = valid ? M[row + (long)j * lda] : 0.0;
        a[q][r][c2] = valid ? v : ((!rhs && i == j) ? 1.0 : 0.0);   // identity padding behind the matrix
      }
  }
  // 4 x 4 Cholesky of block q (lower, in place); the block is REPLACED by the inverse of its factor (all that is needed afterwards)
  auto factor_diag = [&](double (&b)[4][4]) {
    double is[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double d = b[c][c];
#pragma unroll
      for (int k = 0; k < c; ++k) d -= b[c][k] * b[c][k];
      if (!(d > 0)) atomicOr(info, 1);
      double rq = __builtin_amdgcn_rsq(d);
      rq = rq * (1.5 - 0.5 * d * rq * rq);
      rq = rq * (1.5 - 0.5 * d * rq * rq);
      is[c] = rq;
      b[c][c] = d * rq;
#pragma unroll
      for (int rr = c + 1; rr < 4; ++rr) {
        double v = b[rr][c];
#pragma unroll
        for (int k = 0; k < c; ++k) v -= b[rr][k] * b[c][k];
        b[rr][c] = v * rq;
      }
    }
    double xi[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      xi[c][c] = is[c];
#pragma unroll
      for (int rr = c + 1; rr < 4; ++rr) {
        double v = 0;
#pragma unroll
        for (int k = c; k < rr; ++k) v += b[rr][k] * xi[k][c];
        xi[rr][c] = -v * is[rr];
      }
    }
    int p = 0;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        b[rr][c] = c <= rr ? xi[rr][c] : 0.0;
        if (c <= rr) dblk[p++] = xi[rr][c];
      }
  };
  if (t == 0) factor_diag(a[0]);   // block (0, 0) is thread 0's first
  __syncthreads();
  for (int J = 0; J < NBC; ++J) {
#pragma unroll
    for (int q = 0; q < kCsKB; ++q)
      if (own[q] && bj[q] == J && bi[q] > J) {   // (b) X = A L_JJ^-T
        double li[10];
#pragma unroll
        for (int p = 0; p < 10; ++p) li[p] = dblk[p];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double a0 = a[q][r][0], a1 = a[q][r][1], a2 = a[q][r][2], a3 = a[q][r][3];
          a[q][r][0] = a0 * li[0];
          a[q][r][1] = a0 * li[1] + a1 * li[2];
          a[q][r][2] = a0 * li[3] + a1 * li[4] + a2 * li[5];
          a[q][r][3] = a0 * li[6] + a1 * li[7] + a2 * li[8] + a3 * li[9];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) colbuf[c * kCsMaxRows + 4 * bi[q] + r] = a[q][r][c];
      }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kCsKB; ++q)
      if (own[q] && bj[q] > J) {                 // (c) rank-4 update
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          double rv[4], cv[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) { rv[r] = colbuf[k * kCsMaxRows + 4 * bi[q] + r]; cv[r] = colbuf[k * kCsMaxRows + 4 * bj[q] + r]; }
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) a[q][r][c] -= rv[r] * cv[c];
        }
        if (bi[q] == bj[q] && bj[q] == J + 1) factor_diag(a[q]);   // (a) of the next step
      }
    __syncthreads();
  }
  // ---- L^T x = y.  zs <- y (local row 0 of the last block row); diagonal blocks hold the inverses of their factors
#pragma unroll
  for (int q = 0; q < kCsKB; ++q)
    if (own[q] && bi[q] == NBC) {
#pragma unroll
      for (int c = 0; c < 4; ++c) zs[4 * bj[q] + c] = a[q][0][c];
    }
  __syncthreads();
  for (int J = NBC - 1; J >= 0; --J) {
#pragma unroll
    for (int q = 0; q < kCsKB; ++q)
      if (own[q] && bi[q] == J && bj[q] == J) {   // x_J = L_JJ^-T z_J
        double z[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) z[r] = zs[4 * J + r];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double v = 0;
#pragma unroll
          for (int r = c; r < 4; ++r) v += a[q][r][c] * z[r];
          xs[c] = v;
          if (4 * J + c < n) x[4 * J + c] = v;
        }
      }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kCsKB; ++q)
      if (own[q] && bi[q] == J && bj[q] < J) {    // z_j -= L(J, j)^T x_J
        double xv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) xv[r] = xs[r];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double v = zs[4 * bj[q] + c];
#pragma unroll
          for (int r = 0; r < 4; ++r) v -= a[q][r][c] * xv[r];
          zs[4 * bj[q] + c] = v;
        }
      }
    __syncthreads();
  }
}

// ---- backward substitution L^T x = y, panel by panel from the last ------------------------------------------
// z[c] = y[k0+c] - sum_{i >= k0+nb}^{n-1} L[i][k0+c] x[i]   (one workgroup per column: contiguous dot product)
static __global__ __launch_bounds__(256) void k_chol_backdot(const double* __restrict__ M, long lda, int n, int k0, int nb,
                                                      const double* __restrict__ x, double* __restrict__ z) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  if (c >= nb) return;
  const double* col = M + (long)(k0 + c) * lda;
  double s = 0;
  for (long i = (long)k0 + nb + threadIdx.x; i < n; i += 256) s += col[i] * x[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) z[c] = col[n] - red[0];  // row n holds y^T
}
// x[k0 + r] = sum_c Linv[c][r] z[c]  (Linv^T z): one wave per r, lanes over c (contiguous in memory)
static __global__ __launch_bounds__(256) void k_chol_backsolve(const double* __restrict__ Linv, int k0, int nb,
                                                        const double* __restrict__ z, double* __restrict__ x) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= nb) return;
  double s = 0;
  for (int c = lane; c < nb; c += 64) s += Linv[c + r * kNB] * z[c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) x[k0 + r] = s;
}

// ---- backward substitution L^T x = y in ONE launch (round 4) ---------------------------------------------------------------
// The launch-per-panel form above is 2 x ceil(n / 128) dependent launches whose kernels are each a few microseconds of work
// (n = 18,000: 282 launches, ~6 ms of a 46 ms solve).  Here a workgroup owns one panel p at a time (claimed from a counter, see below); it streams
// the blocks L[panel r, panel p] for r = np - 1 .. p + 1 in the order the x_r appear, keeps per-lane partial sums of
// z_p = y_p - sum_r L_rp^T x_r in registers (ONE cross-lane reduction at the end, fixed order => bit-reproducible), then
// x_p = Linv_p^T z_p from an LDS copy of Linv_p staged at the start, and publishes x_p.  Block r - 1 is fetched before the
// flag of x_{r-1} is polled, so the only things on the chain per panel are: flag -> 1 KB of x -> 32 FMAs -> reduction -> the
// 128 x 128 product from LDS -> publish.
// Hand-off (guide G16, recipe R1): x_p is stored write-through (relaxed agent-scope atomic stores = sc1), every storing wave
// drains its stores, one lane stores the flag; the consumer polls the flag relaxed from ONE lane and reads x_r with sc1 loads
// (L1 bypassed: no acquire fence on the chain).  Flags are zeroed by a memset in front of every launch.  Every spin is bounded:
// on a timeout bit 1 of info is set and every waiter gives up (the host reports an error instead of hanging the device).
// Panels are CLAIMED, last panel first, from one counter (flags[np]; round 6): a workgroup takes the next unclaimed panel
// when it arrives and again whenever it has finished one.  Panel p waits only for panels > p, and every one of those was claimed
// earlier by a workgroup that had already started, i.e. is resident and will finish it -- no assumption about dispatch order, about
// all G workgroups fitting the device at once, or about a second round of a workgroup's own panels (round 5's static
// `p -= gridDim.x` made ticket b's second panel wait for first-round panels of tickets that might not have started on a CU-masked
// device).  G = min(np, CUs of the device).
// Read a word other workgroups of the SAME launch write: a device-scope atomic ADD OF ZERO, written as inline assembly.
// Measured on MI355X (round 4): an agent-scope (sc1) LOAD in a poll loop -- and every atomic the compiler or the L2 can treat as a
// read: fetch_or 0 is folded into a load, a compare-and-swap that fails writes nothing -- can keep returning the value the line had
// when the poller's XCD first fetched it, for as long as nothing evicts the line: with all 256 workgroups waiting (nobody streams
// data) the chain sat on "3" for 300 ms while a copy from another stream showed 4.  An atomic that WRITES has to own the line, and
// the task counter of these very kernels shows those are coherent across the XCDs.  ~1-3 us per poll; pollers sleep in between.
__device__ __forceinline__ int chol_peek(int* word) {
  int seen;
  const int zero = 0;
  asm volatile("global_atomic_add %0, %1, %2, off sc0\n\ts_waitcnt vmcnt(0)" : "=v"(seen) : "v"(word), "v"(zero) : "memory");
  return seen;
}
constexpr int kBsThreads = 512;
constexpr int kBsMaxGrid = 256;
constexpr size_t kBsLds = (size_t)(kNB * kNB + kNB) * sizeof(double);
// sum over the 64 lanes of 16 per-lane values in 17 shuffles: after the four halving steps lane l holds the partial of value
// 8 b5 + 4 b4 + 2 b3 + b2 (b_k = bit k of l) summed over the lanes that agree with it in bits 1..0; two plain butterflies finish.
// The total of value v ends up in every lane of the quad { l : bits 5..2 of l spell v }.
__device__ __forceinline__ double bs_reduce16(double (&a)[16], int lane) {
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
  double b[8], c[4], d[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) { const double mine = h5 ? a[8 + i] : a[i], send = h5 ? a[i] : a[8 + i]; b[i] = mine + __shfl_xor(send, 32, 64); }
#pragma unroll
  for (int i = 0; i < 4; ++i) { const double mine = h4 ? b[4 + i] : b[i], send = h4 ? b[i] : b[4 + i]; c[i] = mine + __shfl_xor(send, 16, 64); }
#pragma unroll
  for (int i = 0; i < 2; ++i) { const double mine = h3 ? c[2 + i] : c[i], send = h3 ? c[i] : c[2 + i]; d[i] = mine + __shfl_xor(send, 8, 64); }
  double e = (h2 ? d[1] : d[0]) + __shfl_xor(h2 ? d[0] : d[1], 4, 64);
  e += __shfl_xor(e, 2, 64);
  e += __shfl_xor(e, 1, 64);
  return e;
}
static __global__ __launch_bounds__(kBsThreads) void k_chol_backsub(const double* __restrict__ M, long lda, int n, int np,
                                                                    const double* __restrict__ Linv_ws, double* x,
                                                                    int* flags, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  typedef double double2_t __attribute__((ext_vector_type(2)));
  double* Li = sm;                 // Linv_p, 128 x 128 column-major
  double* zs = sm + kNB * kNB;     // z_p
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  bool aborted = false;            // (thread 0 only; no static __shared__ here: it would shift the 16-byte alignment of sm, guide G17)
  const int c0 = 16 * wave;                                                   // this wave's 16 columns of the panel
  const int vcol = c0 + ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);   // bs_reduce16: whose total this lane ends up with
  for (;;) {
    __syncthreads();                                                           // the previous panel's readers of Li / zs are done
    if (t == 0) reinterpret_cast<int*>(zs)[0] = atomicAdd(&flags[np], 1);     // claim the next panel (the word behind the np panel flags)
    __syncthreads();
    const int p = np - 1 - reinterpret_cast<const int*>(zs)[0];
    __syncthreads();                                                           // everybody holds p before zs is written again
    if (p < 0) break;
    const int k0 = p * kNB, nb = (n - k0 < kNB) ? (n - k0) : kNB;
    {
      const double2_t* src = reinterpret_cast<const double2_t*>(Linv_ws + (size_t)p * kNB * kNB);
      double2_t* dst = reinterpret_cast<double2_t*>(Li);
#pragma unroll 4
      for (int e = t; e < kNB * kNB / 2; e += kBsThreads) dst[e] = src[e];
    }
    const double yv = (vcol < nb) ? M[(long)n + (long)(k0 + vcol) * lda] : 0.0;   // row n of the factored matrix: y = L^-1 b
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    double2_t blk[16];
    auto load_blk = [&](int r) {   // rows r 128 + 2 lane, + 1 of this wave's 16 columns
      const long row = (long)r * kNB + 2 * lane;
      const double* src = M + row + (long)(k0 + c0) * lda;
      if ((long)r * kNB + kNB <= (long)n) {
#pragma unroll
        for (int i = 0; i < 16; ++i) blk[i] = *reinterpret_cast<const double2_t*>(src + (long)i * lda);
      } else {                      // the last panel's partial block: rows >= n hold y^T and padding
        const bool v0 = row < n, v1 = row + 1 < n;
#pragma unroll
        for (int i = 0; i < 16; ++i) { blk[i].x = v0 ? src[(long)i * lda] : 0.0; blk[i].y = v1 ? src[(long)i * lda + 1] : 0.0; }
      }
    };
    if (np - 1 > p) load_blk(np - 1);
    for (int r = np - 1; r > p; --r) {
      if (t == 0 && !aborted) {
        const long long t0 = (long long)wall_clock64();
        unsigned spins = 0;
        while (chol_peek(&flags[r]) == 0) {
          __builtin_amdgcn_s_sleep(2);
          if ((++spins & 255u) == 0) {
            if (chol_peek(info) & 2) { aborted = true; break; }
            if ((long long)wall_clock64() - t0 > 300000000LL) { atomicOr(info, 2); aborted = true; break; }   // 3 s at 100 MHz
          }
        }
      }
      __syncthreads();
      const long xr = (long)r * kNB + 2 * lane;
      const double x0 = (xr < n) ? __hip_atomic_load(x + xr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      const double x1 = (xr + 1 < n) ? __hip_atomic_load(x + xr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] += blk[i].x * x0 + blk[i].y * x1;
      if (r - 1 > p) load_blk(r - 1);
    }
    const double tot = bs_reduce16(acc, lane);
    if ((lane & 3) == 0) zs[vcol] = yv - tot;
    __syncthreads();                                                           // z_p complete (and Li staged long ago)
    {
      const double z0 = zs[2 * lane], z1 = zs[2 * lane + 1];
      double o[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {                                           // x[r] = sum_c Linv(c, r) z[c]: column r of Linv is contiguous in c
        const double2_t v = *reinterpret_cast<const double2_t*>(Li + 2 * lane + (c0 + i) * kNB);
        o[i] = v.x * z0 + v.y * z1;
      }
      const double xo = bs_reduce16(o, lane);
      if ((lane & 3) == 0 && vcol < nb) __hip_atomic_store(x + k0 + vcol, xo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // write-through
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                           // every storing wave drains its stores ...
    __syncthreads();
    if (t == 0) __hip_atomic_store(&flags[p], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... then ONE lane publishes
  }
}

// pack / unpack of rows [r0, rows) x columns [c0, c0 + w) of M (dir 0: M -> buf, 1: buf -> M); buf column-major, height rows - r0
static __global__ __launch_bounds__(256) void k_chol_pack(double* __restrict__ M, long lda, long rows, long r0, long c0, double* __restrict__ buf, int dir) {
  const long h = rows - r0, i = (long)blockIdx.x * 256 + threadIdx.x, cidx = blockIdx.y;
  if (i >= h) return;
  if (dir == 0) buf[i + cidx * h] = M[(r0 + i) + (c0 + cidx) * lda];
  else M[(r0 + i) + (c0 + cidx) * lda] = buf[i + cidx * h];
}

// C += sum over the K slices of their partial products (slice order), lower triangle only
static __global__ __launch_bounds__(256) void k_chol_splitk_reduce(double* __restrict__ M, long lda, long rows, long ncols,
                                                                   const double* __restrict__ part, int nsplit) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long col = t / rows, row = t - col * rows;
  if (col >= ncols || row < col) return;
  double s = 0;
  for (int y = 0; y < nsplit; ++y) s += part[(size_t)y * (size_t)lda * (size_t)ncols + row + col * lda];
  M[row + col * lda] += s;
}

}  // namespace esl
