// esl_chol_plan.hpp — the static task list of the persistent dense factorisation (k_chol_persist, esl_chol_persist.hpp): host code and
// __host__ __device__ helpers only.  tests/test_chol_plan.py replays the list on the CPU through esl_debug_chol_plan.
#pragma once
#include <algorithm>
#include <vector>

#include "esl_chol_kernels.hpp"   // kNB

namespace esl {

// Tasks of the list (the roles and the dependency words: esl_chol_persist.hpp), on the absolute tile grid:
// 0: S(panel a, strip b)   1: u(panel a, row tile b, column tile c)   2: U(outer panel a, row tile b, column tile c)
// 3: a QUARTER of u(panel a, row tile b, column tile c & 0xffff): rows 256 b + 128 h, columns 128 J + 64 g with h = bit 16, g = bit 17
//    of c, bits 18-20 = the number of quarters of THIS update that are tasks, bits 21-23 = the number a whole update of the tile has
//    (those that meet the lower triangle and the matrix; fewer are tasks when the chain takes the diagonal block itself).
//    The DIAGONAL tile of the next panels takes its rank-128 updates in quarters: it sits between the solve of panel k and the
//    diagonal block of panel k + 1, i.e. on the critical path of the chain, where one workgroup needs 42 us for the whole tile and
//    four need ~12 us for a quarter each (round 4: 62 panels x 30 us of the last 8,000 columns of an order-18,000 system).
struct CholTask { int type, a, b, c; };
struct CholPlan {
  int n = 0, np = 0, W = 0, n_outer = 0, nR = 0;
  int fuse = 0;          // the chain solves the two strips under its diagonal block and updates the next diagonal block itself (below)
  int merge = 1;         // far updates of a tile taken `merge` outer panels at a time (round 6: one visit with K = merge x W x 128)
  int strip_merge = 0;   // the strips of a row tile away from the diagonal as one task (round 6)
  int sp = 1;            // leading column panels of an outer panel whose chain tiles are fed rank-128 updates panel by panel (chol_tile_special)
  std::vector<CholTask> tasks;
  std::vector<int> ns;   // [np][nR]
};
// Updates a tile (R, J) of the lower triangle receives before panel J is factored, in this order: nU rank-(W x 128) updates U(o), one
// per EARLIER outer panel, then rank-128 updates from the panels in front of J.  Ordinarily those are the J % W panels of J's own
// outer panel.  The DIAGONAL tile of an outer panel's FIRST column panel (J % W == 0, R == J / 2) is special: it takes the
// previous outer panel's contribution as W rank-128 updates (in quarters), one per panel as that panel is solved, instead of
// inside U(o - 1) -- otherwise the chain's step across an outer-panel boundary waits for a whole rank-512 tile update (~150 us)
// that cannot start before the LAST panel of the outer panel is solved.
// Round 6: SP leading column panels of every outer panel are special in this sense (default 2), in the diagonal tile's row AND the row tile
// under it (R == J / 2 + 1: its strips of panel J are what the next panels' chain tiles wait for).  Measured with SP = 1, R == J / 2
// only, by the panel's position in its outer panel over the chain-bound part: gap to the next block 60 / 36 / 27 / 27 us at n = 8,192
// against 26 us of the chain's own work -- at the first panel of an outer panel the fused stage waited ~34 us for the rank-(W x 128)
// update of the NEXT diagonal tile (ke / 2, ke + 1), which cannot start before the outer panel's last solve.  Making only that tile
// special moved the stall to the next step (27 / 68 / 27 / 27): there the chain waits for tile (ke / 2 + 1, ke + 1), whose update by panel
// ke needs panel ke's strips in row tile ke / 2 + 1, which wait for tile (ke / 2 + 1, ke) to be final -- another 150 us rank-512 update.
// A special tile receives, in this order: the rank-(W x 128) updates of outer panels 0 .. J / W - 2, then W rank-128 updates from the
// panels of outer panel J / W - 1, then J % W rank-128 updates from the earlier panels of its own outer panel.
__host__ __device__ __forceinline__ bool chol_tile_special(int R, int J, int W, int SP) { return J >= W && (J % W) < SP && (R == J / 2 || R == J / 2 + 1); }
__host__ __device__ __forceinline__ int chol_tile_nU(int R, int J, int W, int SP) { return J / W - (chol_tile_special(R, J, W, SP) ? 1 : 0); }
// index, among the rank-128 updates tile (R, J) receives, of the one from panel a (a in J's outer panel or, special tiles, the one before)
__host__ __device__ __forceinline__ int chol_tile_ridx(int R, int J, int W, int SP, int a) { return ((a / W == J / W && chol_tile_special(R, J, W, SP)) ? W : 0) + a % W; }
// sequence number of that update: the value of ver[R][J] it waits for (and leaves at + 1)
__host__ __device__ __forceinline__ int chol_tile_seq(int R, int J, int W, int SP, int a) { return chol_tile_nU(R, J, W, SP) + chol_tile_ridx(R, J, W, SP, a); }
__host__ __device__ __forceinline__ int chol_tile_final(int R, int J, int W, int SP) { return chol_tile_nU(R, J, W, SP) + (chol_tile_special(R, J, W, SP) ? W : 0) + J % W; }
// quarter (h, g) of tile (R, J): rows 256 R + 128 h .. + 128, columns 128 J + 64 g .. + 64
__host__ __device__ inline bool chol_quarter_live(int R, int J, int h, int g, long rows, int n) {
  const long i0 = 256L * R + 128L * h, j0 = 128L * J + 64L * g;
  return i0 < rows && j0 < n && i0 + 127 >= j0;
}
inline void chol_plan_build(int n, int W, int filler, CholPlan& pl, bool fuse = false, int merge = 1, bool strip_merge = false, int sp = 1) {
  const long rows = (long)n + 1;
  pl.fuse = fuse ? 1 : 0;
  pl.merge = merge < 1 ? 1 : merge;
  pl.strip_merge = strip_merge ? 1 : 0;
  pl.sp = sp < 1 ? 1 : (sp > W ? W : sp);
  const int SP = pl.sp;
  pl.n = n; pl.W = W; pl.np = (n + kNB - 1) / kNB; pl.n_outer = (pl.np + W - 1) / W; pl.nR = (int)((rows + 255) / 256);
  const int np = pl.np, nR = pl.nR;
  pl.ns.assign((size_t)np * nR, 0);
  pl.tasks.clear();
  auto live = [&](int R, int J) { return 256L * R + 255 >= 128L * J && 256L * R < rows; };   // the tile meets the lower triangle (or the b row)
  auto k0s = [&](int k) { const long k0 = 128L * k; return k0 + std::min<long>(kNB, n - k0); };   // first row under panel k's diagonal block
  auto strips = [&](int k) { const long k0 = 128L * k, nb = std::min<long>(kNB, n - k0), below = rows - (k0 + nb); return (int)(below > 0 ? (below + 63) / 64 : 0); };
  for (int k = 0; k < np; ++k) {
    const long k0 = 128L * k, nb = std::min<long>(kNB, n - k0);
    for (int i = 0; i < strips(k); ++i) pl.ns[(size_t)k * nR + (size_t)((k0 + nb + 64L * i) / 256)]++;
  }
  std::vector<CholTask> prevA, prevB;   // the previous outer panel's rank-(W x 128) updates: this outer panel's columns / everything beyond
  for (int o = 0; o < pl.n_outer; ++o) {
    const int kb = o * W, ke = std::min(np, kb + W);
    pl.tasks.insert(pl.tasks.end(), prevA.begin(), prevA.end());
    size_t bpos = 0;
    auto fill = [&]() { const size_t e = std::min(prevB.size(), bpos + (size_t)filler); pl.tasks.insert(pl.tasks.end(), prevB.begin() + bpos, prevB.begin() + e); bpos = e; };
    for (int k = kb; k < ke; ++k) {
      fill();                                              // (work for the others while the chain factors block k)
      // (fused: strips 0, 1 are the chain's.)  Round 6: the strips of ONE row tile are one task where nobody is waiting for the first
      // of them alone -- every consumer of a solved row tile waits for all of its strips (sdone == ns) anyway, and a strip is ~9 us of
      // work behind ~20 us of task hand-off.  The row tiles next to the diagonal block keep their 64-row strips: they feed the quarters
      // of the next diagonal tiles, i.e. the chain, and four workgroups finish them sooner than one.  c = strips in the task.
      for (int i = fuse ? 2 : 0; i < strips(k);) {
        const long R = (k0s(k) + 64L * i) / 256;
        int cnt = 1;
        if (pl.strip_merge && R >= k0s(k) / 256 + 2)
          while (i + cnt < strips(k) && (k0s(k) + 64L * (i + cnt)) / 256 == R) ++cnt;
        pl.tasks.push_back(CholTask{0, k, i, cnt});
        i += cnt;
      }
      bool any = false;
      auto quarters = [&](int R, int J) {
        // (q & 1 = h: which 128 rows, q >> 1 = g: which 64 columns.)  Fused chain: panel J - 1's update of the diagonal BLOCK of
        // tile (J / 2, J) -- the half h = J & 1 -- is the chain's; the workers keep the other half, if it is below the diagonal
        const bool chains = fuse && k == J - 1 && R == J / 2;
        int full = 0, mine = 0;
        for (int q = 0; q < 4; ++q)
          if (chol_quarter_live(R, J, q & 1, q >> 1, rows, n)) { ++full; if (!(chains && (q & 1) == (J & 1))) ++mine; }
        for (int q = 0; q < 4; ++q)
          if (chol_quarter_live(R, J, q & 1, q >> 1, rows, n) && !(chains && (q & 1) == (J & 1)))
            pl.tasks.push_back(CholTask{3, k, R, J | ((q & 1) << 16) | ((q >> 1) << 17) | (mine << 18) | (full << 21)});
      };
      // the next outer panel's first diagonal tile takes this panel's rank-128 contribution now (chol_tile_special); of all of the
      // panel's updates it is the one the chain will wait for soonest when k is the outer panel's last, so it goes first
      for (int J = ke; J < std::min(np, ke + W); ++J)
        for (int R = J / 2; R <= J / 2 + 1; ++R)
          if (chol_tile_special(R, J, W, SP) && live(R, J)) { if (!any) { fill(); any = true; } quarters(R, J); }
      for (int J = k + 1; J < ke; ++J)
        for (int R = J / 2; R < nR; ++R)
          if (live(R, J)) {
            if (!any) { fill(); any = true; }
            // quarters for the diagonal tile AND, when panel J's block is the lower half of its tile (J odd), for the tile under it:
            // its upper half holds the rows under block J, which the fused chain solves next -- as one task it is 42 us in the
            // chain's way on every other step
            if (R != J / 2 && R != (J + 1) / 2) { pl.tasks.push_back(CholTask{1, k, R, J}); continue; }
            quarters(R, J);
          }
    }
    pl.tasks.insert(pl.tasks.end(), prevB.begin() + bpos, prevB.end());
    prevA.clear(); prevB.clear();
    const int ne = std::min(np, ke + W);
    // Round 6: a tile's FAR updates -- those of outer panels o <= J / W - 2, which only fill the workers' time -- are taken `merge` outer
    // panels at a time: one visit of the tile with K = merge x W x 128 instead of `merge` visits (each visit pays ~22 us of task
    // hand-off, first-chunk staging and the read-modify-write of C beside ~127 us of K loop).  A group [g0, g0 + cnt) goes into the
    // list when its LAST outer panel is solved; the update of the outer panel right in front of the tile's own (o = J / W - 1, the one
    // the chain waits for) stays a visit of its own.  c = J | cnt << 16; sequence number g0 -> g0 + cnt.
    for (int J = ke; J < np; ++J)
      for (int R = J / 2; R < nR; ++R)
        if (live(R, J) && !(J < ne && chol_tile_special(R, J, W, SP))) {   // (special tiles took this outer panel's contribution panel by panel)
          if (J < ne) { prevA.push_back(CholTask{2, o, R, J | (1 << 16)}); continue; }
          const int far = J / W - 1;                     // far updates of this tile: o = 0 .. far - 1 (this o is one of them: J >= ne)
          // the groups of different tiles are STAGGERED (boundaries shifted by a hash of the tile): with one grid of boundaries for all
          // tiles every far task of `merge` outer panels enters the list at once and the panels in between have no filler work at all
          // (measured: waiting 2.7 -> 3.8 ms while the bodies fell 36.5 -> 34.1)
          const int shift = (R + 2 * J) % pl.merge, q = (o + shift) / pl.merge;
          const int g0 = std::max(0, q * pl.merge - shift), ge = std::min((q + 1) * pl.merge - shift, far) - 1;
          if (o == ge) prevB.push_back(CholTask{2, g0, R, J | ((ge - g0 + 1) << 16)});
        }
  }
}

}  // namespace esl
