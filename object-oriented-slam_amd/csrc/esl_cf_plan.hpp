// esl_cf_plan.hpp — the layout decisions of the camera-first elimination (esl_cf.hpp: the maths and the kernels) as host-only code:
// dense or sparse X, the form, the segment length, T's column order and staircase, the segments' tables and every length that
// cf_ensure_impl (esl_slam.hip) lays out and ships.  No HIP header, no context: tests/cf_plan_main.cpp compiles this file alone and
// tests/test_cf_plan.py holds what it prints to numpy written from the definitions.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace esl {

constexpr int kCfFwdCh = 16;       // slots per chunk of the forward substitution (k_cf_forward) = the shortest segment
constexpr int kCfSyT = 128;        // tile of the per-segment product kernel (compact columns)
constexpr int kCfSegRows = 96;     // rows of a slab: 6 (kCfFwdCh - 1) = 90, padded with zero rows to a multiple of the T kernel's row batch
constexpr int kCfMaxStride = 128;  // longest segment of the nested dissection
constexpr int kCfKC = 16;          // K chunk of the rank-K update (kKC of esl_chol_kernels.hpp; esl_slam.hip asserts that they agree)
constexpr int kCfSparseMinCams = 256;   // X is kept sparse from this many free cameras on: below, the plan never looks at the memory size

// ---- choosing the segment length of form 3 -------------------------------------------------------------------------------------------
// Every stride-th camera is a separator, and the separators' dense rows cost a rank-6 (F / stride) update of T: that shrinks as
// 1 / stride, while the one-sided assembly's entry-products and the slabs grow with the segment (sublinearly: a wider segment sees
// more ellipsoids, but not twice as many).  With no stored products nothing else depends on the stride, so per trial
//     ms(stride) = update flops executed under the staircase / kCfUpdFlopsPerMs + entry-products x kCfPairMs + slab elements x kCfSlabMs
// (+ what does not depend on the stride) from counts the layout takes on the host for 16, 32 and 48.  The update's and the slabs'
// rates are the measured ones of the stride-16 form at 10k cameras and 2k ellipsoids (profiles/cf_onesided_gather_c4.md, sections
// 3 and 4):
//   k_chol_update_v        16.1 ms = 0.83 of the FP64 MFMA peak (79 TFLOP/s) on the flops it executes;
//   k_cf_forward<2> + k_cf_seg_back   0.77 + 0.53 ms over slabs of 1.35e8 elements (165 k live (segment, ellipsoid) columns x 9 x 90 rows).
// The assembly's 4.25 ms for 31.05 M entry-products there (0.137 ms per million) is an AVERAGE, and one point cannot tell what of
// it grows with the pairs: measured at the three strides (profiles/cf_stride_c4.md: 4.21 / 6.32 / 7.82 ms for 31.05 / 57.57 / 77.35 M)
// k_cf_T_onesided_lds takes 1.8 ms for its walk over T's 2 M blocks, whatever their lists hold, and 0.078 ms per million
// entry-products on top.  The marginal rate is the one a comparison of strides needs.
// (The rule still prices the row side over every entry, cf_os_counts: the list that is built since -- twins merged, the shorter side,
// cf_os_sides below -- is 0.65 - 0.75 of that at C4 and falls fastest at 48, so it only favours the wider stride;
// profiles/cf_os_sides_c4.md has the kernel's times on it.)
// A wider stride must win by kCfStrideMargin of the stride-16 figure: the rates move with the shapes (the update's C tile weighs more
// against a shorter K loop), and below that the choice is within what the model can tell.  Ties go to the narrower stride.
constexpr double kCfUpdFlopsPerMs = 0.83 * 79.0e9;
constexpr double kCfPairMs = (7.82 - 4.21) / (77.35e6 - 31.05e6);
constexpr double kCfSlabMs = 1.30 / 1.35e8;
constexpr double kCfStrideMargin = 0.05;
inline double cf_stride_cost(double upd_flops, double pairs, double slab) {
  return upd_flops / kCfUpdFlopsPerMs + pairs * kCfPairMs + slab * kCfSlabMs;
}
// upd_flops / pairs / slab [m - 1]: the counts with segments of m chunks.  n_o = order of the reduced system.
inline int cf_stride_choose(long n_o, const double* upd_flops, const double* pairs, const double* slab) {
  if (n_o < 8192) return kCfFwdCh;   // (below: the update is not the launch that carries the build)
  const double base = cf_stride_cost(upd_flops[0], pairs[0], slab[0]);
  int best = 1;
  double best_ms = base * (1.0 - kCfStrideMargin);
  for (int m = 2; m <= 3; ++m) {
    const double ms = cf_stride_cost(upd_flops[m - 1], pairs[m - 1], slab[m - 1]);
    if (ms < best_ms) { best = m; best_ms = ms; }
  }
  return best * kCfFwdCh;
}

// The environment as the caller read it (cf_ensure_impl: ESL_CF_SPARSE, ESL_CF_TPERM and ESL_CF_NO_ND at every layout, ESL_CF_ND_MIN
// once per process, ESL_CF_STRIDE, ESL_CF_OS_KERNEL and ESL_CF_OS_LIST when the context was created)
struct CfSwitches {
  int sparse = -1;         // ESL_CF_SPARSE: -1 unset, else the value's first character -- '0' dense X, '1' sparse (form by memory), '2' / '3' that form
  bool tperm_off = false;  // ESL_CF_TPERM=0: T keeps the ellipsoid order (A/B)
  bool no_nd = false;      // ESL_CF_NO_ND set: the plain chain, X dense (A/B)
  int nd_min = 48;         // ESL_CF_ND_MIN: first free-camera count that is dissected (at least two chunks)
  int stride = 0;          // ESL_CF_STRIDE: 16, 32 or 48 forces form 3's segment length, 0 = by cf_stride_choose
  int os_kernel = 1;       // ESL_CF_OS_KERNEL: 0 = the per-lane gather (k_cf_T_onesided) whatever the offsets' size
  int os_list = 1;         // ESL_CF_OS_LIST: 0 = the assembly's list walks the row side over every entry, twins apart (A/B: the bits of that list)
  int sweep = 1;           // ESL_CF_SWEEP: 0 = form 3 keeps the interior slab (k_cf_forward<2> + k_cf_seg_back + the slab's z: A/B, the parent's bits)
};

// The sparse form's tables for segments of S slots (the last slot of a segment is its separator): what cf_walk returns.
// Per segment the sorted list of ellipsoids with an edge at one of its interior cameras (seg_start / o), the compact slabs Xc
// (xoff / xld); per-segment products P_p = Xc_p^T Xc_p in 9 x 9 blocks (block (i1, i2), i1 >= i2, of segment p at
// boff[p] + i1 (i1 + 1) / 2 + i2), the right-hand side's row of every product (roff), the work lists of the per-segment kernels
// (fw_off: groups of 64 compact columns; tw_off: tiles of the product on and below the diagonal).
struct CfSegTables {
  int S = kCfFwdCh, nseg = 0, nw = 0;   // nw: 64-bit words of an ellipsoid's bitmap of segments
  std::vector<int> p, o, first;         // the incidences by (segment, first interior camera, ellipsoid): segment, ellipsoid, that camera's place in the segment
  std::vector<int> seg_start, xld, fw_off;
  std::vector<long long> xoff, boff, roff, tw_off;
  int n_fwork = 0, n_twork = 0;
  size_t xc_len = 0, p_blocks = 0, prhs_len = 0;
  double sp_flops = 0;   // FMAs of the per-segment products: block lower triangles, rows from each block row's first camera on
};
struct CfPlan : CfSegTables {
  int n_list = 0, n_chunks = 0;   // list entries (edges at free cameras), chunks of kCfFwdCh slots
  // X^T = (L^-1 [W | b_c])^T and T: leading dimensions (whole 128-row tiles: the update tiles read the pad rows instead of guarding
  // their last tile row, chol_update_tile_v), K padded to the update's chunk for all cameras (kpad) and for the separators (kpad_s)
  int64_t ldx = 0, ldt = 0, kpad = 0, kpad_s = 0;
  // nested dissection of the camera chain (esl_cf.hpp): every stride-th slot is a separator (0 = plain chain)
  bool nd = false;
  int stride = 0, n_sep = 0, n_seg = 1;
  // sparse interior rows of X (esl_cf.hpp, "X is sparse"): segments of S = stride slots (kCfFwdCh; form 3: one, two or three chunks).
  // form: 1 = products stored and gathered (k_cf_seg_syrk + k_cf_T_gather), 2 = blocks of T computed from the slabs directly
  // (k_cf_T_sparse: no P, more traffic), 3 = T's interior part assembled one-sided (k_cf_seg_back + k_cf_T_onesided: no P) from
  // Y = L_ii^T (L_p^-T X), one 54-double record per (segment, compact ellipsoid, interior slot), and the right-hand side's column per
  // slot (y_len doubles in all); os_flops = 2 x the FMAs of the assembly's 9 x 6 . 6 x 9 products
  bool sparse = false;
  int form = 0;
  std::vector<int> os, ou;   // every ellipsoid's list entries sorted by (slot, u): the slot, the edge
  size_t y_len = 0;
  // the assembly's pair list, built once per layout (k_cf_os_list): os_npairs (A record, B record) pairs.  os_offsets: a pair holds
  // the two records' first elements (entry x 54, Y record x 54; b row: slot x 6, entry x 54) for k_cf_T_onesided_lds -- false: their
  // numbers, for k_cf_T_onesided, which runs when the switch says so or an offset would not fit 32 bits
  size_t os_npairs = 0;
  bool os_offsets = false;
  double os_flops = 0;
  // The list the assembly walks unless ESL_CF_OS_LIST=0 (esl_cf.hpp, "twins and the shorter side").  A RUN is an ellipsoid's list
  // entries of one slot (a bounding-box and a 3-D edge of one camera: adjacent in os / ou); its first entry is the run's head and
  // stands for the run with the sum of its V records.  os_run[k] = length of the run whose head is entry k, at interior slots; 0 for
  // every other entry (not a head, or at a separator's slot).  os_heads[q] = run heads of incidence q (the order of p / o).
  // Per block of T and shared segment the list walks the ellipsoid with FEWER heads (ties and the diagonal: the row's):
  // osm_npairs = sum over the segments of sum_{i >= j} min(heads_i, heads_j) + the b row's heads; osm_flops as os_flops.
  // osm_row_npairs: twins merged, row side throughout (the middle column of profiles/cf_os_sides_c4.md).
  // os_list: the switch; os_list_npairs = the length of the list that is built, osm_npairs or os_npairs.
  // The sign bit of a pair's first number marks the swapped form; os_offsets keeps every offset below 2^31, so the bit is free.
  bool os_list = false;
  std::vector<int> os_run, os_heads;
  size_t osm_npairs = 0, osm_row_npairs = 0, os_list_npairs = 0;
  double osm_flops = 0;
  // Form 3 without the interior slab (esl_cf_sweep.hpp; ESL_CF_SWEEP).  The by-slot index of the entry lists, for z's W_I x_o:
  // sl_ent[q] = the entry (position in os / ou) that is the q-th of the per-camera lists cu_start / cu_obj, which give the slot's
  // range and the entry's ellipsoid.  xl_len: the last interior slot's six rows of every segment (sum of 6 xld).
  bool sweep = false;
  std::vector<int> sl_ent;
  size_t xl_len = 0;
  // T's ellipsoids in the order of their first free camera (sparse form): column block rank[o] of T / R / Xs belongs to ellipsoid o;
  // kfirst[g] = first row of Xs that can be non-zero in columns [64 g, 64 g + 64) (the rank-K update skips the rest);
  // upd_flops = what the dense update executes with the staircase
  bool tperm = false;
  std::vector<int> rank, unrank, kfirst;
  double upd_flops = 0;
};

// (slot, u) order per ellipsoid = the per-camera lists of slam_alloc (ellipsoids, then u, ascending inside a slot) walked in slot
// order and dealt to the ellipsoids: no comparison sort
inline void cf_entry_lists(int N, int nf, const std::vector<int>& start, const int* cu_start, const int* cu_obj, const int* cu_id,
                           std::vector<int>& os, std::vector<int>& ou) {
  std::vector<int> cur(start.begin(), start.end() - 1);
  os.assign((size_t)start[(size_t)N], 0); ou.assign((size_t)start[(size_t)N], 0);
  for (int sl = 0; sl < nf; ++sl)
    for (int q = cu_start[sl]; q < cu_start[sl + 1]; ++q) { const int at = cur[cu_obj[q]]++; os[(size_t)at] = sl; ou[(size_t)at] = cu_id[q]; }
}
// The same walk meets every (segment, ellipsoid) pair first at the ellipsoid's FIRST interior camera of the segment, slot by slot:
// the incidences come out sorted by (segment, first camera, ellipsoid) -- the compact column order of a segment's slab
// (upper-trapezoidal: column c is zero above row 6 first(c); a tile of the segment's product starts at the first camera of its
// first column) -- with no sort at all.
inline CfSegTables cf_walk(int S, int N, int nf, const int* cu_start, const int* cu_obj) {
  CfSegTables t;
  const int nseg = (nf + S - 1) / S;
  t.S = S; t.nseg = nseg; t.nw = (nseg + 63) / 64;
  std::vector<int> last_seg((size_t)N, -1);
  for (int sl = 0; sl < nf; ++sl) {
    const int p = sl / S, pos = sl - p * S;
    if (pos == S - 1) continue;   // (the last slot of a segment is its separator)
    for (int q = cu_start[sl]; q < cu_start[sl + 1]; ++q) {
      const int o = cu_obj[q];
      if (last_seg[(size_t)o] != p) { last_seg[(size_t)o] = p; t.p.push_back(p); t.o.push_back(o); t.first.push_back(pos); }
    }
  }
  const size_t n_inc = t.p.size();
  // rows of a slab: the padded kCfSegRows of the one-chunk forms' kernels, else the segment's interior rows as they are
  const long long rows = S == kCfFwdCh ? kCfSegRows : 6 * (S - 1);
  t.seg_start.assign((size_t)nseg + 1, 0); t.xld.assign((size_t)nseg, 0); t.fw_off.assign((size_t)nseg + 1, 0);
  t.xoff.assign((size_t)nseg + 1, 0); t.boff.assign((size_t)nseg + 1, 0); t.roff.assign((size_t)nseg + 1, 0); t.tw_off.assign((size_t)nseg + 1, 0);
  for (size_t q = 0; q < n_inc; ++q) ++t.seg_start[(size_t)t.p[q] + 1];
  for (int p = 0; p < nseg; ++p) t.seg_start[(size_t)p + 1] += t.seg_start[(size_t)p];
  for (size_t q = 0; q < n_inc; ++q)    // block row k of the product: k + 1 blocks, rows from its first camera on
    t.sp_flops += 81.0 * (double)(q - (size_t)t.seg_start[(size_t)t.p[q]] + 1) * (6.0 * (S - 1 - t.first[q]));
  for (int p = 0; p < nseg; ++p) {
    const int cnt = t.seg_start[(size_t)p + 1] - t.seg_start[(size_t)p];
    const int m = 9 * cnt + 1;
    t.xld[(size_t)p] = (m + 15) / 16 * 16 + 16;                          // + 16: the T kernel reads 16 columns from any column start
    t.xoff[(size_t)p + 1] = t.xoff[(size_t)p] + rows * t.xld[(size_t)p];
    t.fw_off[(size_t)p + 1] = t.fw_off[(size_t)p] + (m + 63) / 64;
    t.boff[(size_t)p + 1] = t.boff[(size_t)p] + (long long)cnt * (cnt + 1) / 2;
    t.roff[(size_t)p + 1] = t.roff[(size_t)p] + 9LL * cnt;
    const long long nt = (9 * cnt + kCfSyT - 1) / kCfSyT;
    t.tw_off[(size_t)p + 1] = t.tw_off[(size_t)p] + nt * (nt + 1) / 2;     // tiles of the product on and below the diagonal (ellipsoid columns only)
  }
  t.n_fwork = t.fw_off[(size_t)nseg]; t.n_twork = (int)t.tw_off[(size_t)nseg];
  t.xc_len = (size_t)t.xoff[(size_t)nseg] + 2 * kCfSyT;   // (+: the product kernel's last tile reads past the last slab's columns)
  t.p_blocks = (size_t)t.boff[(size_t)nseg]; t.prhs_len = (size_t)t.roff[(size_t)nseg];
  return t;
}
// kfirst per 64 columns of T for segments of S slots: the first separator whose right-hand side R(k) can hold the column's
// ellipsoid is the one in FRONT of the segment of its first camera (an interior camera's segment hands its sum to the separator
// before it; conservative for a separator camera itself), and the right-hand side's ROW (row n_o of T, X^T y) is dense from the
// start.  upd_flops: the flops the update executes (k_chol_update_v, the default tile of the big launches): per 128 x 128 tile of the
// lower triangle, K from the later of the tile's two earliest rows on, rounded down to a chunk pair as the kernel does; a tile on
// the diagonal counts its lower triangle.  (The 256 x 128 tile of ESL_UPD_V=0 starts a little earlier: it executes ~1 % more.)
// first_cam[o]: the first free camera of ellipsoid o (nf: none).
inline double cf_staircase(int S, int N, int nf, const std::vector<int>& unrank, const std::vector<int>& first_cam, std::vector<int>& kfirst) {
  const size_t n_o = (size_t)9 * N;
  double upd_flops = 0;
  const int Ks = (int)((6 * ((size_t)nf / (size_t)S) + kCfKC - 1) / kCfKC * kCfKC);
  kfirst.assign((n_o + 1 + 256) / 64 + 8, Ks);
  for (size_t col = 0; col < n_o; ++col) {
    const int k0 = std::max(0, first_cam[(size_t)unrank[col / 9]] / S - 1);
    kfirst[col / 64] = std::min(kfirst[col / 64], std::min(6 * k0, Ks));
  }
  kfirst[n_o / 64] = 0;   // the right-hand side's row
  const long nti = ((long)n_o + 1 + 127) / 128;
  for (long ti = 0; ti < nti; ++ti) {
    const int ka = std::min(kfirst[(size_t)(ti * 2)], kfirst[(size_t)(ti * 2 + 1)]);
    for (long tj = 0; tj <= ti && tj * 128 < (long)n_o; ++tj) {
      const int kb = std::min(kfirst[(size_t)(tj * 2)], kfirst[(size_t)(tj * 2 + 1)]);
      int ks = std::min(std::max(ka, kb), Ks) & ~(kCfKC - 1);
      if (((Ks - ks) & kCfKC) != 0 && ks >= kCfKC) ks -= kCfKC;
      const double rows_t = (double)std::min<long>(128, (long)n_o + 1 - ti * 128), cols_t = (double)std::min<long>(128, (long)n_o - tj * 128);
      const double in_triangle = tj < ti ? 1.0 : 0.5 * (cols_t + 1.0) / cols_t;
      upd_flops += 2.0 * rows_t * cols_t * (double)(Ks - ks) * in_triangle;
    }
  }
  return upd_flops;
}
// What the one-sided assembly executes with segments of S slots: per block (t1 >= t2) of T and shared segment, one 9 x 6 . 6 x 9
// product per interior list entry of o1 in the segment; the b row one 6 x 9 . 6 product per interior entry.  (Segment, position in
// T's order, entries) of every incidence, by segment and position: the incidence at place q of its segment meets q + 1 partners.
// rank: T's order (empty: the ellipsoid order).
struct CfOsCounts { double prod = 0, rhs_entries = 0; };
inline CfOsCounts cf_os_counts(int S, int N, const std::vector<int>& start, const std::vector<int>& os, const std::vector<int>& rank) {
  std::vector<std::array<int, 3>> inc3;
  CfOsCounts n;
  for (int o = 0; o < N; ++o) {
    int last_p = -1;
    for (int k = start[(size_t)o]; k < start[(size_t)o + 1]; ++k) {
      const int sl = os[(size_t)k];
      if (sl % S == S - 1) continue;
      const int p = sl / S;
      if (p != last_p) { inc3.push_back({p, rank.empty() ? o : rank[(size_t)o], 0}); last_p = p; }
      ++inc3.back()[2]; n.rhs_entries += 1;
    }
  }
  std::sort(inc3.begin(), inc3.end());
  for (size_t q = 0, q0 = 0; q < inc3.size(); ++q) {
    if (inc3[q][0] != inc3[q0][0]) q0 = q;
    n.prod += (double)inc3[q][2] * (double)(q - q0 + 1);
  }
  return n;
}

// Twins and the shorter side (CfPlan::os_run ...): the runs of every ellipsoid's interior entries, the run heads of every incidence
// -- an ellipsoid's incidences come in ascending segment order in p / o, as its entries do in os, so one cursor per ellipsoid finds
// them -- and the lengths of the merged lists.  Per segment with head counts v sorted ascending, sum_{i >= j} min(v_i, v_j) =
// sum_i v_(i) (n - i): the i-th smallest is the minimum against itself and the n - 1 - i larger ones.
// Every incidence has at least one head: cf_walk makes an incidence where it meets an interior entry, so "o2 is live in the segment"
// and "o2 has heads there" are the same set in osm_row_npairs.
inline void cf_os_sides(CfPlan& pl, const std::vector<int>& start) {
  const int S = pl.S;
  const size_t n_inc = pl.p.size();
  pl.os_run.assign(pl.os.size(), 0); pl.os_heads.assign(n_inc, 0);
  std::vector<int> cur(start.begin(), start.end() - 1);
  for (size_t q = 0; q < n_inc; ++q) {
    const int o = pl.o[q], p = pl.p[q], end = start[(size_t)o + 1];
    int k = cur[(size_t)o];
    while (k < end && pl.os[(size_t)k] / S < p) ++k;   // (separator entries of segments without an interior one)
    for (int head = -1; k < end && pl.os[(size_t)k] / S == p; ++k) {
      const int sl = pl.os[(size_t)k];
      if (sl % S == S - 1) continue;
      if (head < 0 || pl.os[(size_t)head] != sl) { head = k; ++pl.os_heads[q]; }
      ++pl.os_run[(size_t)head];
    }
    cur[(size_t)o] = k;
  }
  double both = 0, row = 0, brow = 0;
  std::vector<int> v;
  std::vector<std::pair<int, int>> byrank;
  for (int p = 0; p < pl.nseg; ++p) {
    const int q0 = pl.seg_start[(size_t)p], n = pl.seg_start[(size_t)p + 1] - q0;
    v.assign(pl.os_heads.begin() + q0, pl.os_heads.begin() + q0 + n);
    std::sort(v.begin(), v.end());
    for (int i = 0; i < n; ++i) { both += (double)v[(size_t)i] * (double)(n - i); brow += v[(size_t)i]; }
    byrank.clear();
    for (int i = 0; i < n; ++i) { const int o = pl.o[(size_t)(q0 + i)]; byrank.push_back({pl.rank.empty() ? o : pl.rank[(size_t)o], pl.os_heads[(size_t)(q0 + i)]}); }
    std::sort(byrank.begin(), byrank.end());
    for (int i = 0; i < n; ++i) row += (double)byrank[(size_t)i].second * (double)(i + 1);
  }
  pl.osm_npairs = (size_t)(both + brow); pl.osm_row_npairs = (size_t)(row + brow);
  pl.osm_flops = 2.0 * 6.0 * (81.0 * both + 9.0 * brow);
}

// The plan of one layout.  start = per-ellipsoid list starts (N + 1), cu_* = the per-camera lists of slam_alloc, EU = edge slots
// (bounding-box + 3-D), comm = a communicator is present, total_mem = the device's TOTAL memory in bytes.
// false: the (ellipsoid, camera chunk) range table of this graph exceeds 1 GB (nothing else can fail).
inline bool cf_plan_build(int N, int nf, size_t EU, const std::vector<int>& start, const int* cu_start, const int* cu_obj, const int* cu_id, bool chain_ok,
                          bool comm, size_t total_mem, const CfSwitches& sw, CfPlan& pl) {
  pl = CfPlan{};
  const size_t nfz = (size_t)nf, n_o = (size_t)9 * N;
  const int nch = (nf + kCfFwdCh - 1) / kCfFwdCh;
  pl.ldx = (int64_t)((n_o + 1 + 127) / 128 * 128);
  pl.kpad = (int64_t)((6 * nfz + kCfKC - 1) / kCfKC * kCfKC);
  pl.ldt = pl.ldx;
  pl.n_list = start[(size_t)N]; pl.n_chunks = nch;
  pl.nseg = nch; pl.nw = (nch + 63) / 64;
  if ((size_t)std::max(N, 1) * (size_t)(nch + 1) > ((size_t)1 << 28)) return false;
  cf_entry_lists(N, nf, start, cu_start, cu_obj, cu_id, pl.os, pl.ou);
  CfSegTables& seg = pl;
  if (chain_ok && nf >= kCfSparseMinCams && N > 0 && (size_t)nch * (size_t)(N + 1) <= ((size_t)1 << 28) && !sw.no_nd) {
    seg = cf_walk(kCfFwdCh, N, nf, cu_start, cu_obj);
    // X sparse or dense (esl_cf.hpp, "sparse interior rows"): flops of the dense rank-6 nf update against the separators' dense
    // rows plus the per-segment products at a quarter of the MFMA rate; ESL_CF_SPARSE=1 / 0 forces it (A/B and the parity tests)
    const double dense = (double)n_o * (double)n_o * 6.0 * (double)nfz;
    const double sparse = (double)n_o * (double)n_o * 6.0 * (double)(nfz / kCfFwdCh) + 24.0 * pl.sp_flops;   // (sp_flops: FMAs of the products' lower triangles)
    pl.sparse = sw.sparse >= 0 ? sw.sparse != '0' : (n_o >= 2048 && sparse < 0.5 * dense);
    // the per-segment products are stored when they fit beside everything else (C4: 14 GB); else (or ESL_CF_SPARSE=2) the blocks
    // of T come straight from the slabs (k_cf_T_sparse).  Decided from the graph's size against the device's TOTAL memory, not from
    // what happens to be free at the first trial: the two forms add in different orders, so the bits of T must not depend on what
    // else occupies the GPU; every rank of a replicated run takes the same decision by construction.
    // esl_lm_solver_stats reports the form.
    const double need = 8.0 * (81.0 * (double)pl.p_blocks + (double)pl.xc_len + 2.0 * (double)pl.ldt * (double)n_o +
                               2.0 * 6.0 * (double)(nfz / kCfFwdCh) * (double)pl.ldx /* Xs, R */ + 54.0 * (double)EU /* V */);
    pl.form = sw.sparse == '2' || need > 0.4 * (double)total_mem ? 2 : 1;
    // form 3 (esl_cf.hpp, "one-sided assembly"): no product store, so the memory rule above does not apply to it.  ESL_CF_SPARSE=3
    // forces it; unset, it is the form wherever X is kept sparse on a single rank.  1 / 2 / 0 keep their paths and bits; a run
    // with a communicator keeps its present form.
    if ((sw.sparse < 0 || sw.sparse == '3') && !comm) pl.form = 3;
  }
  const bool sp = pl.sparse;
  // T's ellipsoids by first free camera (sparse form; ESL_CF_TPERM=0: ellipsoid order, A/B): rank by a counting sort over the
  // first slot of every ellipsoid's (slot-sorted) list, ellipsoids without a free-camera edge last
  std::vector<int> first_cam;
  pl.tperm = sp && N > 0 && !sw.tperm_off;
  if (pl.tperm) {
    std::vector<int> cnt(nfz + 2, 0);
    first_cam.assign((size_t)N, nf);
    for (int o = 0; o < N; ++o) if (start[(size_t)o + 1] > start[(size_t)o]) first_cam[(size_t)o] = pl.os[(size_t)start[(size_t)o]];
    for (int o = 0; o < N; ++o) ++cnt[(size_t)first_cam[(size_t)o] + 1];
    for (int s = 0; s <= nf; ++s) cnt[(size_t)s + 1] += cnt[(size_t)s];
    pl.rank.assign((size_t)N, 0); pl.unrank.assign((size_t)N, 0);
    for (int o = 0; o < N; ++o) { const int t = cnt[(size_t)first_cam[(size_t)o]]++; pl.rank[(size_t)o] = t; pl.unrank[(size_t)t] = o; }
  }
  // The segment length of form 3 (above, "choosing the segment length"): ESL_CF_STRIDE, else kCfFwdCh unless the reduced system is large
  // enough for the separators' update to carry the launch (9 N >= 8192: k_chol_update_v), and then what cf_stride_choose makes of this
  // graph's counts.  Every other form, and a run with a communicator, keeps kCfFwdCh.
  if (sp && pl.form == 3 && !comm) {
    int want = sw.stride;
    CfSegTables cand[3];
    if (!want && pl.tperm && n_o >= 8192) {
      double upd[3], pairs[3], slab[3];
      for (int m = 1; m <= 3; ++m) {
        const int S = m * kCfFwdCh;
        cand[m - 1] = cf_walk(S, N, nf, cu_start, cu_obj);
        const CfOsCounts n = cf_os_counts(S, N, start, pl.os, pl.rank);
        long long cols = 0;
        for (int x : cand[m - 1].xld) cols += x;
        upd[m - 1] = cf_staircase(S, N, nf, pl.unrank, first_cam, pl.kfirst); pairs[m - 1] = n.prod + n.rhs_entries; slab[m - 1] = 6.0 * (S - 1) * (double)cols;
      }
      want = cf_stride_choose((long)n_o, upd, pairs, slab);
      seg = std::move(cand[want / kCfFwdCh - 1]);
    }
    if (!want) want = kCfFwdCh;
    if (want != pl.S) seg = cf_walk(want, N, nf, cu_start, cu_obj);
  }
  // nested dissection of the camera chain from nd_min free cameras on (default 48, three segments; 128 until round 6: at 119 free
  // cameras the plain chain's two serial sweeps, k_cf_chain 72 us + k_cf_forward 69 us, were a quarter of a streaming-size trial):
  // stride = 16 x round(sqrt(nf) / 16) in [16, 128] (a multiple of the forward substitution's chunk, so that segments start on chunk
  // boundaries), the segment length S when X is kept sparse; ESL_CF_NO_ND=1 keeps the plain chain (A/B)
  pl.nd = nfz >= (size_t)std::max(sw.nd_min, 2 * kCfFwdCh) && !sw.no_nd;
  if (pl.nd) {
    int sd = 16 * (int)std::max(1.0, std::floor(std::sqrt((double)nfz) / 16.0 + 0.5));
    sd = std::min(sd, kCfMaxStride);
    if (sp) sd = pl.S;
    pl.stride = sd; pl.n_sep = nf / sd; pl.n_seg = (nf + sd - 1) / sd;
  }
  if (sp) pl.kpad_s = (int64_t)((6 * (size_t)pl.n_sep + kCfKC - 1) / kCfKC * kCfKC);
  if (pl.tperm) pl.upd_flops = cf_staircase(pl.S, N, nf, pl.unrank, first_cam, pl.kfirst);
  if (sp && pl.form == 3) {
    const CfOsCounts n = cf_os_counts(pl.S, N, start, pl.os, pl.rank);
    const size_t y_recs = std::max<size_t>(pl.p.size(), 1) * (size_t)(pl.S - 1);
    pl.os_flops = 2.0 * 6.0 * (81.0 * n.prod + 9.0 * n.rhs_entries);
    pl.os_npairs = (size_t)(n.prod + n.rhs_entries);   // (record pairs of the assembly: the length of its list)
    pl.y_len = y_recs * 54 + std::max<size_t>(nfz, 1) * 6;
    // element offsets for k_cf_T_onesided_lds where every record's first element fits the list's 32 bits (C4: 1.4e8), else record
    // numbers and the per-lane gather
    pl.os_offsets = sw.os_kernel != 0 && 54 * std::max(EU, y_recs) <= (size_t)INT32_MAX;
    cf_os_sides(pl, start);
    pl.os_list = sw.os_list != 0;
    pl.os_list_npairs = pl.os_list ? pl.osm_npairs : pl.os_npairs;
    pl.sweep = sw.sweep != 0;
    if (pl.sweep) {   // cf_entry_lists' walk again: entry `at` of the ellipsoid's list is the q-th of its camera's
      std::vector<int> cur(start.begin(), start.end() - 1);
      pl.sl_ent.assign((size_t)cu_start[nf], 0);
      for (int sl = 0; sl < nf; ++sl)
        for (int q = cu_start[sl]; q < cu_start[sl + 1]; ++q) pl.sl_ent[(size_t)q] = cur[cu_obj[q]]++;
      long long cols = 0;
      for (int x : pl.xld) cols += x;
      pl.xl_len = 6 * (size_t)cols;
    }
  }
  return true;
}

}  // namespace esl
