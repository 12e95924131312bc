// esl_dense_planes.hip — esl_dense_planes (include/esl.h, "dominant planes and the ground from the dense map"; the steps' numbers below
// are the header's; arithmetic and host decisions: esl_dense_planes.hpp).  It works on the dense map's sorted list (esl_dense_int.hpp,
// whose rule on stores and bounded probes holds here): k_dpl_gate (eligible voxels, their total and box); per round a stable select
// of the unassigned eligible voxels (U_r: dense_select_free), k_dpl_pack (centre and count of every entry, 32 bytes), k_dpl_gather (the keys of
// the hypotheses' entries; the host builds the planes), k_dpl_score (every hypothesis against all of U_r: lane = hypothesis, the list
// staged in LDS tiles and read by broadcast; with fewer than 64 hypotheses k_dpl_few scores them, lane = voxel) and k_dpl_one (one
// plane against U_r, lane = voxel: the integer moments of its inliers, and their assignment); k_dpl_vout (every voxel's plane).
#include "esl_dense_int.hpp"
#include "esl_dense_planes.hpp"

namespace esl {

// the call's buffers (DenseState::pl_set)
enum { DB_PSTATE, DB_PCTR, DB_PBOX, DB_PLIST, DB_PSELTMP, DB_PVOX, DB_PGKEY, DB_PPLANES, DB_PVALID, DB_PHACC, DB_PMOM, DB_PVOUT, DB_PL_COUNT };
static_assert(DB_PL_COUNT == kDplBufs, "esl_dense_int.hpp sizes DenseState::pl_set");

// state[i] of voxel i of the sorted list: -1 not eligible, -2 eligible and unassigned, p >= 0 assigned to plane p.  U_r is the list of
// the indices i with state -2, ascending (a stable select), and vox[j] the centre and count of its j-th entry.
enum { DP_ELIGIBLE, DP_NR, DP_COUNT };
constexpr int kDplTile = 512;       // entries of U_r per LDS tile of k_dpl_score: 16 KiB
constexpr int kDplGroup = 256;      // hypotheses per workgroup of k_dpl_score, one per lane
constexpr int kDplMaxChunks = 256;  // workgroups along the list
constexpr int kDplSmall = 64;       // fewer hypotheses than this (one wave) are scored by k_dpl_few, lane = voxel
struct DplVox { double x[3]; long long count; };
static_assert(sizeof(DplVox) == 32, "two 16-byte loads per entry");

struct DplArgs {
  const DenseRec* rec; u64 H;
  const u64* skey; const unsigned int* sval; int n;
  int* state;
  int min_count, skip_labelled;
  u64* ctr; int* box;                       // DP_*; kmin, kmax of the eligible voxels
  const int* list; DplVox* vox;             // U_r (its length: ctr[DP_NR]); n entries at most
  u64* gkeys; int n_hyp, round; u64 seed;   // 3 n_hyp packed keys
  const double* planes; const int* valid;   // n_hyp x 4; n_hyp
  u64* hacc;                                // n_hyp x 2: inlier voxels, inlier samples
  int n_r;
  double leaf, dist_tol;
  double one[4]; int assign; int kmin[3]; u64* mom;   // the one-plane pass: kDplMoments sums; assign >= 0: the inliers take this plane
  int* vout; long long n_vout;
};

// The two kernels with one target for all their sums (k_dpl_gate, k_dpl_one) run as at most kDplReduceBlocks workgroups that stride over
// the list: a lane keeps its sums in registers, a wave folds them by a butterfly, the workgroup's waves meet in LDS and one lane per
// sum emits the workgroup's atomic.  One atomic per WAVE and sum on the same few addresses cost 0.13 ms (k_dpl_one) and 0.48 ms
// (k_dpl_gate) per launch on the synthetic room's 435,533 voxels.
constexpr int kDplReduceBlocks = 512;
constexpr int kDplWaves = kDenseThreads / 64;

// step 1 over the sorted list
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_gate(DplArgs a) {
  __shared__ int part[kDplWaves][7];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt = 0;
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  for (long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x; i < a.n; i += (long long)gridDim.x * kDenseThreads) {
    const unsigned int slot = a.sval[i];
    bool el = false;
    if (slot < a.H) {
      const u64 best = a.rec[slot].best, count = a.rec[slot].count;
      el = (long long)count >= (long long)a.min_count && !(a.skip_labelled && best != 0);
    }
    a.state[i] = el ? -2 : -1;
    if (el) {
      int k[3];
      dense_unpack(a.skey[i], k);
      for (int c = 0; c < 3; ++c) { lo[c] = min(lo[c], k[c]); hi[c] = max(hi[c], k[c]); }
      ++cnt;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_xor(cnt, off, 64);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = min(lo[c], __shfl_xor(lo[c], off, 64));
      hi[c] = max(hi[c], __shfl_xor(hi[c], off, 64));
    }
  }
  if (lane == 0) {
    part[wave][0] = cnt;
    for (int c = 0; c < 3; ++c) { part[wave][1 + c] = lo[c]; part[wave][4 + c] = hi[c]; }
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int c = threadIdx.x;
    int t = part[0][c];
    for (int w = 1; w < kDplWaves; ++w) t = c == 0 ? t + part[w][c] : c < 4 ? min(t, part[w][c]) : max(t, part[w][c]);
    if (c == 0) { if (t) atomicAdd(&a.ctr[DP_ELIGIBLE], (u64)t); }
    else if (c < 4) { if (t != INT_MAX) atomicMin(&a.box[c - 1], t); }
    else if (t != INT_MIN) atomicMax(&a.box[c - 1], t);
  }
}

// step 2: centre and count of every entry of U_r.  The grid covers n; the list's length is read on the device.
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_pack(DplArgs a) {
  const long long j = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const long long n_r = (long long)min(a.ctr[DP_NR], (u64)a.n);
  if (j >= n_r) return;
  const int i = a.list[j];
  if (i < 0 || i >= a.n) return;
  int k[3];
  dense_unpack(a.skey[i], k);
  const unsigned int slot = a.sval[i];
  DplVox v;
  for (int c = 0; c < 3; ++c) v.x[c] = dobj_center(k[c], a.leaf);
  v.count = slot < a.H ? (long long)a.rec[slot].count : 0;
  a.vox[j] = v;
}

// step 3: the packed keys of the entries i_0, i_1, i_2 of every hypothesis (all ones with fewer than three entries)
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_gather(DplArgs a) {
  const int t = blockIdx.x * kDenseThreads + threadIdx.x;
  if (t >= 3 * a.n_hyp) return;
  const long long n_r = (long long)min(a.ctr[DP_NR], (u64)a.n);
  u64 key = kDenseEmpty;
  if (n_r >= 3) {
    const int i = a.list[dpl_index(a.seed, a.round, a.n_hyp, t / 3, t % 3, (int)n_r)];
    if (i >= 0 && i < a.n) key = a.skey[i];
  }
  a.gkeys[t] = key;
}

// step 4, the hot kernel.  Lane = hypothesis: its plane and its two sums stay in registers.  grid = (hypothesis groups, chunks of the
// list); a workgroup stages tile after tile of its chunk in LDS, and every lane reads every entry by broadcast.  Integer sums: the
// order of the chunks' atomics does not show.  An invalid hypothesis's lane runs along with a zero plane and adds nothing.  The host
// launches it for kDplSmall hypotheses or more only: below a wave most lanes would idle while every wave still walks every tile.
static __global__ __launch_bounds__(kDplGroup) void k_dpl_score(DplArgs a) {
  __shared__ DplVox tile[kDplTile];
  const int h = blockIdx.x * kDplGroup + threadIdx.x;
  const bool on = h < a.n_hyp && a.valid[h] != 0;
  double pl[4] = {0, 0, 0, 0};
  if (on) {
    for (int c = 0; c < 4; ++c) pl[c] = a.planes[(size_t)h * 4 + c];
  }
  unsigned int n_in = 0;
  u64 smp = 0;
  const int n_tiles = (a.n_r + kDplTile - 1) / kDplTile;
  for (int t = blockIdx.y; t < n_tiles; t += gridDim.y) {   // workgroup-uniform
    const int base = t * kDplTile, m = min(kDplTile, a.n_r - base);
    __syncthreads();   // the tile before this one has been read by every wave
    for (int j = threadIdx.x; j < m; j += kDplGroup) tile[j] = a.vox[base + j];
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < m; ++j) {
      const DplVox v = tile[j];
      const bool in = dpl_inlier(pl, v.x, a.dist_tol);
      n_in += in ? 1u : 0u;
      smp += in ? (u64)v.count : 0ull;
    }
  }
  if (on && n_in) {
    atomicAdd(&a.hacc[(size_t)h * 2], (u64)n_in);
    atomicAdd(&a.hacc[(size_t)h * 2 + 1], smp);
  }
}

// step 4 with fewer hypotheses than a wave (n_hyp < kDplSmall), where k_dpl_score's lanes would mostly idle: lane = voxel.  At most
// kDplReduceBlocks workgroups; hypothesis after hypothesis (workgroup-uniform) a lane strides over U_r with the two sums in registers,
// the wave folds them, the waves meet in LDS and one lane emits the workgroup's two atomics.  The list is read n_hyp times, from cache.
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_few(DplArgs a) {
  __shared__ u64 part[kDplWaves][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int h = 0; h < a.n_hyp; ++h) {
    if (!a.valid[h]) continue;
    double pl[4];
    for (int c = 0; c < 4; ++c) pl[c] = a.planes[(size_t)h * 4 + c];
    u64 n_in = 0, smp = 0;
    for (long long j = (long long)blockIdx.x * kDenseThreads + threadIdx.x; j < a.n_r; j += (long long)gridDim.x * kDenseThreads) {
      const DplVox e = a.vox[j];
      const bool in = dpl_inlier(pl, e.x, a.dist_tol);
      n_in += in ? 1ull : 0ull;
      smp += in ? (u64)e.count : 0ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { n_in += __shfl_xor(n_in, off, 64); smp += __shfl_xor(smp, off, 64); }
    if (lane == 0) { part[wave][0] = n_in; part[wave][1] = smp; }
    __syncthreads();
    if (threadIdx.x < 2) {
      u64 t = 0;
      for (int w = 0; w < kDplWaves; ++w) t += part[w][threadIdx.x];
      if (t) atomicAdd(&a.hacc[(size_t)h * 2 + threadIdx.x], t);
    }
    __syncthreads();   // part is free again
  }
}

// steps 6 and 7: one plane against U_r, a lane per entry and stride.  The inliers' n, samples, s and M relative to kmin (64-bit integer
// sums); with assign >= 0 the inliers take that plane.
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_one(DplArgs a) {
  __shared__ u64 part[kDplWaves][kDplMoments];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 v[kDplMoments];
  for (int c = 0; c < kDplMoments; ++c) v[c] = 0;
  for (long long j = (long long)blockIdx.x * kDenseThreads + threadIdx.x; j < a.n_r; j += (long long)gridDim.x * kDenseThreads) {
    const DplVox e = a.vox[j];
    const int i = a.list[j];
    if (!dpl_inlier(a.one, e.x, a.dist_tol) || i < 0 || i >= a.n) continue;
    int k[3];
    dense_unpack(a.skey[i], k);
    const long long d0 = (long long)k[0] - a.kmin[0], d1 = (long long)k[1] - a.kmin[1], d2 = (long long)k[2] - a.kmin[2];
    v[0] += 1; v[1] += (u64)e.count; v[2] += (u64)d0; v[3] += (u64)d1; v[4] += (u64)d2;
    v[5] += (u64)(d0 * d0); v[6] += (u64)(d0 * d1); v[7] += (u64)(d0 * d2); v[8] += (u64)(d1 * d1); v[9] += (u64)(d1 * d2); v[10] += (u64)(d2 * d2);
    if (a.assign >= 0) a.state[i] = a.assign;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < kDplMoments; ++c) v[c] += __shfl_xor(v[c], off, 64);
  }
  if (lane == 0) {
    for (int c = 0; c < kDplMoments; ++c) part[wave][c] = v[c];
  }
  __syncthreads();
  if (threadIdx.x < kDplMoments) {
    u64 t = 0;
    for (int w = 0; w < kDplWaves; ++w) t += part[w][threadIdx.x];
    if (t) atomicAdd(&a.mom[threadIdx.x], t);
  }
}

// step 8
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_vout(DplArgs a) {
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  if (i >= a.n_vout) return;
  a.vout[i] = a.state[i];
}

}  // namespace esl

using namespace esl;

extern "C" void esl_dense_plane_params_default(esl_dense_plane_params* p) {
  if (!p) return;
  p->dist_tol = 0.02; p->up[0] = p->up[1] = p->up[2] = 0; p->up_min_cos = 0.7071067811865476;
  p->n_hypotheses = 1024; p->max_planes = 8; p->min_inliers = 1000; p->min_baseline = 8; p->min_count = 1; p->skip_labelled = 0;
  p->refine = 1; p->pad = 0; p->seed = 0;
}

extern "C" int esl_debug_dense_planes_layout(int32_t* tile_out, int32_t* group_out) {
  if (!tile_out || !group_out) return dense_fail(ESL_ERR_INVALID, "esl_debug_dense_planes_layout", "null pointer");
  *tile_out = kDplTile; *group_out = kDplGroup;
  return ESL_OK;
}

// one launch of k_dpl_one and its eleven sums on the host (a host round trip)
static int dpl_one_pass(esl_ctx* c, DplArgs& a, const double pl[4], int assign, long long mom[kDplMoments]) {
  for (int e = 0; e < 4; ++e) a.one[e] = pl[e];
  a.assign = assign;
  ESL_HIP_TRY(hipMemsetAsync(a.mom, 0, kDplMoments * sizeof(u64), c->stream));
  {
    ProfScope ps(c, 4);
    hipLaunchKernelGGL(k_dpl_one, dim3(std::min<unsigned>(dense_blocks((u64)a.n_r), kDplReduceBlocks)), dim3(kDenseThreads), 0, c->stream, a);
  }
  ESL_HIP_TRY(hipGetLastError());
  ESL_HIP_TRY(hipMemcpyAsync(mom, a.mom, kDplMoments * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  return ESL_OK;
}

extern "C" int esl_dense_planes(esl_ctx* c, const esl_dense_plane_params* pp, double* planes_out, double* centroid_out, int32_t* stats_out,
                                int64_t* samples_out, double* ground_out, int64_t voxel_cap, int32_t* voxel_plane_out, int64_t* hyp_out,
                                esl_dense_plane_result* out) {
  const char* who = "esl_dense_planes";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (!out) return dense_fail(ESL_ERR_INVALID, who, "null out");
  if (!planes_out) return dense_fail(ESL_ERR_INVALID, who, "null planes_out");
  if (voxel_cap < 0) return dense_fail(ESL_ERR_INVALID, who, "negative voxel_cap");
  if (voxel_cap > 0 && !voxel_plane_out) return dense_fail(ESL_ERR_INVALID, who, "null voxel_plane_out with voxel_cap > 0");
  esl_dense_plane_params p;
  if (pp) p = *pp; else esl_dense_plane_params_default(&p);
  if (!std::isfinite(p.dist_tol) || !(p.dist_tol > 0)) return dense_fail(ESL_ERR_INVALID, who, "dist_tol not finite or <= 0");
  if (!dpl_up_valid(p.up)) return dense_fail(ESL_ERR_INVALID, who, "up not finite, or neither zero nor longer than 1e-12");
  if (!(p.up_min_cos >= 0 && p.up_min_cos <= 1)) return dense_fail(ESL_ERR_INVALID, who, "up_min_cos outside 0 .. 1");
  if (p.n_hypotheses < 1 || p.n_hypotheses > 65536) return dense_fail(ESL_ERR_INVALID, who, "n_hypotheses outside 1 .. 65536");
  if (p.max_planes < 1 || p.max_planes > 64) return dense_fail(ESL_ERR_INVALID, who, "max_planes outside 1 .. 64");
  if (p.min_inliers < 3) return dense_fail(ESL_ERR_INVALID, who, "min_inliers < 3");
  if (p.min_baseline < 1) return dense_fail(ESL_ERR_INVALID, who, "min_baseline < 1");
  if ((long long)p.max_planes * p.n_hypotheses >= (1ll << 31)) return dense_fail(ESL_ERR_INVALID, who, "max_planes n_hypotheses reaches 2^31");
  if (!dense_begun(c, who)) return ESL_ERR_STATE;
  DenseState& d = *c->dense;
  std::memset(out, 0, sizeof(*out));
  if (dense_map_invalid(d, out)) return ESL_OK;   // nothing is written
  const long long n = d.n_voxels, n_vox_w = std::min<long long>(n, voxel_cap);
  const int Hn = p.n_hypotheses, P = p.max_planes;
  out->n_voxels = (int32_t)n; out->ground_index = -1; out->stop_reason = 1;
  for (int i = 0; i < P * 4; ++i) planes_out[i] = 0;
  if (centroid_out) for (int i = 0; i < P * 3; ++i) centroid_out[i] = 0;
  if (stats_out) for (int i = 0; i < P * 8; ++i) stats_out[i] = 0;
  if (samples_out) for (int i = 0; i < P; ++i) samples_out[i] = 0;
  if (ground_out) for (int i = 0; i < 4; ++i) ground_out[i] = 0;
  if (hyp_out) std::memset(hyp_out, 0, (size_t)P * Hn * 3 * sizeof(int64_t));
  if (n == 0) return ESL_OK;   // step 2 with n_0 = 0

  ESL_HIP_TRY(hipSetDevice(c->device));
  ScratchSet<DB_PL_COUNT>& s = d.pl_set;
  DenseList L;
  size_t sel_bytes = 0;
  if (const int rc = dense_list_begin(c, d, L)) return rc;
  const DenseOutArgs& k = L.k;
  {
    const size_t sn = (size_t)n, sh = (size_t)Hn;
    const DenseSlot want[] = {{DB_PSTATE, sn * 4}, {DB_PCTR, DP_COUNT * sizeof(u64)}, {DB_PBOX, 6 * 4}, {DB_PLIST, sn * 4},
                              {DB_PVOX, sn * sizeof(DplVox)}, {DB_PGKEY, sh * 3 * 8}, {DB_PPLANES, sh * 4 * 8}, {DB_PVALID, sh * 4},
                              {DB_PHACC, sh * 2 * 8}, {DB_PMOM, kDplMoments * sizeof(u64)}, {DB_PVOUT, (size_t)n_vox_w * 4}};
    if (const int rc = dense_grow(c, s, want, false)) return rc;
  }
  DplArgs a;
  std::memset(&a, 0, sizeof(a));
  a.rec = k.rec; a.H = k.H; a.skey = k.skey; a.sval = k.sval; a.n = (int)n;
  a.state = s.at<int>(DB_PSTATE); a.min_count = p.min_count; a.skip_labelled = p.skip_labelled != 0;
  a.ctr = s.at<u64>(DB_PCTR); a.box = s.at<int>(DB_PBOX);
  a.list = s.at<int>(DB_PLIST); a.vox = s.at<DplVox>(DB_PVOX);
  a.gkeys = s.at<u64>(DB_PGKEY); a.n_hyp = Hn; a.seed = p.seed;
  a.planes = s.at<double>(DB_PPLANES); a.valid = s.at<int>(DB_PVALID); a.hacc = s.at<u64>(DB_PHACC);
  a.leaf = d.p.leaf; a.dist_tol = p.dist_tol; a.mom = s.at<u64>(DB_PMOM);
  a.vout = s.at<int>(DB_PVOUT); a.n_vout = n_vox_w;
  if (const int rc = dense_select_free(c, nullptr, sel_bytes, a.state, s.at<int>(DB_PLIST), a.ctr + DP_NR, (size_t)n)) return rc;
  if (const int rc = s.grow(c, DB_PSELTMP, sel_bytes)) return rc;
  const dim3 blk(kDenseThreads), grid_n(dense_blocks((u64)n));

  // step 1
  int box[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
  u64 ctr[DP_COUNT];
  ESL_HIP_TRY(hipMemsetAsync(a.ctr, 0, DP_COUNT * sizeof(u64), c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(a.box, box, sizeof(box), hipMemcpyHostToDevice, c->stream));
  {
    ProfScope ps(c, 4);
    if (const int rc = dense_list_launch(c, d, L, d.with_inst && a.skip_labelled, false)) return rc;
    hipLaunchKernelGGL(k_dpl_gate, dim3(std::min<unsigned>(dense_blocks((u64)n), kDplReduceBlocks)), blk, 0, c->stream, a);
  }
  ESL_HIP_TRY(hipGetLastError());
  ESL_HIP_TRY(hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(box, a.box, sizeof(box), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  out->n_eligible = (int32_t)ctr[DP_ELIGIBLE];
  long long span = 1;
  if (ctr[DP_ELIGIBLE] > 0) {
    for (int e = 0; e < 3; ++e) { span = std::max<long long>(span, (long long)box[3 + e] - box[e] + 1); a.kmin[e] = box[e]; }
  }

  std::vector<u64> gkeys((size_t)Hn * 3), hacc((size_t)Hn * 2);
  std::vector<double> planes((size_t)Hn * 4);
  std::vector<int> valid((size_t)Hn);
  std::vector<int32_t> plane_in;   // the reported planes' inlier voxels (the ground choice)
  const unsigned groups = (unsigned)((Hn + kDplGroup - 1) / kDplGroup);
  int stop = 0;
  for (int r = 0; r < P; ++r) {
    // step 2: U_r, its entries' centres and counts, and the keys of the hypotheses' entries
    a.round = r;
    {
      ProfScope ps(c, 4);
      if (const int rc = dense_select_free(c, s.buf[DB_PSELTMP], sel_bytes, a.state, s.at<int>(DB_PLIST), a.ctr + DP_NR, (size_t)n)) return rc;
      hipLaunchKernelGGL(k_dpl_pack, grid_n, blk, 0, c->stream, a);
      hipLaunchKernelGGL(k_dpl_gather, dim3(dense_blocks((u64)Hn * 3)), blk, 0, c->stream, a);
    }
    ESL_HIP_TRY(hipGetLastError());
    ESL_HIP_TRY(hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(gkeys.data(), a.gkeys, gkeys.size() * 8, hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    const long long n_r = (long long)std::min<u64>(ctr[DP_NR], (u64)n);
    if (n_r < 3) { stop = 1; break; }
    a.n_r = (int)n_r;
    out->rounds = r + 1;
    // step 3 on the host
    int n_valid = 0;
    for (int h = 0; h < Hn; ++h) {
      int idx[3], key[3][3];
      for (int e = 0; e < 3; ++e) { idx[e] = dpl_index(p.seed, r, Hn, h, e, (int)n_r); dense_unpack(gkeys[(size_t)h * 3 + e], key[e]); }
      valid[(size_t)h] = dpl_hypothesis(idx, key[0], key[1], key[2], p.min_baseline, d.p.leaf, planes.data() + (size_t)h * 4) ? 1 : 0;
      n_valid += valid[(size_t)h];
    }
    if (n_valid == 0) { stop = 2; break; }   // the round's rows of hyp_out stay zero
    // step 4
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[DB_PPLANES], planes.data(), planes.size() * 8, hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[DB_PVALID], valid.data(), valid.size() * 4, hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemsetAsync(a.hacc, 0, hacc.size() * 8, c->stream));
    {
      ProfScope ps(c, 4);
      if (Hn < kDplSmall) {   // fewer hypotheses than a wave: lane = voxel
        hipLaunchKernelGGL(k_dpl_few, dim3(std::min<unsigned>(dense_blocks((u64)n_r), kDplReduceBlocks)), blk, 0, c->stream, a);
      } else {
        const unsigned n_tiles = (unsigned)((n_r + kDplTile - 1) / kDplTile);
        const unsigned chunks = std::min(n_tiles, std::min<unsigned>(kDplMaxChunks, std::max(1u, 1024u / groups)));
        hipLaunchKernelGGL(k_dpl_score, dim3(groups, chunks), dim3(kDplGroup), 0, c->stream, a);
      }
    }
    ESL_HIP_TRY(hipGetLastError());
    ESL_HIP_TRY(hipMemcpyAsync(hacc.data(), a.hacc, hacc.size() * 8, hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    // step 5
    const int win = dpl_winner(valid.data(), hacc.data(), Hn, hyp_out ? hyp_out + (size_t)r * Hn * 3 : nullptr);   // n_valid > 0: one wins
    const long long win_n = (long long)hacc[(size_t)win * 2], win_s = (long long)hacc[(size_t)win * 2 + 1];
    double fin[4];
    for (int e = 0; e < 4; ++e) fin[e] = planes[(size_t)win * 4 + e];
    long long fin_n = win_n;
    long long mom[kDplMoments];
    // step 6
    int refined = 0;
    if (p.refine) {
      if (dobj_guard(win_n, span)) refined = 3;
      else {
        if (const int rc = dpl_one_pass(c, a, fin, -1, mom)) return rc;
        double re[4];
        dpl_refit(mom, a.kmin, d.p.leaf, re);
        if (const int rc = dpl_one_pass(c, a, re, -1, mom)) return rc;
        if (dpl_refit_kept(mom[0], mom[1], win_n, win_s)) {
          refined = 1; fin_n = mom[0];
          for (int e = 0; e < 4; ++e) fin[e] = re[e];
        } else {
          refined = 2;
        }
      }
    }
    // step 7
    if (fin_n < p.min_inliers) { stop = 3; break; }
    if (const int rc = dpl_one_pass(c, a, fin, r, mom)) return rc;
    const int q = out->n_planes;   // = r
    double* po = planes_out + 4 * q;
    for (int e = 0; e < 4; ++e) po[e] = fin[e];
    dpl_orient_out(po);
    if (centroid_out) dpl_centroid(mom, a.kmin, d.p.leaf, centroid_out + 3 * q);
    if (stats_out) {
      int32_t* so = stats_out + 8 * q;
      so[0] = (int32_t)mom[0]; so[1] = (int32_t)n_r; so[2] = n_valid; so[3] = win; so[4] = (int32_t)win_n; so[5] = refined; so[6] = 0; so[7] = 0;
    }
    if (samples_out) samples_out[q] = mom[1];
    plane_in.push_back((int32_t)mom[0]);
    out->n_planes = q + 1; out->n_assigned += (int32_t)mom[0];
  }
  out->stop_reason = stop;
  // step 8: every voxel's plane
  if (n_vox_w > 0) {
    {
      ProfScope ps(c, 4);
      hipLaunchKernelGGL(k_dpl_vout, dim3(dense_blocks((u64)n_vox_w)), blk, 0, c->stream, a);
    }
    ESL_HIP_TRY(hipGetLastError());
    ESL_HIP_TRY(hipMemcpyAsync(voxel_plane_out, a.vout, (size_t)n_vox_w * 4, hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  }
  // step 9
  double uh[3], ground[4];
  if (dpl_up(p.up, uh)) {
    out->ground_index = dpl_ground(planes_out, plane_in.data(), out->n_planes, uh, p.up_min_cos, ground);
    if (ground_out) for (int e = 0; e < 4; ++e) ground_out[e] = ground[e];
  }
  return ESL_OK;
}
