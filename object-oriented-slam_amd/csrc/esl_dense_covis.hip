// esl_dense_covis.hip — esl_dense_covis_frames (include/esl.h, "covisibility of the dense map"; the steps' numbers below are the
// header's; the arithmetic: esl_dense_covis.hpp and, for step V2, esl_dense_carve.hpp's dcv_observe itself).  It works on the dense
// map's sorted list (esl_dense_int.hpp, whose rule on stores and bounded loops holds here): the list and extract's gather of xyz into
// this unit's buffers, then
//   k_dco_observe   one lane per voxel; grid.y runs over chunks of kDcoChunk frames, so a workgroup's frame is uniform and its R, t and
//                   K are scalar loads.  Step V2 per lane and frame; __ballot(agree) IS the 64-bit word of the wave's 64 voxels in the
//                   frame's row of the bit matrix (bits[f W + word], W = ceil(n / 64)): lane 0 stores it, one writer per word, the tail
//                   bits zero because a lane beyond n has no class, so the matrix needs no memset.  The lane's k over the chunk as ONE
//                   int32 atomicAdd per lane and chunk; the frame's four counts by ballot + popcount, one atomic per wave and count.
//   k_dco_pairs     the bit product B B^T (step V4).  A workgroup takes one kDcoTile x kDcoTile tile of frame pairs of the upper
//                   triangle of tiles and slabs of kDcoSlab words; the tile's two row blocks of a slab are staged in LDS at a row pitch of
//                   kDcoSlab + 1 words (a pitch of kDcoSlab words = 512 bytes is a multiple of the 256-byte bank span: every row would
//                   start in one bank).  16 x 16 threads, a 2 x 2 block of pairs per thread in registers: four 8-byte LDS reads feed
//                   four AND + popcount per word.  The partial counts reach pair[a][b] and, off the diagonal tiles, pair[b][a] as int32
//                   atomicAdd: an integer sum in any order.
//   k_dco_mask      one lane per voxel: cov[word] = ballot(k - 1 >= min_others), uni[word] = ballot(k == 1); n_seen and
//                   sum k (k - 1) / 2 by ballot / wave sum, one atomic per wave.
//   k_dco_cover     grid.y over the frames, a lane per word of the row: popc(bits[f] & cov), in round 0 popc(bits[f] & uni) too, summed
//                   over the wave by shuffles, one int32 atomic per wave.  A culled frame's row is skipped.
//   k_dco_drop      a cull round: one lane per voxel; where the culled frame's bit is set k -= 1 by a plain store (the lane owns the
//                   voxel), then cov[word] re-balloted; thread 0 clears the frame's alive flag.
// The pick of step V6 is host code on F int32 read back per round.  No atomic's value is read, no loop waits for another thread, every
// loop's bound stands beside it.
#include "esl_dense_int.hpp"
#include "esl_dense_covis.hpp"
#include "esl_dense_check.hpp"

namespace esl {

// the call's buffers (DenseState::co_set)
enum { DO_XYZ, DO_K, DO_POSE, DO_DEPTH, DO_FCTR, DO_BITS, DO_PAIR, DO_COV, DO_UNI, DO_CVR, DO_ALIVE, DO_CTR, DO_COUNT };
static_assert(DO_COUNT == kDcoBufs, "esl_dense_int.hpp sizes DenseState::co_set");
enum { DOC_SEEN, DOC_PAIRS, DOC_COUNT };                                                                    // the device counters
enum { DOF_IN_VIEW, DOF_DEPTH_OUT, DOF_OUTSIDE, DOF_SEEN, DOF_COVERED, DOF_UNIQUE, DOF_ROUND, DOF_PAD, DOF_COUNT };   // frame_out's row

constexpr int kDcoPitch = kDcoSlab + 1;                 // the LDS row pitch in words
constexpr int kDcoSide = 16;                            // threads along each edge of the tile
static_assert(kDcoSide * kDcoSide == kDenseThreads && kDcoSide * 2 == kDcoTile, "a 2 x 2 block of pairs per thread");
constexpr int kDcoMaxSlabBlocks = 1024;                 // grid.y of k_dco_pairs at most: a workgroup strides over the slabs
static_assert(kDcoChunk >= 1 && kDcoSlab >= 1, "");

struct DcoArgs {
  const double* xyz; int n; long long W;
  const double* pose; int F, n_chunks;
  const unsigned short* depth;
  double K[4]; int rows, cols;
  double depth_scale, depth_min, depth_max, depth_tol;
  int window, min_others;
  int* kcount; int* fctr; u64* bits; u64* cov; u64* uni; int* cvr; int* alive; u64* ctr;
  int* pair; int T; long long n_slabs;
  int round0, culled;
};

// steps V2 and V3.  grid = (blocks over the voxels, chunks of frames: at most kDcoMaxFrames / kDcoChunk, a workgroup takes blockIdx.y, + gridDim.y, ...)
static __global__ __launch_bounds__(kDenseThreads) void k_dco_observe(DcoArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const long long word = i >> 6;   // wave-uniform: the wave's 64 voxels are the word's 64 bits
  const bool in = i < a.n;
  double p[3] = {0, 0, 0};
  if (in) {
    for (int c = 0; c < 3; ++c) p[c] = a.xyz[i * 3 + c];
  }
  const size_t npix = (size_t)a.rows * a.cols;
  for (int ch = blockIdx.y; ch < a.n_chunks; ch += gridDim.y) {   // at most n_chunks rounds; workgroup-uniform
    const int f0 = ch * kDcoChunk, f1 = f0 + kDcoChunk < a.F ? f0 + kDcoChunk : a.F;
    int k = 0;   // the frames of the chunk that see this lane's voxel: at most kDcoChunk
    for (int f = f0; f < f1; ++f) {   // at most kDcoChunk frames; workgroup-uniform
      int cls = -1;
      if (in) cls = dcv_observe(a.pose + (size_t)f * kDensePose, a.K, p, a.depth + (size_t)f * npix, a.rows, a.cols, a.window, a.depth_scale,
                                a.depth_min, a.depth_max, a.depth_tol);
      const u64 m_s = __ballot(cls == DCV_AGREE), m_z = __ballot(cls == DCV_DEPTH_OUT), m_o = __ballot(cls == DCV_OUTSIDE),
                m_v = __ballot(cls >= 0 && cls <= DCV_NODATA);
      if (cls == DCV_AGREE) ++k;
      if (lane == 0) {
        if (word < a.W) a.bits[(size_t)f * (size_t)a.W + (size_t)word] = m_s;   // the word's one writer
        int* fc = a.fctr + (size_t)f * DOF_COUNT;
        if (m_v) atomicAdd(&fc[DOF_IN_VIEW], __popcll(m_v));
        if (m_z) atomicAdd(&fc[DOF_DEPTH_OUT], __popcll(m_z));
        if (m_o) atomicAdd(&fc[DOF_OUTSIDE], __popcll(m_o));
        if (m_s) atomicAdd(&fc[DOF_SEEN], __popcll(m_s));
      }
    }
    if (k) atomicAdd(&a.kcount[i], k);   // k != 0 only with i < n
  }
}

// step V4.  grid = (tiles of the upper triangle: T (T + 1) / 2, slab blocks: at most kDcoMaxSlabBlocks, a workgroup takes blockIdx.y, + gridDim.y, ...)
static __global__ __launch_bounds__(kDenseThreads) void k_dco_pairs(DcoArgs a) {
  __shared__ u64 sA[kDcoTile * kDcoPitch], sB[kDcoTile * kDcoPitch];
  int ta = 0, rem = (int)blockIdx.x;
  for (int it = 0; it < a.T && rem >= a.T - ta; ++it) { rem -= a.T - ta; ++ta; }   // at most T rounds: the tile row of this index
  const int tb = ta + rem;   // ta <= tb < T
  const int fa0 = ta * kDcoTile, fb0 = tb * kDcoTile;
  const int ty = threadIdx.x / kDcoSide, tx = threadIdx.x % kDcoSide;   // rows 2 ty, 2 ty + 1 of the a block; 2 tx, 2 tx + 1 of the b block
  int acc[2][2] = {{0, 0}, {0, 0}};   // at most 64 n_slab_rounds kDcoSlab <= 64 W: n < 2^31 bits in all
  const size_t W = (size_t)a.W;
  for (long long sl = blockIdx.y; sl < a.n_slabs; sl += gridDim.y) {   // at most n_slabs rounds; workgroup-uniform
    const long long w0 = sl * kDcoSlab;
    for (int idx = threadIdx.x; idx < kDcoTile * kDcoSlab; idx += kDenseThreads) {   // kDcoTile kDcoSlab / kDenseThreads rounds
      const int r = idx / kDcoSlab, w = idx % kDcoSlab;
      const bool wi = w0 + w < a.W;
      sA[r * kDcoPitch + w] = wi && fa0 + r < a.F ? a.bits[(size_t)(fa0 + r) * W + (size_t)(w0 + w)] : 0ull;
      sB[r * kDcoPitch + w] = wi && fb0 + r < a.F ? a.bits[(size_t)(fb0 + r) * W + (size_t)(w0 + w)] : 0ull;
    }
    __syncthreads();
    const u64* ra = sA + (2 * ty) * kDcoPitch;
    const u64* rb = sB + (2 * tx) * kDcoPitch;
#pragma unroll 8
    for (int w = 0; w < kDcoSlab; ++w) {   // kDcoSlab words
      const u64 a0 = ra[w], a1 = ra[kDcoPitch + w], b0 = rb[w], b1 = rb[kDcoPitch + w];
      acc[0][0] += __popcll(a0 & b0); acc[0][1] += __popcll(a0 & b1);
      acc[1][0] += __popcll(a1 & b0); acc[1][1] += __popcll(a1 & b1);
    }
    __syncthreads();   // the next slab overwrites the rows
  }
#pragma unroll
  for (int y = 0; y < 2; ++y) {
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      const int fa = fa0 + 2 * ty + y, fb = fb0 + 2 * tx + x;
      if (fa < a.F && fb < a.F && acc[y][x]) {
        atomicAdd(&a.pair[(size_t)fa * a.F + fb], acc[y][x]);
        if (ta != tb) atomicAdd(&a.pair[(size_t)fb * a.F + fa], acc[y][x]);   // a diagonal tile holds both cells itself
      }
    }
  }
}

// steps V3 and V5: the two masks of round 0.  grid = blocks over the voxels
static __global__ __launch_bounds__(kDenseThreads) void k_dco_mask(DcoArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const long long word = i >> 6;
  const int k = i < a.n ? a.kcount[i] : 0;
  const u64 m_c = __ballot(k - 1 >= a.min_others), m_u = __ballot(k == 1), m_s = __ballot(k >= 1);
  u64 pairs = (u64)k * (u64)(k > 0 ? k - 1 : 0) / 2;   // k <= 4096
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pairs += __shfl_down(pairs, off, 64);   // 6 steps
  if (lane == 0) {
    if (word < a.W) { a.cov[word] = m_c; a.uni[word] = m_u; }
    if (m_s) atomicAdd(&a.ctr[DOC_SEEN], (u64)__popcll(m_s));
    if (pairs) atomicAdd(&a.ctr[DOC_PAIRS], pairs);
  }
}

// step V5 per alive frame.  grid = (blocks over the words of a row, frames: at most kDcoMaxFrames, a workgroup takes blockIdx.y, + gridDim.y, ...)
static __global__ __launch_bounds__(kDenseThreads) void k_dco_cover(DcoArgs a) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const bool in = w < a.W;
  const u64 cov = in ? a.cov[w] : 0ull, uni = in && a.round0 ? a.uni[w] : 0ull;
  for (int f = blockIdx.y; f < a.F; f += gridDim.y) {   // at most F rounds; workgroup-uniform
    if (!a.alive[f]) continue;   // workgroup-uniform
    const u64 b = in ? a.bits[(size_t)f * (size_t)a.W + (size_t)w] : 0ull;
    int c = __popcll(b & cov), u = __popcll(b & uni);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { c += __shfl_down(c, off, 64); u += __shfl_down(u, off, 64); }   // 6 steps
    if (lane == 0) {
      if (a.round0) {
        if (c) atomicAdd(&a.fctr[(size_t)f * DOF_COUNT + DOF_COVERED], c);
        if (u) atomicAdd(&a.fctr[(size_t)f * DOF_COUNT + DOF_UNIQUE], u);
      } else if (c) {
        atomicAdd(&a.cvr[f], c);
      }
    }
  }
}

// step V6: frame `culled` leaves.  grid = blocks over the voxels
static __global__ __launch_bounds__(kDenseThreads) void k_dco_drop(DcoArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const long long word = i >> 6;
  int k = 0;
  if (i < a.n) {   // then word < W
    const u64 b = a.bits[(size_t)a.culled * (size_t)a.W + (size_t)word];
    k = a.kcount[i];
    if ((b >> lane) & 1ull) { k -= 1; a.kcount[i] = k; }   // only this lane writes this voxel
  }
  const u64 m_c = __ballot(k - 1 >= a.min_others);
  if (lane == 0 && word < a.W) a.cov[word] = m_c;
  if (i == 0) a.alive[a.culled] = 0;
}

}  // namespace esl

using namespace esl;

extern "C" void esl_dense_covis_params_default(esl_dense_covis_params* p) {
  if (!p) return;
  p->depth_scale = 5000.0; p->depth_min = 0.1; p->depth_max = 6.0; p->depth_tol = 0.05;
  p->window = 1; p->min_others = 3; p->cover_num = 9; p->cover_den = 10; p->max_cull = 0; p->reserved = 0;
}

extern "C" int esl_dense_covis_frames(esl_ctx* c, const double* cams, int32_t F, const uint16_t* depth, const uint8_t* keep_in, const double K[4],
                                      int32_t rows, int32_t cols, const esl_dense_covis_params* pp, int64_t vox_cap, int32_t* vox_out,
                                      int32_t* frame_out, int32_t* pair_out, esl_dense_covis_result* out) {
  const char* who = "esl_dense_covis_frames";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (!out) return dense_fail(ESL_ERR_INVALID, who, "null out");
  if (F < 0) return dense_fail(ESL_ERR_INVALID, who, "negative F");
  if (const char* m = dense_image_check(K, rows, cols)) return dense_fail(ESL_ERR_INVALID, who, m);
  if (vox_cap < 0) return dense_fail(ESL_ERR_INVALID, who, "negative vox_cap");
  esl_dense_covis_params p;
  if (pp) p = *pp; else esl_dense_covis_params_default(&p);
  if (const char* m = dco_params_check(p)) return dense_fail(ESL_ERR_INVALID, who, m);
  if (F > kDcoMaxFrames) return dense_fail(ESL_ERR_INVALID, who, "F > 4096");
  if (F > 0 && !depth) return dense_fail(ESL_ERR_INVALID, who, "null depth");
  if (!dense_begun(c, who)) return ESL_ERR_STATE;
  DenseState& d = *c->dense;
  if (const int rc = resident_source_check(c, who, !cams && F > 0, F, false, 0)) return rc;
  std::memset(out, 0, sizeof(*out));
  if (dense_map_invalid(d, out)) return ESL_OK;   // step V7
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (F > 0) {   // the poses: R and t of every frame on the host, before anything runs
    if (const int rc = dense_frames_poses(c, who, cams, F, d.cams, d.pose)) return rc;
  }

  const long long n = d.n_voxels, n_vw = vox_out ? std::min<long long>(n, vox_cap) : 0;
  const long long W = (n + 63) / 64;
  const size_t npix = (size_t)rows * cols, n_depth = (size_t)F * npix, sF = (size_t)F;
  out->n_voxels = (int32_t)n;
  ScratchSet<DO_COUNT>& s = d.co_set;
  DenseList L;
  DenseOutArgs& k = L.k;
  if (n > 0) {
    if (const int rc = dense_list_begin(c, d, L)) return rc;
  }
  {
    const size_t sn = (size_t)n, sW = (size_t)W;
    const DenseSlot want[] = {{DO_XYZ, sn * 3 * sizeof(double)}, {DO_K, sn * sizeof(int32_t)}, {DO_POSE, sF * kDensePose * sizeof(double)},
                              {DO_DEPTH, n_depth * sizeof(uint16_t)}, {DO_FCTR, sF * DOF_COUNT * sizeof(int32_t)},
                              {DO_BITS, sF * sW * sizeof(u64)}, {DO_PAIR, pair_out ? sF * sF * sizeof(int32_t) : 0},
                              {DO_COV, sW * sizeof(u64)}, {DO_UNI, sW * sizeof(u64)}, {DO_CVR, sF * sizeof(int32_t)},
                              {DO_ALIVE, sF * sizeof(int32_t)}, {DO_CTR, DOC_COUNT * sizeof(u64)}};
    if (const int rc = dense_grow(c, s, want, true)) return rc;
  }
  DcoArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = (int)n; a.W = W; a.F = F; a.n_chunks = (F + kDcoChunk - 1) / kDcoChunk;
  a.rows = rows; a.cols = cols;
  for (int i = 0; i < 4; ++i) a.K[i] = K[i];
  a.depth_scale = p.depth_scale; a.depth_min = p.depth_min; a.depth_max = p.depth_max; a.depth_tol = p.depth_tol;
  a.window = p.window; a.min_others = p.min_others;
  a.xyz = s.at<double>(DO_XYZ); a.kcount = s.at<int>(DO_K); a.fctr = s.at<int>(DO_FCTR); a.bits = s.at<u64>(DO_BITS);
  a.cov = s.at<u64>(DO_COV); a.uni = s.at<u64>(DO_UNI); a.cvr = s.at<int>(DO_CVR); a.alive = s.at<int>(DO_ALIVE); a.ctr = s.at<u64>(DO_CTR);
  a.T = (F + kDcoTile - 1) / kDcoTile; a.n_slabs = (W + kDcoSlab - 1) / kDcoSlab;
  a.round0 = 1; a.culled = 0;
  if (pair_out) a.pair = s.at<int>(DO_PAIR);
  const dim3 blk(kDenseThreads);
  const bool run = n > 0 && F > 0;   // without voxels or frames every count is 0
  const unsigned cover_y = (unsigned)std::min(F, 65535);

  ESL_HIP_TRY(hipMemsetAsync(a.ctr, 0, DOC_COUNT * sizeof(u64), c->stream));
  if (F > 0) {
    if (const int rc = upload(c, s, DO_POSE, (const double*)d.pose.data(), sF * kDensePose * sizeof(double), &a.pose)) return rc;
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[DO_DEPTH], depth, n_depth * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    a.depth = s.at<unsigned short>(DO_DEPTH);
    ESL_HIP_TRY(hipMemsetAsync(a.fctr, 0, sF * DOF_COUNT * sizeof(int32_t), c->stream));
    ESL_HIP_TRY(hipMemsetAsync(a.alive, 1, sF * sizeof(int32_t), c->stream));   // any non-zero word is alive
    if (a.pair) ESL_HIP_TRY(hipMemsetAsync(a.pair, 0, sF * sF * sizeof(int32_t), c->stream));
  }
  if (n > 0) {   // steps V1 to V5
    k.oxyz = s.at<double>(DO_XYZ);
    k.n_write = n; k.with_color = d.with_color;
    ESL_HIP_TRY(hipMemsetAsync(a.kcount, 0, (size_t)n * sizeof(int32_t), c->stream));
    {
      ProfScope ps(c, 4);
      if (const int rc = dense_list_launch(c, d, L, false, true)) return rc;
      if (F > 0) {
        hipLaunchKernelGGL(k_dco_observe, dim3(dense_blocks((u64)n), (unsigned)a.n_chunks), blk, 0, c->stream, a);
        if (a.pair) hipLaunchKernelGGL(k_dco_pairs, dim3((unsigned)(a.T * (a.T + 1) / 2), (unsigned)std::min<long long>(a.n_slabs, kDcoMaxSlabBlocks)),
                                       blk, 0, c->stream, a);
        hipLaunchKernelGGL(k_dco_mask, dim3(dense_blocks((u64)n)), blk, 0, c->stream, a);
        hipLaunchKernelGGL(k_dco_cover, dim3(dense_blocks((u64)W), cover_y), blk, 0, c->stream, a);
      }
    }
    ESL_HIP_TRY(hipGetLastError());
  }
  // the outputs of round 0
  std::vector<int32_t> fc(sF * DOF_COUNT, 0), cvr(sF, 0);
  if (n_vw > 0) ESL_HIP_TRY(hipMemcpyAsync(vox_out, a.kcount, (size_t)n_vw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (F > 0) ESL_HIP_TRY(hipMemcpyAsync(fc.data(), a.fctr, sF * DOF_COUNT * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (F > 0 && pair_out) ESL_HIP_TRY(hipMemcpyAsync(pair_out, a.pair, sF * sF * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  u64 ctr[DOC_COUNT];
  ESL_HIP_TRY(hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's arrays are free again, round 0's outputs filled
  out->n_seen = (int32_t)ctr[DOC_SEEN]; out->sum_pairs = (int64_t)ctr[DOC_PAIRS];
  for (int f = 0; f < F; ++f) {
    out->sum_seen += fc[(size_t)f * DOF_COUNT + DOF_SEEN];
    fc[(size_t)f * DOF_COUNT + DOF_ROUND] = -1;
    cvr[(size_t)f] = fc[(size_t)f * DOF_COUNT + DOF_COVERED];
  }
  // step V6: the pick on the host, the counts on the device
  std::vector<unsigned char> alive(sF, 1);
  const int rounds = std::min(p.max_cull, F);   // a round culls a frame: at most F of them do anything
  for (int r = 0; r < rounds; ++r) {   // at most min(max_cull, F) rounds
    int best = -1, best_unc = 0;
    for (int f = 0; f < F; ++f) {   // F frames
      if (!alive[(size_t)f] || (keep_in && keep_in[f])) continue;
      const int seen = fc[(size_t)f * DOF_COUNT + DOF_SEEN], cov = cvr[(size_t)f];
      if (!dco_redundant(seen, cov, p.cover_num, p.cover_den)) continue;
      if (best < 0 || dco_before(seen - cov, f, best_unc, best)) { best = f; best_unc = seen - cov; }
    }
    if (best < 0) break;
    alive[(size_t)best] = 0;
    fc[(size_t)best * DOF_COUNT + DOF_ROUND] = r;
    out->n_culled = r + 1;
    if (r + 1 == rounds || !run) continue;   // no round follows (or the frame saw nothing): the counts are not needed
    a.round0 = 0; a.culled = best;
    ESL_HIP_TRY(hipMemsetAsync(a.cvr, 0, sF * sizeof(int32_t), c->stream));
    {
      ProfScope ps(c, 4);
      hipLaunchKernelGGL(k_dco_drop, dim3(dense_blocks((u64)n)), blk, 0, c->stream, a);
      hipLaunchKernelGGL(k_dco_cover, dim3(dense_blocks((u64)W), cover_y), blk, 0, c->stream, a);
    }
    ESL_HIP_TRY(hipGetLastError());
    ESL_HIP_TRY(hipMemcpyAsync(cvr.data(), a.cvr, sF * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  }
  if (frame_out && F > 0) std::memcpy(frame_out, fc.data(), sF * DOF_COUNT * sizeof(int32_t));
  return ESL_OK;
}
