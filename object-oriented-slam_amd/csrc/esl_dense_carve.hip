// esl_dense_carve.hip — esl_dense_carve_frames (include/esl.h, "carving the dense map"; the steps' numbers below are the header's; the
// arithmetic: esl_dense_carve.hpp).  It works on the dense map's sorted list (esl_dense_int.hpp, whose rule on stores and bounded loops
// holds here): the list and extract's gather of xyz into this unit's buffers, then
//   k_dcv_observe   one lane per voxel; grid.y runs over chunks of kDcvChunk observer frames, so a workgroup's frame is uniform and its
//                   R, t and K are scalar loads.  Step C2 per lane and frame; the lane's four counts of a chunk stay in registers as four
//                   16-bit fields of one word and reach the voxel's accumulator as ONE 64-bit integer atomicAdd per lane and chunk (the
//                   fields sum to at most F_obs <= 65535: no carry).  The frame's seven counts by ballot + popcount, one atomic per
//                   wave and count.
//   k_dcv_verdict   one lane per voxel: the accumulator unpacked, step C4, vox_out / carved_out for the first vox_cap voxels, the
//                   verdict as a byte at the voxel's table slot (through the sorted list's slot values), n_carved and n_tested by
//                   ballot + popcount.
//   k_dcv_mark      one lane per sampled pixel of an owner frame, the frame uniform per workgroup.  The sample by k_dense_insert's
//                   header functions (dense_sample_pixel, steps 1 to 3 as in dense_sample_key), dense_lookup (nothing is claimed), a live count, the
//                   slot's byte.  Only a carved pixel is written: 0 into the kept image (which starts as a device copy of depth_own), the
//                   raw value into the cleared carved-depth image, 1 into the cleared mask.  The frame's four counts by ballot +
//                   popcount.
// No atomic's value is read, no loop waits for another thread, every loop's bound stands beside it.
// Step C6 goes through esl_dense_remove_frames itself from a host copy of the carved-depth images: k_dense_insert and k_dense_audit are
// the removal's kernels as they are.  The copy costs 2 bytes per owner pixel down and, inside the removal, 2 up again.
#include "esl_dense_int.hpp"
#include "esl_dense_carve.hpp"
#include "esl_dense_check.hpp"

namespace esl {

// the call's buffers (DenseState::cv_set)
enum { DV_XYZ, DV_ACC, DV_POSE, DV_OBS, DV_FCTR, DV_VOX, DV_CARVED, DV_FLAG, DV_CTR, DV_POSE_OWN, DV_KEPT, DV_CDEPTH, DV_MASK, DV_OWN, DV_COUNT };
static_assert(DV_COUNT == kDcvBufs, "esl_dense_int.hpp sizes DenseState::cv_set");
enum { DVC_CARVED, DVC_TESTED, DVC_COUNT };                                                  // the device counters
enum { DVF_IN_VIEW, DVF_DEPTH_OUT, DVF_OUTSIDE, DVF_AGREE, DVF_NEARER, DVF_THROUGH, DVF_NODATA, DVF_PAD, DVF_COUNT };   // obs_out's row
enum { DVO_USED, DVO_FOUND, DVO_CARVED, DVO_NOT_FOUND, DVO_COUNT };                          // own_out's row

struct DcvArgs {
  // the voxels and the observers
  const double* xyz; int n;
  const double* pose; int F_obs, n_chunks;
  const unsigned short* obs;
  double K[4]; int rows, cols;
  double depth_scale, depth_min, depth_max, depth_tol;
  int window, min_through, through_per_agree;
  u64* acc; int* fctr; u64* ctr;
  const unsigned int* sval; u64 H;
  int* vox; unsigned char* carved; long long n_vw;   // vox / carved null: not asked for
  unsigned char* flag;
  // the owners
  const double* pose_own; int F_own, stride, srows, scols;
  double leaf, m_scale, m_min, m_max;                // the map's own esl_dense_params
  const u64* keys; const DenseRec* rec;
  unsigned short* kept; unsigned short* cdepth; unsigned char* mask; int* own;   // cdepth / mask null: not asked for
};

// steps C2 and C3.  grid = (blocks over the voxels, chunks of frames: at most 65535 / kDcvChunk + 1, a workgroup takes blockIdx.y, + gridDim.y, ...)
static __global__ __launch_bounds__(kDenseThreads) void k_dcv_observe(DcvArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const bool in = i < a.n;
  double p[3] = {0, 0, 0};
  if (in) {
    for (int c = 0; c < 3; ++c) p[c] = a.xyz[i * 3 + c];
  }
  const size_t npix = (size_t)a.rows * a.cols;
  for (int ch = blockIdx.y; ch < a.n_chunks; ch += gridDim.y) {   // at most n_chunks rounds; workgroup-uniform
    const int f0 = ch * kDcvChunk, f1 = f0 + kDcvChunk < a.F_obs ? f0 + kDcvChunk : a.F_obs;
    u64 word = 0;   // this lane's counts of the chunk: at most kDcvChunk in a field
    for (int f = f0; f < f1; ++f) {   // at most kDcvChunk frames; workgroup-uniform
      int cls = -1;
      if (in) cls = dcv_observe(a.pose + (size_t)f * kDensePose, a.K, p, a.obs + (size_t)f * npix, a.rows, a.cols, a.window, a.depth_scale,
                                a.depth_min, a.depth_max, a.depth_tol);
      if (cls >= 0 && cls <= DCV_NODATA) word += dcv_pack_one(cls);
      {   // the frame's counts: one atomic per wave and count
        const u64 m_z = __ballot(cls == DCV_DEPTH_OUT), m_o = __ballot(cls == DCV_OUTSIDE);
        u64 m_c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) m_c[k] = __ballot(cls == k);
        if (lane == 0) {
          int* fc = a.fctr + (size_t)f * DVF_COUNT;
          const u64 m_v = m_c[0] | m_c[1] | m_c[2] | m_c[3];
          if (m_v) atomicAdd(&fc[DVF_IN_VIEW], __popcll(m_v));
          if (m_z) atomicAdd(&fc[DVF_DEPTH_OUT], __popcll(m_z));
          if (m_o) atomicAdd(&fc[DVF_OUTSIDE], __popcll(m_o));
#pragma unroll
          for (int k = 0; k < 4; ++k) if (m_c[k]) atomicAdd(&fc[DVF_AGREE + k], __popcll(m_c[k]));
        }
      }
    }
    if (word) atomicAdd(&a.acc[i], word);   // word != 0 only with i < n
  }
}

// step C4.  grid = blocks over the voxels
static __global__ __launch_bounds__(kDenseThreads) void k_dcv_verdict(DcvArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  bool carve = false, tested = false;
  if (i < a.n) {
    const u64 w = a.acc[i];
    const int agree = dcv_unpack(w, DCV_AGREE), nearer = dcv_unpack(w, DCV_NEARER), through = dcv_unpack(w, DCV_THROUGH),
              nodata = dcv_unpack(w, DCV_NODATA);
    carve = dcv_verdict(agree, through, a.min_through, a.through_per_agree);
    tested = agree + nearer + through > 0;
    if (i < a.n_vw) {
      if (a.vox) *(int4*)(a.vox + i * 4) = make_int4(agree, nearer, through, nodata);
      if (a.carved) a.carved[i] = carve ? 1 : 0;
    }
    const unsigned int slot = a.sval[i];
    if (slot < a.H) a.flag[slot] = carve ? 1 : 0;   // every live slot is in the list: k_dcv_mark reads no other byte
  }
  const u64 m_c = __ballot(carve), m_t = __ballot(tested);
  if (lane == 0) {
    if (m_c) atomicAdd(&a.ctr[DVC_CARVED], (u64)__popcll(m_c));
    if (m_t) atomicAdd(&a.ctr[DVC_TESTED], (u64)__popcll(m_t));
  }
}

// step C5.  grid = (blocks over the sampled pixels of a frame, frames: at most 65535, a workgroup takes blockIdx.y, + gridDim.y, ...)
static __global__ __launch_bounds__(kDenseThreads) void k_dcv_mark(DcvArgs a) {
  const int lane = threadIdx.x & 63;
  const long long per = (long long)a.srows * a.scols;
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const bool in = i < per;
  int row = 0, col = 0;
  if (in) { const DensePixel p = dense_sample_pixel(i, a.stride, a.scols); row = p.row; col = p.col; }
  for (int f = blockIdx.y; f < a.F_own; f += gridDim.y) {   // at most F_own rounds; workgroup-uniform
    const double* P = a.pose_own + (size_t)f * kDensePose;
    bool used = false, found = false, carve = false;
    if (in) {
      const size_t px = ((size_t)f * a.rows + row) * a.cols + col;
      const unsigned raw = a.kept[px];   // still depth_own's value: only this lane writes this pixel
      double pc[3], pw[3];
      int k[3];
      // dense_sample_key's three calls, written out: through the helper the listing changes
      if (dense_sample(raw, col, row, a.K, a.m_scale, a.m_min, a.m_max, pc) == DENSE_USED) {
        dense_world(P, pc, pw);
        if (dense_key(pw, a.leaf, k)) {
          used = true;
          const long long slot = dense_lookup(a.keys, a.H, dense_pack(k[0], k[1], k[2]));   // at most H probes
          found = slot >= 0 && a.rec[slot].count != 0;
          carve = found && a.flag[slot] != 0;
          if (carve) {
            a.kept[px] = 0;
            if (a.cdepth) a.cdepth[px] = (unsigned short)raw;
            if (a.mask) a.mask[px] = 1;
          }
        }
      }
    }
    const u64 m_u = __ballot(used), m_f = __ballot(found), m_c = __ballot(carve), m_n = __ballot(used && !found);
    if (lane == 0) {
      int* oc = a.own + (size_t)f * DVO_COUNT;
      if (m_u) atomicAdd(&oc[DVO_USED], __popcll(m_u));
      if (m_f) atomicAdd(&oc[DVO_FOUND], __popcll(m_f));
      if (m_c) atomicAdd(&oc[DVO_CARVED], __popcll(m_c));
      if (m_n) atomicAdd(&oc[DVO_NOT_FOUND], __popcll(m_n));
    }
  }
}

}  // namespace esl

using namespace esl;

extern "C" void esl_dense_carve_params_default(esl_dense_carve_params* p) {
  if (!p) return;
  p->depth_scale = 5000.0; p->depth_min = 0.1; p->depth_max = 6.0; p->depth_tol = 0.05;
  p->window = 1; p->min_through = 2; p->through_per_agree = 1; p->apply = 0;
}

extern "C" int esl_dense_carve_frames(esl_ctx* c, const double* cams_obs, int32_t F_obs, const uint16_t* depth_obs, const double* cams_own,
                                      int32_t F_own, const uint16_t* depth_own, const uint8_t* bgr_own, const int32_t* inst_own,
                                      const double K[4], int32_t rows, int32_t cols, const esl_dense_carve_params* pp, int64_t vox_cap,
                                      int32_t* vox_out, uint8_t* carved_out, int32_t* obs_out, uint16_t* depth_kept_out, uint8_t* mask_out,
                                      int32_t* own_out, esl_dense_carve_result* out) {
  const char* who = "esl_dense_carve_frames";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (!out) return dense_fail(ESL_ERR_INVALID, who, "null out");
  if (F_obs < 0) return dense_fail(ESL_ERR_INVALID, who, "negative F_obs");
  if (F_own < 0) return dense_fail(ESL_ERR_INVALID, who, "negative F_own");
  if (const char* m = dense_image_check(K, rows, cols)) return dense_fail(ESL_ERR_INVALID, who, m);
  if (vox_cap < 0) return dense_fail(ESL_ERR_INVALID, who, "negative vox_cap");
  esl_dense_carve_params p;
  if (pp) p = *pp; else esl_dense_carve_params_default(&p);
  if (const char* m = dcv_params_check(p)) return dense_fail(ESL_ERR_INVALID, who, m);
  if (F_obs > kDcvMaxObs) return dense_fail(ESL_ERR_INVALID, who, "F_obs > 65535");
  if (F_obs > 0 && !depth_obs) return dense_fail(ESL_ERR_INVALID, who, "null depth_obs");
  if (F_own > 0 && !cams_own) return dense_fail(ESL_ERR_INVALID, who, "null cams_own");
  if (F_own > 0 && !depth_own) return dense_fail(ESL_ERR_INVALID, who, "null depth_own");
  if (!dense_begun(c, who)) return ESL_ERR_STATE;
  DenseState& d = *c->dense;
  if (p.apply && F_own > 0 && d.with_color && !bgr_own) return dense_fail(ESL_ERR_STATE, who, "null bgr_own on a map begun with colour");
  if (p.apply && F_own > 0 && d.with_inst && !inst_own) return dense_fail(ESL_ERR_STATE, who, "null inst_own on a map begun with labels");
  if (const int rc = resident_source_check(c, who, !cams_obs && F_obs > 0, F_obs, false, 0)) return rc;
  std::memset(out, 0, sizeof(*out));
  if (dense_map_invalid(d, out)) return ESL_OK;   // step C7
  ESL_HIP_TRY(hipSetDevice(c->device));
  // the poses: R and t of every frame on the host, before anything runs
  if (F_obs > 0) {
    if (const int rc = dense_frames_poses(c, who, cams_obs, F_obs, d.cams, d.pose)) return rc;
  }
  if (F_own > 0) {
    if (const int rc = dense_frames_poses(c, who, cams_own, F_own, d.cams2, d.pose2)) return rc;
  }
  const int stride = d.p.stride, srows = (rows + stride - 1) / stride, scols = (cols + stride - 1) / stride;
  if ((long long)srows * scols * F_own >= (1ll << 31)) return dense_fail(ESL_ERR_INVALID, who, "more samples than a map holds: 2^31");

  const long long n = d.n_voxels, n_vw = (vox_out || carved_out) ? std::min<long long>(n, vox_cap) : 0;
  const size_t npix = (size_t)rows * cols, n_obs = (size_t)F_obs * npix, n_own = (size_t)F_own * npix;
  const bool apply = p.apply && F_own > 0, want_mask = mask_out && F_own > 0;
  out->n_voxels = (int32_t)n;
  ScratchSet<DV_COUNT>& s = d.cv_set;
  DenseList L;
  DenseOutArgs& k = L.k;
  if (n > 0) {
    if (const int rc = dense_list_begin(c, d, L)) return rc;
  }
  {
    const size_t sn = (size_t)n;
    const DenseSlot want[] = {{DV_XYZ, sn * 3 * sizeof(double)}, {DV_ACC, sn * sizeof(u64)}, {DV_POSE, (size_t)F_obs * kDensePose * sizeof(double)},
                              {DV_OBS, n_obs * sizeof(uint16_t)}, {DV_FCTR, (size_t)F_obs * DVF_COUNT * sizeof(int32_t)},
                              {DV_VOX, vox_out ? (size_t)n_vw * 4 * sizeof(int32_t) : 0}, {DV_CARVED, carved_out ? (size_t)n_vw : 0},
                              {DV_FLAG, (size_t)d.H}, {DV_CTR, DVC_COUNT * sizeof(u64)},
                              {DV_POSE_OWN, (size_t)F_own * kDensePose * sizeof(double)}, {DV_KEPT, n_own * sizeof(uint16_t)},
                              {DV_CDEPTH, apply ? n_own * sizeof(uint16_t) : 0}, {DV_MASK, want_mask ? n_own : 0},
                              {DV_OWN, (size_t)F_own * DVO_COUNT * sizeof(int32_t)}};
    if (const int rc = dense_grow(c, s, want, true)) return rc;
  }
  DcvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = (int)n; a.F_obs = F_obs; a.n_chunks = (F_obs + kDcvChunk - 1) / kDcvChunk;
  a.rows = rows; a.cols = cols;
  for (int i = 0; i < 4; ++i) a.K[i] = K[i];
  a.depth_scale = p.depth_scale; a.depth_min = p.depth_min; a.depth_max = p.depth_max; a.depth_tol = p.depth_tol;
  a.window = p.window; a.min_through = p.min_through; a.through_per_agree = p.through_per_agree;
  a.xyz = s.at<double>(DV_XYZ); a.acc = s.at<u64>(DV_ACC); a.fctr = s.at<int>(DV_FCTR); a.ctr = s.at<u64>(DV_CTR);
  a.H = d.H; a.flag = s.at<unsigned char>(DV_FLAG);
  if (vox_out) a.vox = s.at<int>(DV_VOX);
  if (carved_out) a.carved = s.at<unsigned char>(DV_CARVED);
  a.n_vw = n_vw;
  a.F_own = F_own; a.stride = stride; a.srows = srows; a.scols = scols;
  a.leaf = d.p.leaf; a.m_scale = d.p.depth_scale; a.m_min = d.p.depth_min; a.m_max = d.p.depth_max;
  a.keys = d.set.at<u64>(DB_KEYS); a.rec = d.set.at<DenseRec>(DB_REC);
  a.kept = s.at<unsigned short>(DV_KEPT); a.own = s.at<int>(DV_OWN);
  if (apply) a.cdepth = s.at<unsigned short>(DV_CDEPTH);
  if (want_mask) a.mask = s.at<unsigned char>(DV_MASK);
  const dim3 blk(kDenseThreads);

  ESL_HIP_TRY(hipMemsetAsync(a.ctr, 0, DVC_COUNT * sizeof(u64), c->stream));
  if (F_obs > 0) {
    if (const int rc = upload(c, s, DV_POSE, (const double*)d.pose.data(), (size_t)F_obs * kDensePose * sizeof(double), &a.pose)) return rc;
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[DV_OBS], depth_obs, n_obs * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    a.obs = s.at<unsigned short>(DV_OBS);
    ESL_HIP_TRY(hipMemsetAsync(a.fctr, 0, (size_t)F_obs * DVF_COUNT * sizeof(int32_t), c->stream));
  }
  if (n > 0) {   // steps C1 to C4
    k.oxyz = s.at<double>(DV_XYZ);
    k.n_write = n; k.with_color = d.with_color;
    a.sval = k.sval;
    ESL_HIP_TRY(hipMemsetAsync(a.acc, 0, (size_t)n * sizeof(u64), c->stream));
    {
      ProfScope ps(c, 4);
      if (const int rc = dense_list_launch(c, d, L, false, true)) return rc;
      if (F_obs > 0) hipLaunchKernelGGL(k_dcv_observe, dim3(dense_blocks((u64)n), (unsigned)a.n_chunks), blk, 0, c->stream, a);
      hipLaunchKernelGGL(k_dcv_verdict, dim3(dense_blocks((u64)n)), blk, 0, c->stream, a);
    }
    ESL_HIP_TRY(hipGetLastError());
  }
  if (F_own > 0) {   // step C5
    if (const int rc = upload(c, s, DV_POSE_OWN, (const double*)d.pose2.data(), (size_t)F_own * kDensePose * sizeof(double), &a.pose_own)) return rc;
    ESL_HIP_TRY(hipMemcpyAsync(a.kept, depth_own, n_own * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemsetAsync(a.own, 0, (size_t)F_own * DVO_COUNT * sizeof(int32_t), c->stream));
    if (a.cdepth) ESL_HIP_TRY(hipMemsetAsync(a.cdepth, 0, n_own * sizeof(uint16_t), c->stream));
    if (a.mask) ESL_HIP_TRY(hipMemsetAsync(a.mask, 0, n_own, c->stream));
    {
      ProfScope ps(c, 4);
      hipLaunchKernelGGL(k_dcv_mark, dim3(dense_blocks((u64)srows * (u64)scols), (unsigned)std::min(F_own, 65535)), blk, 0, c->stream, a);
    }
    ESL_HIP_TRY(hipGetLastError());
  }
  // the outputs
  if (n_vw > 0 && vox_out) ESL_HIP_TRY(hipMemcpyAsync(vox_out, a.vox, (size_t)n_vw * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (n_vw > 0 && carved_out) ESL_HIP_TRY(hipMemcpyAsync(carved_out, a.carved, (size_t)n_vw, hipMemcpyDeviceToHost, c->stream));
  if (F_obs > 0 && obs_out) ESL_HIP_TRY(hipMemcpyAsync(obs_out, a.fctr, (size_t)F_obs * DVF_COUNT * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  d.carve_own.assign((size_t)F_own * DVO_COUNT, 0);
  if (F_own > 0) {
    ESL_HIP_TRY(hipMemcpyAsync(d.carve_own.data(), a.own, (size_t)F_own * DVO_COUNT * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (depth_kept_out) ESL_HIP_TRY(hipMemcpyAsync(depth_kept_out, a.kept, n_own * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    if (mask_out) ESL_HIP_TRY(hipMemcpyAsync(mask_out, a.mask, n_own, hipMemcpyDeviceToHost, c->stream));
    if (apply) {
      d.carved_depth.resize(n_own);
      ESL_HIP_TRY(hipMemcpyAsync(d.carved_depth.data(), a.cdepth, n_own * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    }
  }
  u64 ctr[DVC_COUNT];
  ESL_HIP_TRY(hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's arrays are free again, the outputs filled
  out->n_carved = (int32_t)ctr[DVC_CARVED]; out->n_tested = (int32_t)ctr[DVC_TESTED];
  for (int f = 0; f < F_own; ++f) {
    out->samples_found += d.carve_own[(size_t)f * DVO_COUNT + DVO_FOUND];
    out->samples_carved += d.carve_own[(size_t)f * DVO_COUNT + DVO_CARVED];
  }
  if (own_out && F_own > 0) std::memcpy(own_out, d.carve_own.data(), (size_t)F_own * DVO_COUNT * sizeof(int32_t));
  if (apply) {   // step C6: dense-map step 8 on the carved samples alone
    if (const int rc = esl_dense_remove_frames(c, cams_own, F_own, K, rows, cols, d.carved_depth.data(), bgr_own, inst_own, &out->removed)) return rc;
    out->status = out->removed.status;
  }
  return ESL_OK;
}
