// esl_dense_render.hip — esl_dense_render (include/esl.h, "viewing the dense map"; the steps' numbers below are the header's; the
// arithmetic: esl_dense_proj.hpp).  It works on the dense map's sorted list (esl_dense_int.hpp, whose rule on stores and bounded loops
// holds here): the list and extract's gather into this unit's buffers (xyz, count, bgr, inst per voxel), then per chunk of frames
//   k_drn_splat     one lane per (voxel, frame); a workgroup's frame is uniform, so its R, t and K are scalar loads.  Steps 2 and 3 per
//                   lane, the frame's three counts by ballot + popcount, one atomic per wave and count.  Every pixel of the footprint
//                   takes a 64-bit atomicMin of zq << 32 | i into the chunk's z-buffer.  LOADFIRST: a relaxed load of the word first and
//                   the atomic only when the candidate is smaller -- the words only decrease, so a stale load can cost an atomic too
//                   many and never loses a winner; both forms leave the same bytes.  ESL_DRN_LOADFIRST=1 picks that form; the
//                   default is the unconditional atomic, the faster of the two on the synthetic room, where 94 % of the candidates
//                   pass the load (measurement: scripts/dense_render_bench.py).
//   k_drn_resolve   one lane per pixel of the chunk: the winner's index, its z recomputed by the same header function (the same
//                   bits), the images, the class against depth_meas; the frame's five counts by ballot + popcount, the voxel's counts
//                   by 32-bit integer atomics.
// A build with -DESL_DRN_COUNT also counts the candidates formed and the atomicMins issued and prints both on stderr: timing-only, the
// shipped kernel carries no such counter.
#include "esl_dense_int.hpp"
#include "esl_dense_check.hpp"
#include "esl_dense_proj.hpp"

#include <cstdio>

namespace esl {

// the call's buffers (DenseState::rn_set): per voxel, per call, per chunk of frames
enum { DR_XYZ, DR_CNT, DR_BGR, DR_INST, DR_POSE, DR_CTR, DR_FCTR, DR_VCTR, DR_ZBUF, DR_MEAS, DR_ODEPTH, DR_OVOX, DR_OBGR, DR_OINST, DR_COUNT };
static_assert(DR_COUNT == kDrnBufs, "esl_dense_int.hpp sizes DenseState::rn_set");
enum { DRC_SMALL, DRC_CAND, DRC_ATOM, DRC_COUNT };   // the device counters; the last two only in a -DESL_DRN_COUNT build
enum { DRF_DRAWN, DRF_DEPTH_OUT, DRF_OUTSIDE, DRF_COVERED, DRF_AGREE, DRF_NEARER, DRF_FARTHER, DRF_NODATA, DRF_COUNT };   // frame_out's row

struct DrnArgs {
  const double* xyz; const int* cnt; const unsigned char* bgr; const int* inst; int n;   // the voxels; bgr / inst null: not asked for
  const double* pose; double K[4]; int rows, cols;
  double e, depth_scale, depth_min, depth_max, depth_tol;
  int max_radius, min_count;
  u64* zbuf; int f0, nf;                        // the chunk: frames f0 .. f0 + nf - 1, nf rows cols words
  const unsigned short* meas;                   // the chunk's measured depth or null
  u64* ctr; int* fctr; int* vctr; long long n_vctr;   // DRC_*; F x 8; n_vctr x 4 (null: not asked for)
  double* odepth; int* ovox; unsigned char* obgr; int* oinst;   // the chunk's images; null: not asked for
};

// step 1: the voxels below min_count, once per call
static __global__ __launch_bounds__(kDenseThreads) void k_drn_small(DrnArgs a) {
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const u64 m = __ballot(i < a.n && a.cnt[i] < a.min_count);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.ctr[DRC_SMALL], (u64)__popcll(m));
}

// steps 2 to 4.  grid = (blocks over the voxels, frames of the chunk: at most 65535, a workgroup takes blockIdx.y, + gridDim.y, ...)
template <bool LOADFIRST>
static __global__ __launch_bounds__(kDenseThreads) void k_drn_splat(DrnArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  double p[3] = {0, 0, 0};
  bool live = false;
  if (i < a.n) {
    live = a.cnt[i] >= a.min_count;
    for (int c = 0; c < 3; ++c) p[c] = a.xyz[i * 3 + c];
  }
  const size_t npix = (size_t)a.rows * a.cols;
#ifdef ESL_DRN_COUNT
  u64 n_cand = 0, n_atom = 0;
#endif
  for (int fl = blockIdx.y; fl < a.nf; fl += gridDim.y) {   // at most nf rounds; workgroup-uniform
    const double* P = a.pose + (size_t)(a.f0 + fl) * kDensePose;
    int cat = -1, box[4] = {0, -1, 0, -1};
    double z = 0;
    if (live) cat = drn_project(P, a.K, p, a.e, a.max_radius, a.rows, a.cols, a.depth_min, a.depth_max, &z, box);
    {   // the frame's counts: one atomic per wave and count
      const u64 m_d = __ballot(cat == DRN_DRAWN), m_z = __ballot(cat == DRN_DEPTH_OUT), m_o = __ballot(cat == DRN_OUTSIDE);
      if (lane == 0) {
        int* fc = a.fctr + (size_t)(a.f0 + fl) * DRF_COUNT;
        if (m_d) atomicAdd(&fc[DRF_DRAWN], __popcll(m_d));
        if (m_z) atomicAdd(&fc[DRF_DEPTH_OUT], __popcll(m_z));
        if (m_o) atomicAdd(&fc[DRF_OUTSIDE], __popcll(m_o));
      }
    }
    if (cat != DRN_DRAWN) continue;
    const u64 word = drn_word(z, (unsigned)i);
    u64* zb = a.zbuf + (size_t)fl * npix;
    // 0 <= box[2] <= box[3] <= rows - 1 and 0 <= box[0] <= box[1] <= cols - 1 (drn_axis clips), each range at most 2 max_radius + 1
    // long: at most (2 max_radius + 1)^2 <= 129^2 pixels
    for (int r = box[2]; r <= box[3]; ++r) {
      u64* row = zb + (size_t)r * a.cols;
      for (int c = box[0]; c <= box[1]; ++c) {
#ifdef ESL_DRN_COUNT
        ++n_cand;
#endif
        if (LOADFIRST && !(word < __hip_atomic_load(&row[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) continue;
        atomicMin(&row[c], word);
#ifdef ESL_DRN_COUNT
        ++n_atom;
#endif
      }
    }
  }
#ifdef ESL_DRN_COUNT
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { n_cand += __shfl_xor(n_cand, off, 64); n_atom += __shfl_xor(n_atom, off, 64); }
  if (lane == 0 && n_cand) { atomicAdd(&a.ctr[DRC_CAND], n_cand); atomicAdd(&a.ctr[DRC_ATOM], n_atom); }
#endif
}

// steps 4 to 6.  grid = (blocks over the pixels of a frame, frames of the chunk as above)
static __global__ __launch_bounds__(kDenseThreads) void k_drn_resolve(DrnArgs a) {
  const int lane = threadIdx.x & 63;
  const size_t npix = (size_t)a.rows * a.cols;
  const size_t px = (size_t)blockIdx.x * kDenseThreads + threadIdx.x;
  const bool in = px < npix;
  for (int fl = blockIdx.y; fl < a.nf; fl += gridDim.y) {   // at most nf rounds; workgroup-uniform
    const int f = a.f0 + fl;
    const double* P = a.pose + (size_t)f * kDensePose;
    const size_t o = (size_t)fl * npix + px;
    const u64 word = in ? a.zbuf[o] : kDrnEmpty;
    const unsigned i = drn_word_index(word);
    const bool won = word != kDrnEmpty && i < (unsigned)a.n;
    double z = __builtin_nan("");
    int cat = -1;
    if (won) {
      z = drn_cam_z(P, a.xyz + (size_t)i * 3);
      if (a.meas) cat = drn_compare(a.meas[o], z, a.depth_scale, a.depth_min, a.depth_max, a.depth_tol);
    }
    if (in) {
      if (a.odepth) a.odepth[o] = z;
      if (a.ovox) a.ovox[o] = won ? (int)i : -1;
      if (a.obgr) {
        for (int c = 0; c < 3; ++c) a.obgr[o * 3 + c] = won ? a.bgr[(size_t)i * 3 + c] : (unsigned char)0;
      }
      if (a.oinst) a.oinst[o] = won ? a.inst[i] : -1;
    }
    {   // the frame's counts: one atomic per wave and count
      const u64 m_w = __ballot(won);
      u64 m_c[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) m_c[k] = __ballot(cat == k);
      if (lane == 0 && m_w) {
        int* fc = a.fctr + (size_t)f * DRF_COUNT;
        atomicAdd(&fc[DRF_COVERED], __popcll(m_w));
#pragma unroll
        for (int k = 0; k < 4; ++k) if (m_c[k]) atomicAdd(&fc[DRF_AGREE + k], __popcll(m_c[k]));
      }
    }
    if (won && a.vctr && (long long)i < a.n_vctr) {
      atomicAdd(&a.vctr[(size_t)i * 4], 1);
      if (cat >= 0 && cat < 3) atomicAdd(&a.vctr[(size_t)i * 4 + 1 + cat], 1);
    }
  }
}

}  // namespace esl

using namespace esl;

extern "C" void esl_dense_render_params_default(esl_dense_render_params* p) {
  if (!p) return;
  p->depth_scale = 5000.0; p->depth_min = 0.1; p->depth_max = 6.0; p->depth_tol = 0.05; p->footprint = 1.0;
  p->max_radius = 8; p->min_count = 1; p->zbuf_bytes = 268435456;
}

namespace {

// ESL_DRN_LOADFIRST: 1 = the load-first form; otherwise (and unset) every candidate takes its atomicMin
bool drn_load_first() {
  const char* e = std::getenv("ESL_DRN_LOADFIRST");
  return e && e[0] == '1' && e[1] == 0;
}

}  // namespace

extern "C" int esl_dense_render(esl_ctx* c, const double* cams, int32_t F, const double K[4], int32_t rows, int32_t cols,
                                const uint16_t* depth_meas, const esl_dense_render_params* pp, double* depth_out, int32_t* voxel_out,
                                uint8_t* bgr_out, int32_t* inst_out, int32_t* frame_out, int64_t vox_cap, int32_t* vox_out,
                                esl_dense_render_result* out) {
  const char* who = "esl_dense_render";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (!out) return dense_fail(ESL_ERR_INVALID, who, "null out");
  if (F < 0) return dense_fail(ESL_ERR_INVALID, who, "negative F");
  if (const char* m = dense_image_check(K, rows, cols)) return dense_fail(ESL_ERR_INVALID, who, m);
  if (vox_cap < 0) return dense_fail(ESL_ERR_INVALID, who, "negative vox_cap");
  if (vox_cap > 0 && !vox_out) return dense_fail(ESL_ERR_INVALID, who, "null vox_out with vox_cap > 0");
  esl_dense_render_params p;
  if (pp) p = *pp; else esl_dense_render_params_default(&p);
  const size_t npix = (size_t)rows * cols;
  if (const char* m = drn_params_check(p, npix)) return dense_fail(ESL_ERR_INVALID, who, m);
  if (!dense_begun(c, who)) return ESL_ERR_STATE;
  if (const int rc = resident_source_check(c, who, !cams && F > 0, F, false, 0)) return rc;
  DenseState& d = *c->dense;
  std::memset(out, 0, sizeof(*out));
  if (dense_map_invalid(d, out)) return ESL_OK;   // step 8: nothing is written
  ESL_HIP_TRY(hipSetDevice(c->device));
  // the poses: R and t of every frame on the host, before anything runs
  if (F > 0) {
    if (const int rc = dense_frames_poses(c, who, cams, F, d.cams, d.pose)) return rc;
  }
  const long long n = d.n_voxels, n_vw = vox_out ? std::min<long long>(n, vox_cap) : 0;
  const long long chunk = std::max<long long>(1, (long long)((u64)p.zbuf_bytes / (8 * (u64)npix)));   // step 7
  out->n_voxels = (int32_t)n;
  out->n_chunks = (int32_t)((F + chunk - 1) / chunk);
  const bool images = depth_out || voxel_out || bgr_out || inst_out;
  const bool frames = F > 0 && (images || frame_out || n_vw > 0);
  if (n == 0) {   // nothing to draw: empty images, zero counts
    const size_t n_img = (size_t)F * npix;
    if (depth_out) std::fill(depth_out, depth_out + n_img, std::nan(""));
    if (voxel_out) std::fill(voxel_out, voxel_out + n_img, -1);
    if (bgr_out) std::memset(bgr_out, 0, n_img * 3);
    if (inst_out) std::fill(inst_out, inst_out + n_img, -1);
    if (frame_out) std::memset(frame_out, 0, (size_t)F * DRF_COUNT * sizeof(int32_t));
    return ESL_OK;
  }

  ScratchSet<DR_COUNT>& s = d.rn_set;
  DenseList L;
  if (const int rc = dense_list_begin(c, d, L)) return rc;
  DenseOutArgs& k = L.k;
  const int cf = (int)std::min<long long>(F, chunk);   // frames per chunk
  {
    const size_t sn = (size_t)n, sc = (size_t)cf * npix;
    const DenseSlot want[] = {{DR_XYZ, frames ? sn * 3 * sizeof(double) : 0}, {DR_CNT, sn * sizeof(int32_t)},
                              {DR_BGR, frames && bgr_out ? sn * 3 : 0}, {DR_INST, frames && inst_out ? sn * sizeof(int32_t) : 0},
                              {DR_POSE, frames ? (size_t)F * kDensePose * sizeof(double) : 0}, {DR_CTR, DRC_COUNT * sizeof(u64)},
                              {DR_FCTR, frames ? (size_t)F * DRF_COUNT * sizeof(int32_t) : 0}, {DR_VCTR, frames ? (size_t)n_vw * 4 * sizeof(int32_t) : 0},
                              {DR_ZBUF, frames ? sc * sizeof(u64) : 0}, {DR_MEAS, frames && depth_meas ? sc * sizeof(uint16_t) : 0},
                              {DR_ODEPTH, frames && depth_out ? sc * sizeof(double) : 0}, {DR_OVOX, frames && voxel_out ? sc * sizeof(int32_t) : 0},
                              {DR_OBGR, frames && bgr_out ? sc * 3 : 0}, {DR_OINST, frames && inst_out ? sc * sizeof(int32_t) : 0}};
    if (const int rc = dense_grow(c, s, want, true)) return rc;
  }
  DrnArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = (int)n; a.cnt = s.at<int>(DR_CNT); a.ctr = s.at<u64>(DR_CTR);
  a.rows = rows; a.cols = cols;
  for (int i = 0; i < 4; ++i) a.K[i] = K[i];
  a.e = p.footprint * d.p.leaf / 2;   // step 3: one double, computed here
  a.depth_scale = p.depth_scale; a.depth_min = p.depth_min; a.depth_max = p.depth_max; a.depth_tol = p.depth_tol;
  a.max_radius = p.max_radius; a.min_count = p.min_count;
  k.ocnt = s.at<int>(DR_CNT);
  if (frames) {
    k.oxyz = s.at<double>(DR_XYZ); a.xyz = k.oxyz;
    if (bgr_out) { k.obgr = s.at<unsigned char>(DR_BGR); a.bgr = k.obgr; }
    if (inst_out) { k.oinst = s.at<int>(DR_INST); a.inst = k.oinst; }
  }
  k.n_write = n; k.with_color = d.with_color;
  const dim3 blk(kDenseThreads);

  // step 1: the list, the voxels' numbers, n_small
  ESL_HIP_TRY(hipMemsetAsync(a.ctr, 0, DRC_COUNT * sizeof(u64), c->stream));
  {
    ProfScope ps(c, 4);
    if (const int rc = dense_list_launch(c, d, L, d.with_inst && frames && inst_out, true)) return rc;
    hipLaunchKernelGGL(k_drn_small, dim3(dense_blocks((u64)n)), blk, 0, c->stream, a);
  }
  ESL_HIP_TRY(hipGetLastError());

  if (frames) {
    if (const int rc = upload(c, s, DR_POSE, (const double*)d.pose.data(), (size_t)F * kDensePose * sizeof(double), &a.pose)) return rc;
    a.fctr = s.at<int>(DR_FCTR);
    ESL_HIP_TRY(hipMemsetAsync(a.fctr, 0, (size_t)F * DRF_COUNT * sizeof(int32_t), c->stream));
    if (n_vw > 0) {
      a.vctr = s.at<int>(DR_VCTR); a.n_vctr = n_vw;
      ESL_HIP_TRY(hipMemsetAsync(a.vctr, 0, (size_t)n_vw * 4 * sizeof(int32_t), c->stream));
    }
    a.zbuf = s.at<u64>(DR_ZBUF);
    if (depth_out) a.odepth = s.at<double>(DR_ODEPTH);
    if (voxel_out) a.ovox = s.at<int>(DR_OVOX);
    if (bgr_out) a.obgr = s.at<unsigned char>(DR_OBGR);
    if (inst_out) a.oinst = s.at<int>(DR_OINST);
    const bool load_first = drn_load_first();
    // steps 2 to 7, chunk after chunk; the chunk's buffers are free again once its images have reached the host
    for (long long f0 = 0; f0 < F; f0 += chunk) {
      const int nf = (int)std::min<long long>(chunk, F - f0);
      const size_t cpix = (size_t)nf * npix, off = (size_t)f0 * npix;
      a.f0 = (int)f0; a.nf = nf;
      ESL_HIP_TRY(hipMemsetAsync(a.zbuf, 0xFF, cpix * sizeof(u64), c->stream));   // every word kDrnEmpty
      if (depth_meas) {
        ESL_HIP_TRY(hipMemcpyAsync(s.buf[DR_MEAS], depth_meas + off, cpix * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        a.meas = s.at<unsigned short>(DR_MEAS);
      }
      {
        ProfScope ps(c, 4);
        const unsigned gy = (unsigned)std::min(nf, 65535);
        if (load_first) hipLaunchKernelGGL(k_drn_splat<true>, dim3(dense_blocks((u64)n), gy), blk, 0, c->stream, a);
        else hipLaunchKernelGGL(k_drn_splat<false>, dim3(dense_blocks((u64)n), gy), blk, 0, c->stream, a);
        hipLaunchKernelGGL(k_drn_resolve, dim3(dense_blocks((u64)npix), gy), blk, 0, c->stream, a);
      }
      ESL_HIP_TRY(hipGetLastError());
      if (depth_out) ESL_HIP_TRY(hipMemcpyAsync(depth_out + off, a.odepth, cpix * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      if (voxel_out) ESL_HIP_TRY(hipMemcpyAsync(voxel_out + off, a.ovox, cpix * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      if (bgr_out) ESL_HIP_TRY(hipMemcpyAsync(bgr_out + off * 3, a.obgr, cpix * 3, hipMemcpyDeviceToHost, c->stream));
      if (inst_out) ESL_HIP_TRY(hipMemcpyAsync(inst_out + off, a.oinst, cpix * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      if (f0 + chunk < F) ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (frame_out) ESL_HIP_TRY(hipMemcpyAsync(frame_out, a.fctr, (size_t)F * DRF_COUNT * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (n_vw > 0) ESL_HIP_TRY(hipMemcpyAsync(vox_out, a.vctr, (size_t)n_vw * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  }
  u64 ctr[DRC_COUNT];
  ESL_HIP_TRY(hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's arrays are free again, the outputs filled
  out->n_small = (int32_t)ctr[DRC_SMALL];
#ifdef ESL_DRN_COUNT
  std::fprintf(stderr, "esl_dense_render: candidates %llu atomics %llu\n", ctr[DRC_CAND], ctr[DRC_ATOM]);
#endif
  return ESL_OK;
}
