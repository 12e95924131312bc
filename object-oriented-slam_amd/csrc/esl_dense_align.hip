// esl_dense_align.hip — esl_dense_normals and esl_dense_align_frames (include/esl.h, "normals of the dense map" and "aligning frames to
// the dense map"; the steps' names below are the header's; the arithmetic: esl_dense_align.hpp).  Both work on the dense map's sorted list
// (esl_dense_int.hpp, whose rule on stores and bounded loops holds here) and read the map without changing it:
//   k_dnr_normals   one lane per voxel of the sorted list.  It notes its index under its table slot (sidx: slot -> index, -1 elsewhere),
//                   probes the (2 radius + 1)^3 neighbour keys in ascending packed-key order (dense_lookup), reads each neighbour's
//                   record, sums the moments in that order and runs the Jacobi in registers.  No atomics but the two counts (ballot +
//                   popcount): the per-lane loop is the summation order.
//   k_dal_accum     grid = (sampled pixels / 256, frames); a workgroup's frame is uniform, so its R, t, K and its flag are scalar loads
//                   and a stopped frame is skipped by a uniform branch.  One lane per sample does steps a to c: the sample as k_dense_insert
//                   forms it (dense_sample_pixel / _key), (2 reach + 1)^3 probes, slot -> index -> valid, centroid and normal, the 28 terms.  The 29
//                   integers are folded across the wave by a shuffle butterfly, the waves meet in LDS, and one 64-bit atomicAdd per
//                   workgroup and non-zero term goes into the frame's row; the eight counts by ballot + popcount, one atomic per wave
//                   and count.  No atomic returns a value.
// The Gauss-Newton step runs on the host between the passes (dal_system / dal_solve / dal_update): 12 doubles and a flag per frame go
// up, 37 words per frame come back.
#include "esl_dense_int.hpp"
#include "esl_dense_align.hpp"
#include "esl_dense_check.hpp"

namespace esl {

// the calls' buffers (DenseState::al_set): per voxel, per table slot, per call, per pass
enum { DA_XYZ, DA_SIDX, DA_NRM, DA_CURV, DA_M, DA_VALID, DA_CTR, DA_POSE, DA_FLAG, DA_DEPTH, DA_ACC, DA_COUNT };
static_assert(DA_COUNT == kDalBufs, "esl_dense_int.hpp sizes DenseState::al_set");
enum { DAC_ELIGIBLE, DAC_VALID, DAC_COUNT };

struct DnrArgs {
  const u64* keys; const DenseRec* rec; u64 H;
  const u64* skey; const unsigned int* sval; int n;
  int radius, min_count, min_neighbors; double max_curvature;
  int* sidx; double* nrm; double* curv; int* m; unsigned char* valid; u64* ctr;
};

// steps N1 to N5
static __global__ __launch_bounds__(kDenseThreads) void k_dnr_normals(DnrArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  bool elig = false, val = false;
  if (i < a.n) {
    const unsigned int slot = a.sval[i];
    double n[3] = {0, 0, 0}, curv = __builtin_nan("");
    int m = 0;
    if (slot < a.H) {
      a.sidx[slot] = (int)i;
      const DenseRec* r = a.rec + slot;
      const long long cnt = (long long)r->count;
      elig = cnt >= (long long)a.min_count;
      if (elig) {
        const double ci[3] = {dense_mean(r->S[0], cnt), dense_mean(r->S[1], cnt), dense_mean(r->S[2], cnt)};
        int k[3];
        dense_unpack(a.skey[i], k);
        double s[3] = {0, 0, 0}, M[6] = {0, 0, 0, 0, 0, 0};
        // at most 125 keys, each at most H probes: ascending (kx, ky, kz) is ascending packed key
        for (int dx = -a.radius; dx <= a.radius; ++dx)
          for (int dy = -a.radius; dy <= a.radius; ++dy)
            for (int dz = -a.radius; dz <= a.radius; ++dz) {
              const int kx = k[0] + dx, ky = k[1] + dy, kz = k[2] + dz;
              if (!dense_key_in_range(kx, ky, kz)) continue;
              const long long sj = (dx | dy | dz) == 0 ? (long long)slot : dense_lookup(a.keys, a.H, dense_pack(kx, ky, kz));
              if (sj < 0) continue;
              const DenseRec* rj = a.rec + sj;
              const long long cj = (long long)rj->count;
              if (cj < (long long)a.min_count) continue;   // a dead slot has count 0 < 1
              const double c[3] = {dense_mean(rj->S[0], cj), dense_mean(rj->S[1], cj), dense_mean(rj->S[2], cj)};
              dnr_add(ci, c, &m, s, M);
            }
        val = dnr_finish(m, s, M, a.min_neighbors, a.max_curvature, n, &curv);
      }
    }
    a.nrm[i * 3] = n[0]; a.nrm[i * 3 + 1] = n[1]; a.nrm[i * 3 + 2] = n[2];
    a.curv[i] = curv; a.m[i] = m; a.valid[i] = val ? (unsigned char)1 : (unsigned char)0;
  }
  const u64 m_e = __ballot(elig), m_v = __ballot(val);
  if (lane == 0) {
    if (m_e) atomicAdd(&a.ctr[DAC_ELIGIBLE], (u64)__popcll(m_e));
    if (m_v) atomicAdd(&a.ctr[DAC_VALID], (u64)__popcll(m_v));
  }
}

struct DalArgs {
  const u64* keys; u64 H; const int* sidx; int n;
  const double* xyz; const double* nrm; const unsigned char* valid;
  const double* pose; const int* flag; int F;
  double K[4];
  int rows, cols, stride, srows, scols, reach;
  const unsigned short* depth;
  double leaf, depth_scale, depth_min, depth_max, max_dist2;
  u64* acc;   // F x kDalRow
};

// steps a to c.  grid = (blocks over the sampled pixels of a frame, frames: at most 65535, a workgroup takes blockIdx.y, + gridDim.y, ...)
static __global__ __launch_bounds__(kDenseThreads) void k_dal_accum(DalArgs a) {
  __shared__ long long part[kDenseThreads / 64][kDalFold];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long per = (long long)a.srows * a.scols;
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const bool in = i < per;
  int row = 0, col = 0;
  if (in) { const DensePixel p = dense_sample_pixel(i, a.stride, a.scols); row = p.row; col = p.col; }
  for (int f = blockIdx.y; f < a.F; f += gridDim.y) {   // at most F rounds; workgroup-uniform, and so is the flag
    if (a.flag[f] == 0) continue;
    const double* P = a.pose + (size_t)f * kDensePose;
    double o[3];
    dal_centre(P, o);
    int cat = -1, cls = DAL_CLASS_NONE;
    long long T[kDalFold];
#pragma unroll
    for (int k = 0; k < kDalFold; ++k) T[k] = 0;
    if (in) {
      const size_t px = ((size_t)f * a.rows + row) * a.cols + col;
      double pc[3], pw[3];
      int k[3];
      cat = dense_sample_key(a.depth[px], col, row, a.K, a.depth_scale, a.depth_min, a.depth_max, P, a.leaf, pc, pw, k);
      if (cat == DENSE_USED) {
        long long best = -1;
        double best_d2 = 0;
        // at most 125 keys, each at most H probes: ascending (kx, ky, kz) is ascending packed key, a tie keeps the earlier
        for (int dx = -a.reach; dx <= a.reach; ++dx)
          for (int dy = -a.reach; dy <= a.reach; ++dy)
            for (int dz = -a.reach; dz <= a.reach; ++dz) {
              const int kx = k[0] + dx, ky = k[1] + dy, kz = k[2] + dz;
              if (!dense_key_in_range(kx, ky, kz)) continue;
              const long long slot = dense_lookup(a.keys, a.H, dense_pack(kx, ky, kz));
              if (slot < 0) continue;
              const int j = a.sidx[slot];
              if (j < 0 || j >= a.n || !a.valid[j]) continue;
              const double d2 = dal_dist2(pw, a.xyz + (size_t)j * 3);
              if (best < 0 || d2 < best_d2) { best = j; best_d2 = d2; }
            }
        cls = dal_class(best >= 0, best_d2, a.max_dist2);
        if (cls == DAL_CLASS_INLIER) {
          dal_terms(pw, o, a.xyz + (size_t)best * 3, a.nrm + (size_t)best * 3, T);
          T[DAL_FOLD_N] = 1;
        }
      }
    }
    u64* rowp = a.acc + (size_t)f * kDalRow;
    {   // the eight counts: one atomic per wave and count
      const u64 m[8] = {__ballot(in), __ballot(cat == DENSE_ZERO), __ballot(cat == DENSE_DEPTH_OUT), __ballot(cat == DENSE_KEY_OUT),
                        __ballot(cat == DENSE_USED), __ballot(cls == DAL_CLASS_NOMATCH), __ballot(cls == DAL_CLASS_FAR),
                        __ballot(cls == DAL_CLASS_INLIER)};
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) if (m[k]) atomicAdd(&rowp[DAL_SAMPLED + k], (u64)__popcll(m[k]));
      }
    }
    // the 29 integers: a butterfly across the wave (integer addition: any order gives the same bits), then the waves in LDS
    const bool any = __ballot(cls == DAL_CLASS_INLIER) != 0;   // wave-uniform
#pragma unroll
    for (int k = 0; k < kDalFold; ++k) {
      long long v = T[k];
      if (any) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      }
      if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kDalFold) {
      long long v = 0;
#pragma unroll
      for (int w = 0; w < kDenseThreads / 64; ++w) v += part[w][threadIdx.x];
      if (v) atomicAdd(&rowp[threadIdx.x], (u64)v);
    }
    __syncthreads();   // part is free for the next frame
  }
}

}  // namespace esl

using namespace esl;

extern "C" void esl_dense_normal_params_default(esl_dense_normal_params* p) {
  if (!p) return;
  p->max_curvature = 0.05; p->radius = 1; p->min_count = 1; p->min_neighbors = 5;
}

extern "C" void esl_dense_align_params_default(esl_dense_align_params* p) {
  if (!p) return;
  p->max_dist = 0.0; p->damping = 0.0; p->min_pivot_ratio = 1e-6; p->tol_t = 1e-5; p->tol_r = 1e-5;
  p->iters = 4; p->stride = 2; p->reach = 1; p->min_inliers = 100;
  esl_dense_normal_params_default(&p->normals);
}

namespace {

// Steps N1 to N5 over the map as it is: the sorted list, the centroids (extract's gather) and the normals into al_set, sidx rebuilt.
// counts: DAC_*.  The caller has checked the map's status and set the device.
int dnr_run(esl_ctx* c, DenseState& d, const esl_dense_normal_params& p, DnrArgs& a, u64 counts[DAC_COUNT]) {
  ScratchSet<DA_COUNT>& s = d.al_set;
  const size_t n = (size_t)d.n_voxels;
  DenseList L;
  if (const int rc = dense_list_begin(c, d, L)) return rc;
  DenseOutArgs& k = L.k;
  const DenseSlot want[] = {{DA_XYZ, n * 3 * sizeof(double)}, {DA_SIDX, (size_t)d.H * sizeof(int32_t)}, {DA_NRM, n * 3 * sizeof(double)},
                            {DA_CURV, n * sizeof(double)}, {DA_M, n * sizeof(int32_t)}, {DA_VALID, n}, {DA_CTR, DAC_COUNT * sizeof(u64)}};
  if (const int rc = dense_grow(c, s, want, false)) return rc;
  std::memset(&a, 0, sizeof(a));
  a.keys = k.keys; a.rec = k.rec; a.H = k.H; a.skey = k.skey; a.sval = k.sval; a.n = (int)n;
  a.radius = p.radius; a.min_count = p.min_count; a.min_neighbors = p.min_neighbors; a.max_curvature = p.max_curvature;
  a.sidx = s.at<int>(DA_SIDX); a.nrm = s.at<double>(DA_NRM); a.curv = s.at<double>(DA_CURV); a.m = s.at<int>(DA_M);
  a.valid = s.at<unsigned char>(DA_VALID); a.ctr = s.at<u64>(DA_CTR);
  k.oxyz = s.at<double>(DA_XYZ); k.n_write = (long long)n; k.with_color = d.with_color;
  ESL_HIP_TRY(hipMemsetAsync(a.ctr, 0, DAC_COUNT * sizeof(u64), c->stream));
  ESL_HIP_TRY(hipMemsetAsync(a.sidx, 0xFF, (size_t)d.H * sizeof(int32_t), c->stream));   // every slot -1
  if (n > 0) {
    ProfScope ps(c, 4);
    if (const int rc = dense_list_launch(c, d, L, false, true)) return rc;
    hipLaunchKernelGGL(k_dnr_normals, dim3(dense_blocks((u64)n)), dim3(kDenseThreads), 0, c->stream, a);
  }
  ESL_HIP_TRY(hipGetLastError());
  ESL_HIP_TRY(hipMemcpyAsync(counts, a.ctr, DAC_COUNT * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  return ESL_OK;
}

}  // namespace

extern "C" int esl_dense_normals(esl_ctx* c, const esl_dense_normal_params* pp, int64_t cap, double* normal_out, double* curvature_out,
                                 int32_t* neighbors_out, uint8_t* valid_out, esl_dense_normal_result* out) {
  const char* who = "esl_dense_normals";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (!out) return dense_fail(ESL_ERR_INVALID, who, "null out");
  if (cap < 0) return dense_fail(ESL_ERR_INVALID, who, "negative cap");
  esl_dense_normal_params p;
  if (pp) p = *pp; else esl_dense_normal_params_default(&p);
  if (const char* m = dnr_params_check(p)) return dense_fail(ESL_ERR_INVALID, who, m);
  if (!dense_begun(c, who)) return ESL_ERR_STATE;
  DenseState& d = *c->dense;
  std::memset(out, 0, sizeof(*out));
  if (dense_map_invalid(d, out)) return ESL_OK;
  ESL_HIP_TRY(hipSetDevice(c->device));
  DnrArgs a;
  u64 counts[DAC_COUNT];
  if (const int rc = dnr_run(c, d, p, a, counts)) return rc;
  const size_t nw = (size_t)std::min<long long>(d.n_voxels, cap);
  if (nw > 0) {
    if (normal_out) ESL_HIP_TRY(hipMemcpyAsync(normal_out, a.nrm, nw * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (curvature_out) ESL_HIP_TRY(hipMemcpyAsync(curvature_out, a.curv, nw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (neighbors_out) ESL_HIP_TRY(hipMemcpyAsync(neighbors_out, a.m, nw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (valid_out) ESL_HIP_TRY(hipMemcpyAsync(valid_out, a.valid, nw, hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  }
  out->n_voxels = (int32_t)d.n_voxels; out->n_eligible = (int32_t)counts[DAC_ELIGIBLE]; out->n_valid = (int32_t)counts[DAC_VALID];
  return ESL_OK;
}

extern "C" int esl_dense_align_frames(esl_ctx* c, const double* cams, int32_t F, const double K[4], int32_t rows, int32_t cols,
                                      const uint16_t* depth, const esl_dense_align_params* pp, double* cams_out,
                                      esl_dense_align_frame* frames_out, int64_t* iter_out, esl_dense_align_result* out) {
  const char* who = "esl_dense_align_frames";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (!out) return dense_fail(ESL_ERR_INVALID, who, "null out");
  if (F < 0) return dense_fail(ESL_ERR_INVALID, who, "negative F");
  if (const char* m = dense_image_check(K, rows, cols)) return dense_fail(ESL_ERR_INVALID, who, m);
  if (!std::isfinite(K[2]) || !std::isfinite(K[3])) return dense_fail(ESL_ERR_INVALID, who, "cx or cy not finite");
  if (F > 0 && !depth) return dense_fail(ESL_ERR_INVALID, who, "null depth");
  esl_dense_align_params p;
  if (pp) p = *pp; else esl_dense_align_params_default(&p);
  if (const char* m = dal_params_check(p)) return dense_fail(ESL_ERR_INVALID, who, m);
  if (!dense_begun(c, who)) return ESL_ERR_STATE;
  if (const int rc = resident_source_check(c, who, !cams && F > 0, F, false, 0)) return rc;
  DenseState& d = *c->dense;
  std::memset(out, 0, sizeof(*out));
  if (dense_map_invalid(d, out)) return ESL_OK;   // step e: nothing is written
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (F > 0) {
    if (const int rc = dense_frames_poses(c, who, cams, F, d.cams, d.pose)) return rc;
  }
  const int srows = (rows + p.stride - 1) / p.stride, scols = (cols + p.stride - 1) / p.stride;
  const long long per = (long long)srows * scols;
  if (per * F >= (1ll << 31)) return dense_fail(ESL_ERR_INVALID, who, "more samples than a map holds: 2^31");
  const double max_dist2 = dal_max_dist2(p.max_dist, p.reach, d.p.leaf);
  if (!dal_sums_fit(per, dal_bound(K, rows, cols, d.p.depth_max, max_dist2)))
    return dense_fail(ESL_ERR_INVALID, who, "the sums of a frame could reach 2^62");

  DnrArgs nr;
  u64 counts[DAC_COUNT];
  if (const int rc = dnr_run(c, d, p.normals, nr, counts)) return rc;
  out->n_voxels = (int32_t)d.n_voxels; out->n_valid = (int32_t)counts[DAC_VALID];
  if (F == 0) return ESL_OK;

  ScratchSet<DA_COUNT>& s = d.al_set;
  const int np = p.iters + 1;
  DalArgs a;
  std::memset(&a, 0, sizeof(a));
  a.keys = nr.keys; a.H = nr.H; a.sidx = nr.sidx; a.n = nr.n; a.xyz = s.at<double>(DA_XYZ); a.nrm = nr.nrm; a.valid = nr.valid;
  a.F = F; a.rows = rows; a.cols = cols; a.stride = p.stride; a.srows = srows; a.scols = scols; a.reach = p.reach;
  for (int i = 0; i < 4; ++i) a.K[i] = K[i];
  a.leaf = d.p.leaf; a.depth_scale = d.p.depth_scale; a.depth_min = d.p.depth_min; a.depth_max = d.p.depth_max; a.max_dist2 = max_dist2;
  if (const int rc = upload(c, s, DA_DEPTH, depth, (size_t)F * rows * cols * sizeof(uint16_t), &a.depth)) return rc;
  if (const int rc = s.grow(c, DA_ACC, (size_t)F * kDalRow * sizeof(u64))) return rc;
  a.acc = s.at<u64>(DA_ACC);

  std::vector<double> cam(d.cams.begin(), d.cams.begin() + (size_t)F * 7);   // the frames' poses as they move
  std::vector<int> flag((size_t)F, 1), last((size_t)F, 0);                     // runs this pass; this pass only evaluates
  std::vector<long long> acc((size_t)F * kDalRow);
  std::vector<esl_dense_align_frame> fr((size_t)F);
  std::memset(fr.data(), 0, fr.size() * sizeof(esl_dense_align_frame));
  if (iter_out) std::memset(iter_out, 0, (size_t)F * np * kDalRow * sizeof(int64_t));
  int n_active = F, passes = 0;
  for (int it = 0; it < np && n_active > 0; ++it) {
    for (int f = 0; f < F; ++f) {
      if (flag[f] && !dense_pose(cam.data() + (size_t)f * 7, d.pose.data() + (size_t)f * kDensePose))
        return dense_fail(ESL_ERR_INVALID, who, "a pose with a non-finite number or a quaternion of norm 0");   // dal_update refuses these
    }
    if (const int rc = upload(c, s, DA_POSE, (const double*)d.pose.data(), (size_t)F * kDensePose * sizeof(double), &a.pose)) return rc;
    if (const int rc = upload(c, s, DA_FLAG, (const int*)flag.data(), (size_t)F * sizeof(int), &a.flag)) return rc;
    ESL_HIP_TRY(hipMemsetAsync(a.acc, 0, (size_t)F * kDalRow * sizeof(u64), c->stream));
    {
      ProfScope ps(c, 4);
      hipLaunchKernelGGL(k_dal_accum, dim3(dense_blocks((u64)per), (unsigned)std::min(F, 65535)), dim3(kDenseThreads), 0, c->stream, a);
    }
    ESL_HIP_TRY(hipGetLastError());
    ESL_HIP_TRY(hipMemcpyAsync(acc.data(), a.acc, (size_t)F * kDalRow * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    ++passes;
    // step d, frame by frame
    for (int f = 0; f < F; ++f) {
      if (!flag[f]) continue;
      const long long* row = acc.data() + (size_t)f * kDalRow;
      if (iter_out) std::memcpy(iter_out + ((size_t)f * np + it) * kDalRow, row, kDalRow * sizeof(int64_t));
      esl_dense_align_frame& r = fr[f];
      double H[36], g[6], delta[6];
      dal_system(row, H, g);
      bool stop = last[f] || it == p.iters;
      if (!stop) {
        int st = dal_solve(H, g, row[DAL_INLIER], p.min_inliers, p.damping, p.min_pivot_ratio, delta);
        double next[7];
        if (st == 0 && !dal_update(cam.data() + (size_t)f * 7, delta, next)) st = DAL_DEGENERATE;
        if (st != 0) { r.status = st; stop = true; }
        else {
          std::memcpy(cam.data() + (size_t)f * 7, next, sizeof(next));
          r.iters += 1; r.step_t = dal_norm3(delta); r.step_r = dal_norm3(delta + 3);
          if (dal_converged(delta, p.tol_t, p.tol_r)) { r.status = DAL_CONVERGED; last[f] = 1; }
        }
      }
      if (stop) {   // this pass was the frame's evaluation at its final pose
        r.n_sampled = row[DAL_SAMPLED]; r.n_zero = row[DAL_ZERO]; r.n_depth_out = row[DAL_DEPTH_OUT]; r.n_key_out = row[DAL_KEY_OUT];
        r.n_used = row[DAL_USED]; r.n_nomatch = row[DAL_NOMATCH]; r.n_far = row[DAL_FAR]; r.n_inlier = row[DAL_INLIER];
        r.sum_e2 = (double)row[27] / kDenseFix;
        std::memcpy(r.H, H, sizeof(H));
        flag[f] = 0; --n_active;
      }
    }
  }
  out->n_passes = passes;
  if (cams_out) std::memcpy(cams_out, cam.data(), (size_t)F * 7 * sizeof(double));
  if (frames_out) std::memcpy(frames_out, fr.data(), (size_t)F * sizeof(esl_dense_align_frame));
  return ESL_OK;
}
