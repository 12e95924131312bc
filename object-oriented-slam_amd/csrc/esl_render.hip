// esl_render.hip — esl_render_map: the exact ray cast of every pixel against every ellipsoid of a map, nearest hit kept (include/esl.h,
// "rendering the map"; the steps' numbers below are the header's).
//   k_render_prep   one thread per (frame, object): steps 1 and 2 -- validity, Rco / tco from box_geom, the body A, g, c0 -- the flags, and
//                   the inclusive pixel bounds from box_from_conic's box (esl_render_ray.hpp render_bounds).  The bounds only cull.
//   k_render_tiles  one workgroup of 256 threads per 16 x 16 pixel tile per frame, one pixel per thread.  The workgroup streams its frame's
//                   records in chunks of 256: a thread tests one record's bounds against the tile, the survivors are compacted into LDS in
//                   ascending m (ballot per wave + the four wave counts, as phase A of k_assoc_frames), then every pixel walks the
//                   compacted chunk -- all lanes read the same entry, an LDS broadcast -- with step 3 and carries the running (z, m)
//                   minimum across the chunks.  The ray's monomials are formed once per pixel, so a test is eleven multiply-adds; the
//                   square root and the division are spent only on a hit that can still win (render_behind: a conservative bound, no
//                   bit of a result depends on it).  No capacity limit, no spill path.
//   counts          cover[0]: per compacted entry a ballot / popcount of the hits into an LDS integer, one global integer atomic per
//                   (tile, entry) with a non-zero count.  cover[1] and cmp: a pixel's winner is final only after the LAST chunk, when its
//                   LDS entry is gone, so the lanes of a wave that share a winner are found by ballot and their leader issues one global
//                   integer atomic per (wave, winner) and count.
// The only atomics are integer atomics: the counts are exact and order-free.  Ties of z go to the lowest m because the records are met in
// ascending m and the comparison is strict.  Everything lives in buffers of its own (esl_ctx::render) on the context's stream; the
// resident graph is only read.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "esl_ctx.hpp"
#include "esl_render_ray.hpp"

namespace esl {

static_assert(sizeof(esl_render_params) == 32, "include/esl.h states this size");
static_assert(sizeof(RenderRec) == 96, "ten doubles and four ints");

constexpr int kRenderThreads = 256;   // = the chunk of records = the pixels of a tile
constexpr int kRenderTile = 16;

struct RenderArgs {
  const double* cams; const double* objs;
  int F, M;
  double K[4];
  int rows, cols;
  const unsigned short* meas;
  double depth_scale, depth_min, depth_max, depth_tol;
  RenderRec* rec;
  double* depth; int* inst; int* cover; int* cmp; int* flags;   // null: not asked for
};

enum { RB_CAMS, RB_OBJS, RB_REC, RB_MEAS, RB_DEPTH, RB_INST, RB_COVER, RB_CMP, RB_FLAGS, RB_COUNT };
struct RenderState { ScratchSet<RB_COUNT> set; };

static __global__ __launch_bounds__(kRenderThreads) void k_render_prep(RenderArgs a) {
  const long long i = (long long)blockIdx.x * kRenderThreads + threadIdx.x;
  if (i >= (long long)a.F * a.M) return;
  const int f = (int)(i / a.M), m = (int)(i - (long long)f * a.M);
  const double* v = a.objs + (size_t)m * 10;
  RenderRec r;
  for (int k = 0; k < kRenderBody; ++k) r.b[k] = 0.0;
  r.x0 = 0; r.x1 = -1; r.y0 = 0; r.y1 = -1;
  double q[4], s[3];
  int flags = RENDER_INVALID;
  if (render_valid(v, q, s)) {
    Ell e;
    e.pose.t[0] = v[0]; e.pose.t[1] = v[1]; e.pose.t[2] = v[2];
    e.pose.r.x = q[0]; e.pose.r.y = q[1]; e.pose.r.z = q[2]; e.pose.r.w = q[3];
    e.s[0] = s[0]; e.s[1] = s[1]; e.s[2] = s[2];
    const SE3 Tcw = se3_load(a.cams + (size_t)f * 7);
    BoxGeom g;
    box_geom(Tcw, e, a.K, g);
    double bb[4], sq[2];
    box_from_conic(g, bb, sq);
    render_body(g.n, s, r.b);
    flags = render_bounds(bb, g.C22, g.n[3][2], r.b[9], a.rows, a.cols, r.x0, r.x1, r.y0, r.y1);
  }
  a.rec[i] = r;
  if (a.flags) a.flags[i] = flags;
}

// grid = (tiles along x, tiles along y, frames, at most 65535 of them: a workgroup takes the frames blockIdx.z, + gridDim.z, ...)
static __global__ __launch_bounds__(kRenderThreads) void k_render_tiles(RenderArgs a) {
  __shared__ double s_body[kRenderThreads * kRenderBody];   // 20 KB
  __shared__ int s_m[kRenderThreads], s_hits[kRenderThreads], s_cnt[8];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int X0 = blockIdx.x * kRenderTile, Y0 = blockIdx.y * kRenderTile;
  const int X1 = min(X0 + kRenderTile - 1, a.cols - 1), Y1 = min(Y0 + kRenderTile - 1, a.rows - 1);
  const int col = X0 + (tid & (kRenderTile - 1)), row = Y0 + (tid >> 4);   // a wave holds four rows of sixteen pixels
  const bool in_img = col < a.cols && row < a.rows;
  const RenderRay d = render_ray(a.K, col, row);
  const size_t npix = (size_t)a.rows * a.cols;
  for (int f = blockIdx.z; f < a.F; f += gridDim.z) {
    const RenderRec* rec = a.rec + (size_t)f * a.M;
    double best_z = __builtin_inf();
    int best_m = -1, it = 0;
    for (int m0 = 0; m0 < a.M; m0 += kRenderThreads, ++it) {
      __syncthreads();   // the chunk before is read and flushed
      const int m = m0 + tid;
      bool ok = false;
      if (m < a.M) {
        const RenderRec& r = rec[m];
        ok = r.x0 <= X1 && r.x1 >= X0 && r.y0 <= Y1 && r.y1 >= Y0;
      }
      const unsigned long long mask = __ballot(ok);
      int* cnt = s_cnt + (it & 1) * 4;
      if (lane == 0) cnt[wv] = __popcll(mask);
      s_hits[tid] = 0;
      __syncthreads();
      int off = 0, n = 0;
      for (int w = 0; w < 4; ++w) { const int c = cnt[w]; if (w < wv) off += c; n += c; }
      if (ok) {
        const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));   // pos < n <= 256
        const RenderRec& r = rec[m];
#pragma unroll
        for (int k = 0; k < kRenderBody; ++k) s_body[pos * kRenderBody + k] = r.b[k];
        s_m[pos] = m;
      }
      __syncthreads();
      for (int j = 0; j < n; ++j) {   // workgroup-uniform trip count; every lane reads entry j: a broadcast
        const double* body = s_body + j * kRenderBody;
        double beta, delta;
        const bool hit = in_img && render_hit_terms(body, d, beta, delta);
        if (a.cover) {
          const unsigned long long hm = __ballot(hit);
          if (lane == 0 && hm) atomicAdd(&s_hits[j], __popcll(hm));
        }
        if (hit && !render_behind(body[9], beta, delta, best_z)) {   // the root and the division only where the hit can win
          const double z = render_depth(body[9], beta, delta);
          if (z < best_z) { best_z = z; best_m = s_m[j]; }
        }
      }
      if (a.cover) {
        __syncthreads();
        if (tid < n && s_hits[tid]) atomicAdd(&a.cover[((size_t)f * a.M + s_m[tid]) * 2], s_hits[tid]);
      }
    }
    if (in_img) {   // sixteen consecutive pixels of a row per quarter wave
      const size_t px = (size_t)f * npix + (size_t)row * a.cols + col;
      if (a.depth) a.depth[px] = best_m >= 0 ? best_z : __builtin_nan("");
      if (a.inst) a.inst[px] = best_m;
    }
    if (a.cover || a.cmp) {
      int cat = 0;
      if (a.cmp && in_img && best_m >= 0)
        cat = render_compare(a.meas[(size_t)f * npix + (size_t)row * a.cols + col], best_z, a.depth_scale, a.depth_min, a.depth_max, a.depth_tol);
      bool pend = in_img && best_m >= 0;
      for (;;) {   // one round per distinct winner of the wave
        const unsigned long long pm = __ballot(pend);
        if (!pm) break;
        const int leader = __ffsll((long long)pm) - 1;
        const int wm = __shfl(best_m, leader, 64);
        const bool same = pend && best_m == wm;
        const unsigned long long sm = __ballot(same);
        unsigned long long cm[4] = {0, 0, 0, 0};
        if (a.cmp) {
#pragma unroll
          for (int k = 0; k < 4; ++k) cm[k] = __ballot(same && cat == k);
        }
        if (lane == leader) {
          const size_t o = (size_t)f * a.M + wm;
          if (a.cover) atomicAdd(&a.cover[o * 2 + 1], __popcll(sm));
          if (a.cmp) {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (cm[k]) atomicAdd(&a.cmp[o * 4 + k], __popcll(cm[k]));
          }
        }
        pend = pend && !same;
      }
    }
  }
}

void render_scratch_stats(const esl_ctx* c, int64_t* allocs, int64_t* bytes) {
  if (c->render) { *allocs = c->render->set.allocs(); *bytes = (int64_t)c->render->set.held(); }
}

void render_release(esl_ctx* c) {   // called by esl_ctx_destroy
  if (c->render) c->render->set.release();
  delete c->render;
  c->render = nullptr;
}

}  // namespace esl

using namespace esl;

namespace {

int render_invalid(const char* what) {
  set_error(std::string("esl_render_map: ") + what);
  return ESL_ERR_INVALID;
}

}  // namespace

extern "C" void esl_render_params_default(esl_render_params* p) {
  if (!p) return;
  p->depth_scale = 5000.0; p->depth_min = 0.1; p->depth_max = 6.0; p->depth_tol = 0.05;
}

extern "C" int esl_debug_render_allocs(esl_ctx* c, int64_t* allocs_out, int64_t* bytes_out) {
  return esl_debug_scratch_allocs(c, ESL_SCRATCH_RENDER, allocs_out, bytes_out);
}

extern "C" int esl_render_map(esl_ctx* c, const double* cams, int32_t F, const double* objs, int32_t M, const double K[4], int32_t rows,
                              int32_t cols, const uint16_t* depth_meas, const esl_render_params* pp, double* depth_out, int32_t* inst_out,
                              int32_t* cover_out, int32_t* cmp_out, int32_t* flags_out) {
  if (!c) return render_invalid("null ctx");
  if (F < 0) return render_invalid("negative F");
  if (M < 0) return render_invalid("negative M");
  if (!K) return render_invalid("null K");
  if (rows < 1 || rows > kRenderMaxDim) return render_invalid("rows < 1 or > 16384");
  if (cols < 1 || cols > kRenderMaxDim) return render_invalid("cols < 1 or > 16384");
  if (!std::isfinite(K[0]) || !(K[0] > 0)) return render_invalid("fx not finite or <= 0");
  if (!std::isfinite(K[1]) || !(K[1] > 0)) return render_invalid("fy not finite or <= 0");
  esl_render_params p;
  if (pp) p = *pp; else esl_render_params_default(&p);
  if (!std::isfinite(p.depth_scale) || !(p.depth_scale > 0)) return render_invalid("depth_scale not finite or <= 0");
  if (!std::isfinite(p.depth_min) || p.depth_min < 0) return render_invalid("depth_min not finite or negative");
  if (!std::isfinite(p.depth_max) || p.depth_max < 0) return render_invalid("depth_max not finite or negative");
  if (!std::isfinite(p.depth_tol) || p.depth_tol < 0) return render_invalid("depth_tol not finite or negative");
  if (p.depth_min > p.depth_max) return render_invalid("depth_min > depth_max");
  if (cmp_out && !depth_meas) return render_invalid("cmp_out needs depth_meas");
  if (const int rc = resident_source_check(c, "esl_render_map", !cams && F > 0, F, !objs && M > 0, M)) return rc;
  if (F == 0) return ESL_OK;
  if (!depth_out && !inst_out && !cover_out && !cmp_out && !flags_out) return ESL_OK;
  const size_t npix = (size_t)rows * cols, n_img = (size_t)F * npix, n_rec = (size_t)F * M;
  if (M == 0) {   // nothing to cast: the images are empty, the per-object outputs have no entries
    if (depth_out) std::fill(depth_out, depth_out + n_img, std::nan(""));
    if (inst_out) std::fill(inst_out, inst_out + n_img, -1);
    return ESL_OK;
  }
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (!c->render) c->render = new RenderState();
  ScratchSet<RB_COUNT>& s = c->render->set;
  RenderArgs k;
  std::memset(&k, 0, sizeof(k));
  if (const int rc = source(c, s, RB_CAMS, cams, c->cams, (size_t)F * 7 * sizeof(double), &k.cams)) return rc;
  if (const int rc = source(c, s, RB_OBJS, objs, c->objs, (size_t)M * 10 * sizeof(double), &k.objs)) return rc;
  if (const int rc = s.grow(c, RB_REC, n_rec * sizeof(RenderRec))) return rc;
  k.rec = s.at<RenderRec>(RB_REC);
  const bool tiles = depth_out || inst_out || cover_out || cmp_out;   // flags alone need the prepare kernel only
  if (cmp_out) {
    if (const int rc = upload(c, s, RB_MEAS, depth_meas, n_img * sizeof(uint16_t), &k.meas)) return rc;
    if (const int rc = s.grow(c, RB_CMP, n_rec * 4 * sizeof(int32_t))) return rc;
    k.cmp = s.at<int>(RB_CMP);
    ESL_HIP_TRY(hipMemsetAsync(k.cmp, 0, n_rec * 4 * sizeof(int32_t), c->stream));
  }
  if (depth_out) {
    if (const int rc = s.grow(c, RB_DEPTH, n_img * sizeof(double))) return rc;
    k.depth = s.at<double>(RB_DEPTH);
  }
  if (inst_out) {
    if (const int rc = s.grow(c, RB_INST, n_img * sizeof(int32_t))) return rc;
    k.inst = s.at<int>(RB_INST);
  }
  if (cover_out) {
    if (const int rc = s.grow(c, RB_COVER, n_rec * 2 * sizeof(int32_t))) return rc;
    k.cover = s.at<int>(RB_COVER);
    ESL_HIP_TRY(hipMemsetAsync(k.cover, 0, n_rec * 2 * sizeof(int32_t), c->stream));
  }
  if (flags_out) {
    if (const int rc = s.grow(c, RB_FLAGS, n_rec * sizeof(int32_t))) return rc;
    k.flags = s.at<int>(RB_FLAGS);
  }
  k.F = F; k.M = M; k.rows = rows; k.cols = cols;
  for (int i = 0; i < 4; ++i) k.K[i] = K[i];
  k.depth_scale = p.depth_scale; k.depth_min = p.depth_min; k.depth_max = p.depth_max; k.depth_tol = p.depth_tol;
  {
    ProfScope ps(c, 4);
    hipLaunchKernelGGL(k_render_prep, dim3((unsigned)((n_rec + kRenderThreads - 1) / kRenderThreads)), dim3(kRenderThreads), 0, c->stream, k);
    if (tiles) {
      const dim3 grid((unsigned)((cols + kRenderTile - 1) / kRenderTile), (unsigned)((rows + kRenderTile - 1) / kRenderTile),
                      (unsigned)std::min(F, 65535));
      hipLaunchKernelGGL(k_render_tiles, grid, dim3(kRenderThreads), 0, c->stream, k);
    }
  }
  ESL_HIP_TRY(hipGetLastError());
  if (depth_out) ESL_HIP_TRY(hipMemcpyAsync(depth_out, k.depth, n_img * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (inst_out) ESL_HIP_TRY(hipMemcpyAsync(inst_out, k.inst, n_img * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (cover_out) ESL_HIP_TRY(hipMemcpyAsync(cover_out, k.cover, n_rec * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (cmp_out) ESL_HIP_TRY(hipMemcpyAsync(cmp_out, k.cmp, n_rec * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (flags_out) ESL_HIP_TRY(hipMemcpyAsync(flags_out, k.flags, n_rec * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's arrays are free again, the outputs filled
  return ESL_OK;
}
