// esl_capi.hip — C-ABI of libesl_hip.so (include/esl.h): context, work buffers, launches, LM drivers (graph residency: esl_graph.hip).
//
// Mapping mode (cameras fixed, the shipped setting): esl_optimize_resident enqueues the whole Levenberg-Marquardt run
// ahead of the device; the control flow of OptimizationAlgorithmLevenberg::solve
// (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-164) and SparseOptimizer::optimize
// (core/sparse_optimizer.cpp:354-419) runs in k_lm_step (esl_kernels_chunk.hpp), the host only watches a progress
// counter in mapped memory.  SLAM mode and the step API (esl_lm_*) keep the same statements on the host.  All arithmetic
// on states, residuals, Jacobians and normal equations runs in the HIP kernels of esl_kernels_*.hpp.  There is no CPU
// fallback: without a HIP device every compute entry point fails with ESL_ERR_NO_DEVICE.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "esl_graph_int.hpp"
#include "esl_graph_layout.hpp"
#include "esl_kernels_map.hpp"
#include "esl_kernels_chunk.hpp"
#include "esl_slam.hpp"
#include "esl_fixed.hpp"

namespace esl {
static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }
}  // namespace esl

using namespace esl;

namespace esl {
ProfScope::ProfScope(esl_ctx* ctx, int kind) : c(ctx), slot(-1) {
  if (!c || !c->prof_on) return;
  if (c->prof_level < 2 && (kind != 0 || !c->prof_gate)) return;
  if (c->prof_used + 2 > c->prof_ev.size()) {
    if (c->prof_ev.size() >= 16384) { prof_drain(c); }
    else {
      for (int i = 0; i < 512; ++i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; c->prof_ev.push_back(e); }
      c->prof_kind.resize(c->prof_ev.size() / 2);
    }
  }
  slot = (int)c->prof_used;
  c->prof_kind[slot / 2] = kind;
  c->prof_used += 2;
  (void)hipEventRecord(c->prof_ev[slot], c->stream);
}
ProfScope::~ProfScope() {
  if (slot >= 0) (void)hipEventRecord(c->prof_ev[slot + 1], c->stream);
}
int prof_drain(esl_ctx* c) {
  if (hipStreamSynchronize(c->stream) != hipSuccess) return ESL_ERR_HIP;
  for (size_t s = 0; s + 1 < c->prof_used; s += 2) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->prof_ev[s], c->prof_ev[s + 1]) == hipSuccess) {
      const int k = c->prof_kind[s / 2];
      c->prof_count[k]++;
      c->prof_ms[k] += ms;
    }
  }
  c->prof_used = 0;
  return ESL_OK;
}
}  // namespace esl

// ---- work buffers ---------------------------------------------------------------------------------
// Interior pointers of c->arena_work (grow-only, released with the context; free_graph only forgets them).
struct WorkStage {
  struct Fix { void** dst; size_t off; };
  size_t total = 0;
  std::vector<Fix> fixes;
  template <class T>
  void add(T** dst, size_t n) {
    const size_t off = layout::align_up(total, 256);
    total = off + std::max<size_t>(n, 1) * sizeof(T);
    fixes.push_back({(void**)dst, off});
  }
  int commit(esl_ctx* c) {
    int rc = arena_reserve(&c->arena_work, &c->arena_work_cap, std::max<size_t>(total, 256));
    if (rc) return rc;
    for (const Fix& f : fixes) *f.dst = c->arena_work + f.off;
    return ESL_OK;
  }
};
int esl::work_buffers(esl_ctx* c, size_t cap_objs, size_t cap_cams, size_t cap_chunks) {
  WorkStage wk;
  wk.add(&c->chunk_out, cap_chunks * kChunkOut); wk.add(&c->chunk_out2, cap_chunks * kChunkOut);
  wk.add(&c->chunk_chi, cap_chunks);
  wk.add(&c->blk_part, ((cap_objs + kStepWaves - 1) / kStepWaves + 2) * 2);   // k_chunk_finalize[_rows]: one pair per workgroup
  wk.add(&c->solve_part, ((cap_objs + kStepWaves - 1) / kStepWaves + (cap_objs + 63) / 64 + 2) * 4 * 2);   // k_obj_solve / k_lm_step* (x2: ping-pong)
  wk.add(&c->blk_chi, cap_chunks + 2);                 // <= one workgroup per chunk
  // states + mapping-mode system
  wk.add(&c->cams, cap_cams * 7); wk.add(&c->cams_trial, cap_cams * 7);
  wk.add(&c->objs, cap_objs * 10); wk.add(&c->objs_trial, cap_objs * 10);
  wk.add(&c->Hoo, cap_objs * 45); wk.add(&c->bo, cap_objs * 9); wk.add(&c->xo, cap_objs * 9); wk.add(&c->obj_part, cap_objs * 4);
  int rc = wk.commit(c);
  if (rc) return rc;
  ESL_HIP_TRY(hipMemsetAsync(c->obj_part, 0, std::max<size_t>(cap_objs, 1) * 4 * sizeof(double), c->stream));
  return ESL_OK;
}

extern "C" {

int esl_abi_version(void) { return ESL_ABI_VERSION; }
const char* esl_last_error(void) { return g_err.c_str(); }

int esl_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void esl_lm_params_default(esl_lm_params* p) {
  p->max_iters = 10;
  p->max_trials = 10;
  p->tau = 1e-5;
  p->jacobian_mode = ESL_JAC_NUMERIC;
  p->numeric_delta = 1e-9;
  p->linear_solver = ESL_SOLVER_AUTO;
  p->drop_nan_bbox = 1;
  p->bbox_residual = ESL_BBOX_REPROJECTION;
  p->e3d_half_turn = 0;
}

int esl_ctx_create(int device_id, esl_ctx** out) {
  if (!out) return ESL_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    set_error("no HIP device visible: libesl_hip has no CPU fallback");
    return ESL_ERR_NO_DEVICE;
  }
  if (device_id < 0 || device_id >= n) { set_error("device id out of range"); return ESL_ERR_INVALID; }
  ESL_HIP_TRY(hipSetDevice(device_id));
  esl_ctx* c = new esl_ctx();
  c->device = device_id;
  { const char* ov = std::getenv("ESL_CF_OVERLAP"); c->sw_cf_overlap = (ov && ov[0] >= '0' && ov[0] <= '4') ? ov[0] - '0' : 4; }
  { const char* ok = std::getenv("ESL_CF_OS_KERNEL"); c->sw_cf_os_kernel = (ok && ok[0] == '0') ? 0 : 1; }
  { const char* ol = std::getenv("ESL_CF_OS_LIST"); c->sw_cf_os_list = (ol && ol[0] == '0') ? 0 : 1; }
  { const char* sp = std::getenv("ESL_CF_SWEEP"); c->sw_cf_sweep = (sp && sp[0] == '0') ? 0 : 1; }
  { const char* fp = std::getenv("ESL_CF_FWD_PARTS"); const int v = fp ? std::atoi(fp) : 0; if (v == 2 || v == 4 || v == 8) c->sw_cf_fwd_parts = v; }
  { const char* sd = std::getenv("ESL_CF_STRIDE"); const int v = sd ? std::atoi(sd) : 0; c->sw_cf_stride = (v == 16 || v == 32 || v == 48) ? v : 0; }
  auto init = [&]() -> int {
    ESL_HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    ESL_HIP_TRY(hipHostMalloc((void**)&c->host_part, 16 * sizeof(double), hipHostMallocDefault));
    ESL_HIP_TRY(hipMalloc((void**)&c->dev_part, 16 * sizeof(double)));
    ESL_HIP_TRY(hipMalloc((void**)&c->chol_info, 4 * sizeof(int)));
    ESL_HIP_TRY(hipMemset(c->chol_info, 0, 4 * sizeof(int)));
    ESL_HIP_TRY(hipMalloc((void**)&c->tickets, 4 * sizeof(unsigned int)));
    ESL_HIP_TRY(hipMemset(c->tickets, 0, 4 * sizeof(unsigned int)));
    ESL_HIP_TRY(hipMalloc((void**)&c->dev_scal, 8 * sizeof(double)));
    ESL_HIP_TRY(hipEventCreateWithFlags(&c->ev_try, hipEventDisableTiming));
    ESL_HIP_TRY(hipHostMalloc(&c->host_scal, sizeof(LmScalars), hipHostMallocMapped));
    ESL_HIP_TRY(hipHostGetDevicePointer(&c->host_scal_dev, c->host_scal, 0));
    std::memset(c->host_scal, 0, sizeof(LmScalars));
    ESL_HIP_TRY(hipMalloc(&c->lm_dev, 2 * sizeof(LmCore)));   // ping-pong pair
    ESL_HIP_TRY(hipMemset(c->lm_dev, 0, 2 * sizeof(LmCore)));
    ESL_HIP_TRY(hipHostMalloc(&c->lm_host, sizeof(LmHostView), hipHostMallocMapped));
    ESL_HIP_TRY(hipHostGetDevicePointer(&c->lm_host_dev, c->lm_host, 0));
    std::memset(c->lm_host, 0, sizeof(LmHostView));
    return ESL_OK;
  };
  const int rc = init();
  if (rc) { const std::string msg = g_err; esl_ctx_destroy(c); set_error(msg); return rc; }   // a half-built context is released
  *out = c;
  return ESL_OK;
}

int esl_ctx_destroy(esl_ctx* c) {
  if (!c) return ESL_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);   // a trial may still be in flight (optimize_resident returns before the GPU is idle)
  slam_sync_side(c);
  free_graph(c);
  slam_release(c);
  if (c->arena_graph) (void)hipFree(c->arena_graph);
  if (c->arena_work) (void)hipFree(c->arena_work);
  if (c->stage_host) (void)hipHostFree(c->stage_host);
  if (c->append_dev) (void)hipFree(c->append_dev);
  if (c->slam_tab_dev) (void)hipFree(c->slam_tab_dev);
  c->eq_buf.release();
  if (c->fx_blob) (void)hipFree(c->fx_blob);
  c->chain_ws.release();
  fit_release(c);
  plane_release(c);
  reloc_release(c);
  assoc_release(c);
  merge_release(c);
  render_release(c);
  dense_release(c);
  init_batch_release(c);
  for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
  if (c->host_part) (void)hipHostFree(c->host_part);
  dev_free(&c->dev_part);
  dev_free(&c->chol_info);
  dev_free(&c->tickets); dev_free(&c->dev_scal);
  if (c->host_scal) (void)hipHostFree(c->host_scal);
  if (c->lm_host) (void)hipHostFree(c->lm_host);
  if (c->lm_dev) (void)hipFree(c->lm_dev);
  if (c->ev_try) (void)hipEventDestroy(c->ev_try);
  esl_comm_destroy(c);
  slam_release_runtime(c);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return ESL_OK;
}

// Release the grow-only SOLVER blobs of SLAM mode (the camera-first set: 19.8 GB at BASELINE configs[3]; the reduced camera system:
// 28.8 GB) -- and, when the resident graph has no free cameras, the SLAM list blob too.  The next trial step that needs one
// builds it again (index tables included).  Device pointers obtained from esl_lm_reduced_system die here.
int esl_ctx_trim(esl_ctx* c) {
  if (!c) return ESL_ERR_INVALID;
  ESL_HIP_TRY(hipSetDevice(c->device));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  slam_trim(c, c->graph_loaded && c->g.n_free_cams > 0);
  return ESL_OK;
}

int esl_debug_scratch_allocs(esl_ctx* c, int32_t owner, int64_t* allocs_out, int64_t* bytes_out) {
  if (!c || !allocs_out || !bytes_out || owner < ESL_SCRATCH_RELOC || owner > ESL_SCRATCH_INIT_ROBUST) {
    set_error("esl_debug_scratch_allocs: null pointer or unknown owner");
    return ESL_ERR_INVALID;
  }
  *allocs_out = 0; *bytes_out = 0;
  switch (owner) {
    case ESL_SCRATCH_RELOC: reloc_scratch_stats(c, allocs_out, bytes_out); break;
    case ESL_SCRATCH_ASSOC: assoc_scratch_stats(c, allocs_out, bytes_out); break;
    case ESL_SCRATCH_MERGE: merge_scratch_stats(c, allocs_out, bytes_out); break;
    case ESL_SCRATCH_RENDER: render_scratch_stats(c, allocs_out, bytes_out); break;
    default: init_scratch_stats(c, owner == ESL_SCRATCH_INIT_ROBUST, allocs_out, bytes_out);
  }
  return ESL_OK;
}

int esl_ctx_synchronize(esl_ctx* c) {
  if (!c) return ESL_ERR_INVALID;
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  return ESL_OK;
}

// ---------------------------------------------------------------------------------------------------
// chunked mapping-mode pipeline (esl_kernels_chunk.hpp): launch helpers
// ---------------------------------------------------------------------------------------------------
static ChunkTable chunk_table(const esl_ctx* c) {
  ChunkTable t;
  t.n_chunks = c->n_chunks; t.obj = c->ck_obj; t.type = c->ck_type; t.begin = c->ck_begin; t.end = c->ck_end; t.ostart = c->ck_ostart;
  return t;
}
// Linearise at `src_objs` into `dst_chunk` (defaults: the context's current estimate and chunk_out).
// st != null: the device-resident LM state picks the buffers instead -- the linearisation point is the TRIAL state of
// the pair (c->objs/chunk_out, c->objs_trial/chunk_out2) and the launch is a no-op once the run is done.
// validate: first linearisation of a device-driven run -- also performs the NaN pre-check of the bbox edges.
static int map_launch_linearize(esl_ctx* c, bool finalize, const double* src_objs = nullptr, double* dst_chunk = nullptr,
                                const LmCore* st = nullptr, bool validate = false) {
  const DevGraph& g = c->g;
  if (!src_objs) src_objs = c->objs;
  if (!dst_chunk) dst_chunk = c->chunk_out;
  const double* objs_b = st ? c->objs_trial : nullptr;
  double* chunk_b = st ? c->chunk_out2 : nullptr;
  if (st) { src_objs = c->objs; dst_chunk = c->chunk_out; }
  const ChunkTable ct = chunk_table(c);
  const bool an = c->lm.p.jacobian_mode == ESL_JAC_ANALYTIC;
  const int nb_e3 = (c->n_ids_e3 + 2 * kLinWaves - 1) / (2 * kLinWaves);   // two 32-edge chunks per wave
  const int nb_bb = (c->n_ids_bb + kLinWaves - 1) / kLinWaves;
  robust_dispatch(c->robust_on, [&](auto robust) {
    constexpr bool R = decltype(robust)::value;
    if (ct.n_chunks > 0) {
      ProfScope ps(c, 0);
      const dim3 block(64 * kLinWaves);
      int* cnt = c->chol_info + 2;
      if (an && g.bbox_mode) {   // plane-tangency rows instead of the reprojection residual (never NaN: nothing to validate, but the
                                 // flags are (re)set to valid by the VALIDATE instantiation)
        if (validate && g.check_vis)
          hipLaunchKernelGGL((k_chunk_linearize_both<ESL_JAC_ANALYTIC, 2, true, R>), dim3(nb_e3 + nb_bb), block, 0, c->stream, g, ct, c->ck_ids_e3,
                             c->n_ids_e3, nb_e3, c->ck_ids_bb, c->n_ids_bb, c->cams, src_objs, objs_b, c->lm.p.numeric_delta, dst_chunk,
                             chunk_b, c->blk_chi, st, cnt);
        else if (validate)
          hipLaunchKernelGGL((k_chunk_linearize_both<ESL_JAC_ANALYTIC, 1, true, R>), dim3(nb_e3 + nb_bb), block, 0, c->stream, g, ct, c->ck_ids_e3,
                             c->n_ids_e3, nb_e3, c->ck_ids_bb, c->n_ids_bb, c->cams, src_objs, objs_b, c->lm.p.numeric_delta, dst_chunk,
                             chunk_b, c->blk_chi, st, cnt);
        else
          hipLaunchKernelGGL((k_chunk_linearize_both<ESL_JAC_ANALYTIC, 0, true, R>), dim3(nb_e3 + nb_bb), block, 0, c->stream, g, ct, c->ck_ids_e3,
                             c->n_ids_e3, nb_e3, c->ck_ids_bb, c->n_ids_bb, c->cams, src_objs, objs_b, c->lm.p.numeric_delta, dst_chunk,
                             chunk_b, c->blk_chi, st, cnt);
      } else if (an) {   // both edge types in one launch, 3-D workgroups first
        if (validate && g.check_vis)
          hipLaunchKernelGGL((k_chunk_linearize_both<ESL_JAC_ANALYTIC, 2, false, R>), dim3(nb_e3 + nb_bb), block, 0, c->stream, g, ct, c->ck_ids_e3,
                             c->n_ids_e3, nb_e3, c->ck_ids_bb, c->n_ids_bb, c->cams, src_objs, objs_b, c->lm.p.numeric_delta, dst_chunk,
                             chunk_b, c->blk_chi, st, cnt);
        else if (validate)
          hipLaunchKernelGGL((k_chunk_linearize_both<ESL_JAC_ANALYTIC, 1, false, R>), dim3(nb_e3 + nb_bb), block, 0, c->stream, g, ct, c->ck_ids_e3,
                             c->n_ids_e3, nb_e3, c->ck_ids_bb, c->n_ids_bb, c->cams, src_objs, objs_b, c->lm.p.numeric_delta, dst_chunk,
                             chunk_b, c->blk_chi, st, cnt);
        else
          hipLaunchKernelGGL((k_chunk_linearize_both<ESL_JAC_ANALYTIC, 0, false, R>), dim3(nb_e3 + nb_bb), block, 0, c->stream, g, ct, c->ck_ids_e3,
                             c->n_ids_e3, nb_e3, c->ck_ids_bb, c->n_ids_bb, c->cams, src_objs, objs_b, c->lm.p.numeric_delta, dst_chunk,
                             chunk_b, c->blk_chi, st, cnt);
      } else {    // numeric Jacobians: one kernel per edge type (very different register needs), the long tasks first
        if (nb_e3 > 0)
          hipLaunchKernelGGL((k_chunk_linearize<ESL_JAC_NUMERIC, 1, 0, false, R>), dim3(nb_e3), block, 0, c->stream, g, ct, c->ck_ids_e3,
                             c->n_ids_e3, c->cams, src_objs, objs_b, c->lm.p.numeric_delta, dst_chunk, chunk_b, c->blk_chi, 0, st, cnt);
        if (nb_bb > 0) {
          auto launch_bb = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(nb_bb), block, 0, c->stream, g, ct, c->ck_ids_bb, c->n_ids_bb, c->cams, src_objs, objs_b,
                               c->lm.p.numeric_delta, dst_chunk, chunk_b, c->blk_chi, nb_e3, st, cnt);
          };
          const int vmode = !validate ? 0 : (g.check_vis ? 2 : 1);
          if (g.bbox_mode) { if (vmode == 2) launch_bb(k_chunk_linearize<ESL_JAC_NUMERIC, 0, 2, true, R>); else if (vmode == 1) launch_bb(k_chunk_linearize<ESL_JAC_NUMERIC, 0, 1, true, R>); else launch_bb(k_chunk_linearize<ESL_JAC_NUMERIC, 0, 0, true, R>); }
          else { if (vmode == 2) launch_bb(k_chunk_linearize<ESL_JAC_NUMERIC, 0, 2, false, R>); else if (vmode == 1) launch_bb(k_chunk_linearize<ESL_JAC_NUMERIC, 0, 1, false, R>); else launch_bb(k_chunk_linearize<ESL_JAC_NUMERIC, 0, 0, false, R>); }
        }
      }
    }
  });
  ESL_HIP_TRY(hipGetLastError());
  c->sys_combined = false;
  if (finalize) {
    ProfScope ps(c, 4);
    robust_dispatch(c->robust_on, [&](auto robust) {
      hipLaunchKernelGGL(k_chunk_finalize_rows<decltype(robust)::value>, dim3(std::max(1, (g.n_objs + kStepWaves - 1) / kStepWaves)), dim3(64 * kStepWaves), 0,
                         c->stream, g, ct, dst_chunk, src_objs, c->lm.p.jacobian_mode, c->lm.p.numeric_delta, c->blk_part,
                         c->tickets, c->dev_scal, (LmScalars*)c->host_scal_dev, c->lm.p.tau, (LmCore*)nullptr, (int*)nullptr, 0,
                         (LmHostView*)nullptr);
    });
    ESL_HIP_TRY(hipGetLastError());
  }
  return ESL_OK;
}
// solve (H + lambda I) x = b per ellipsoid from the chunk partials, retract -> objs_trial.
// lambda < 0: use tau * max_diag from device memory (first iteration)
static int map_launch_solve(esl_ctx* c, double lambda, const double* chunk = nullptr) {
  const DevGraph& g = c->g;
  if (!chunk) chunk = c->chunk_out;
  ProfScope ps(c, 1);
  robust_dispatch(c->robust_on, [&](auto robust) {
    hipLaunchKernelGGL(k_obj_solve<decltype(robust)::value>, dim3((g.n_objs + 63) / 64), dim3(64), 0, c->stream, g, chunk_table(c), chunk, c->objs,
                       c->lm.p.jacobian_mode, c->lm.p.numeric_delta, lambda,
                       c->lm.p.tau, c->dev_scal, c->xo, c->objs_trial, c->obj_part, c->solve_part);
  });
  ESL_HIP_TRY(hipGetLastError());
  return ESL_OK;
}
// solve + chi2 of the trial state with the residual-only kernels (step API / sharded loop: H, b of the trial are not wanted)
static int map_launch_try(esl_ctx* c, double lambda, const double* chunk = nullptr) {
  const DevGraph& g = c->g;
  const ChunkTable ct = chunk_table(c);
  int rc = map_launch_solve(c, lambda, chunk);
  if (rc) return rc;
  {
    ProfScope ps(c, 1);
    // 3-D chunks first (no reduction), then the bbox chunks whose last workgroup reduces everything
    robust_dispatch(c->robust_on, [&](auto robust) {
      constexpr bool R = decltype(robust)::value;
      if (c->n_ids_e3 > 0)
        hipLaunchKernelGGL((k_chunk_chi2<1, false, R>), dim3((c->n_ids_e3 + 7) / 8), dim3(256), 0, c->stream, g, ct, c->ck_ids_e3, c->n_ids_e3,
                           c->cams, c->objs_trial, c->obj_part, c->chunk_chi, c->tickets + 1, lambda, c->lm.p.tau, c->dev_scal,
                           (LmScalars*)c->host_scal_dev);
      hipLaunchKernelGGL((k_chunk_chi2<0, true, R>), dim3(std::max(1, (c->n_ids_bb + 3) / 4)), dim3(256), 0, c->stream, g, ct, c->ck_ids_bb,
                         c->n_ids_bb, c->cams, c->objs_trial, c->obj_part, c->chunk_chi, c->tickets + 1, lambda, c->lm.p.tau, c->dev_scal,
                         (LmScalars*)c->host_scal_dev);
    });
  }
  ESL_HIP_TRY(hipGetLastError());
  return ESL_OK;
}
static int map_combine(esl_ctx* c) {
  if (c->sys_combined || c->g.n_objs == 0) return ESL_OK;
  robust_dispatch(c->robust_on, [&](auto robust) {
    hipLaunchKernelGGL(k_chunk_combine<decltype(robust)::value>, dim3((c->g.n_objs * 54 + 255) / 256), dim3(256), 0, c->stream, c->g, chunk_table(c),
                       c->chunk_out, c->objs, c->lm.p.jacobian_mode, c->lm.p.numeric_delta, c->Hoo, c->bo);
  });
  ESL_HIP_TRY(hipGetLastError());
  c->sys_combined = true;
  return ESL_OK;
}

// ---------------------------------------------------------------------------------------------------
// step API
// ---------------------------------------------------------------------------------------------------
static int read_parts(esl_ctx* c, double out[4]) {
  if (c->parts_fresh) {   // (slam_try_step copied them together with the dense solver's flag: one wait per trial)
    c->parts_fresh = false;
    for (int i = 0; i < 4; ++i) out[i] = c->host_part[i];
    return ESL_OK;
  }
  ESL_HIP_TRY(hipMemcpyAsync(c->host_part, c->dev_part, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  for (int i = 0; i < 4; ++i) out[i] = c->host_part[i];
  return ESL_OK;
}

// the context's robust setting (esl_lm_set_robust) into the device graph: read at the start of every run
static void robust_to_graph(esl_ctx* c) {
  c->robust_on = false;
  for (int k = 0; k < ESL_EDGE_CLASSES; ++k) {
    c->g.rk_kind[k] = c->robust.kind[k];
    c->g.rk_delta[k] = c->robust.kind[k] != ESL_ROBUST_NONE ? c->robust.delta[k] : 1.0;
    c->robust_on = c->robust_on || c->robust.kind[k] != ESL_ROBUST_NONE;
  }
}

// NaN pre-check of the bbox edges at the start state (Optimizer.cpp:234-243); the dropped count stays on the device
// (c->chol_info + 2) -- the synchronous caller reads it back, the device-driven run lets k_chunk_finalize report it.
static int lm_begin_enqueue(esl_ctx* c, const esl_lm_params* p, bool validate_in_linearize = false) {
  if (!c->graph_loaded || !c->states_loaded) { set_error("esl_lm_begin: upload graph and states first"); return ESL_ERR_STATE; }
  ESL_HIP_TRY(hipSetDevice(c->device));
  c->lm.p = *p;
  c->g.bbox_mode = p->bbox_residual == ESL_BBOX_TANGENCY ? 1 : 0;
  c->g.yt.as_written = p->e3d_half_turn ? 1 : 0;
  robust_to_graph(c);
  c->pcg_run = c->pcg;   // (esl_lm_set_pcg: read when a run starts)
  c->pcg_reset = true;
  c->lm.slam = c->g.n_free_cams > 0;
  c->lm.have_trial = false;
  int* cnt = c->chol_info + 2;
  const bool validate = p->drop_nan_bbox != 0 || c->g.check_vis != 0;   // the visibility test rides on the NaN pre-check's pass
  if (validate_in_linearize && c->g.n_bbox && validate) {   // counter is zero: context creation, k_chunk_finalize, or esl_lm_begin's read-back
    c->lm.begun = true;
    return ESL_OK;
  }
  ESL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(int), c->stream));
  if (c->g.n_bbox) {
    if (validate) {
      hipLaunchKernelGGL(k_bbox_validate, dim3((c->g.n_bbox + 255) / 256), dim3(256), 0, c->stream, c->g, c->cams, c->objs, cnt);
      ESL_HIP_TRY(hipGetLastError());
    } else {
      ESL_HIP_TRY(hipMemsetAsync(c->g.bb_valid, 1, (size_t)c->g.n_bbox, c->stream));
    }
  }
  c->lm.begun = true;
  return ESL_OK;
}

int esl_lm_begin(esl_ctx* c, const esl_lm_params* p, int32_t* n_valid, int32_t* n_dropped) {
  if (!c || !p) return ESL_ERR_INVALID;
  // the replicated-graph promise is checked on the step API as well (once per uploaded graph; the same point of every rank's sequence)
  if (c->graph_loaded) { const int rcr = comm_check_replicated(c); if (rcr) return rcr; }
  int rc = lm_begin_enqueue(c, p);
  if (rc) return rc;
  int dropped = 0;
  if (c->g.n_bbox && (p->drop_nan_bbox || c->g.check_vis)) {
    ESL_HIP_TRY(hipMemcpyAsync(&dropped, c->chol_info + 2, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    // leave the counter at zero: a device-driven mapping run on this context counts into it without clearing it first
    ESL_HIP_TRY(hipMemsetAsync(c->chol_info + 2, 0, sizeof(int), c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  }
  if (c->fx_on && c->fx.n_bb) {   // the anchored bbox edges are active edges: same pre-check, same counters
    int adrop = 0;
    if (p->drop_nan_bbox || c->g.check_vis) {
      int* cnt = c->chol_info + 3;
      ESL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(int), c->stream));
      hipLaunchKernelGGL(k_anch_validate, dim3((c->fx.n_bb + 255) / 256), dim3(256), 0, c->stream, c->g, c->fx, c->cams, c->objs, cnt);
      ESL_HIP_TRY(hipGetLastError());
      ESL_HIP_TRY(hipMemcpyAsync(&adrop, cnt, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
      ESL_HIP_TRY(hipMemsetAsync(c->fx.bb_valid, 1, (size_t)c->fx.n_bb, c->stream));
    }
    if (n_valid) *n_valid = c->g.n_bbox_edges + c->fx.n_bb - dropped - adrop;
    if (n_dropped) *n_dropped = dropped + adrop;
    return ESL_OK;
  }
  if (n_valid) *n_valid = c->g.n_bbox_edges - dropped;
  if (n_dropped) *n_dropped = dropped;
  return ESL_OK;
}

int esl_lm_linearize(esl_ctx* c, esl_lm_partials* out) {
  if (!c || !out) return ESL_ERR_INVALID;
  if (!c->lm.begun) { set_error("esl_lm_linearize before esl_lm_begin"); return ESL_ERR_STATE; }
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (c->lm.slam) {
    int rc = slam_linearize(c);
    if (rc) return rc;
    double v[4];
    rc = (c->comm && !c->comm_replicated) ? comm_reduce4(c, c->dev_part, v) : read_parts(c, v);
    if (rc) return rc;
    out->chi2 = v[0]; out->max_diag = v[1]; out->scale = 0; out->solve_ok = 1; out->pad = 0;
    return ESL_OK;
  }
  int rc = map_launch_linearize(c, true);
  if (rc) return rc;
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  const LmScalars* h = (const LmScalars*)c->host_scal;
  out->chi2 = h->chi2_lin; out->max_diag = h->max_diag; out->scale = 0; out->solve_ok = 1; out->pad = 0;
  return ESL_OK;
}

int esl_lm_try_step(esl_ctx* c, double lambda, esl_lm_partials* out) {
  if (!c || !out) return ESL_ERR_INVALID;
  if (!c->lm.begun) { set_error("esl_lm_try_step before esl_lm_begin"); return ESL_ERR_STATE; }
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (c->lm.slam) {
    int rc = slam_try_step(c, lambda);
    if (rc) return rc;
    double v[4];
    rc = (c->comm && !c->comm_replicated) ? comm_reduce4(c, c->dev_part, v) : read_parts(c, v);
    if (rc) return rc;
    out->chi2 = v[0]; out->max_diag = 0; out->scale = v[2]; out->solve_ok = (c->g.n_objs == 0 || v[3] > 0.5) ? 1 : 0; out->pad = 0;
  } else {
    int rc = map_launch_try(c, lambda);
    if (rc) return rc;
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    const LmScalars* h = (const LmScalars*)c->host_scal;
    out->chi2 = h->chi2_trial; out->max_diag = 0; out->scale = h->scale; out->solve_ok = h->ok > 0.5 ? 1 : 0; out->pad = 0;
  }
  c->lm.lambda_used = lambda;
  c->lm.have_trial = true;
  return ESL_OK;
}

int esl_lm_commit(esl_ctx* c, int accept) {
  if (!c) return ESL_ERR_INVALID;
  if (!c->lm.begun || !c->lm.have_trial) { set_error("esl_lm_commit without a trial step"); return ESL_ERR_STATE; }
  if (accept) {  // discardTop: the trial states become the estimate
    std::swap(c->objs, c->objs_trial);
    if (c->lm.slam) { std::swap(c->cams, c->cams_trial); c->cams_match_snap = false; }
  }
  c->lm.have_trial = false;
  return ESL_OK;
}

int esl_lm_reduced_system(esl_ctx* c, double lambda, void** dev_ptr, int64_t* n, int64_t* lda) {
  if (!c || !dev_ptr || !n || !lda) return ESL_ERR_INVALID;
  if (!c->lm.begun) return ESL_ERR_STATE;
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (!c->lm.slam) { *dev_ptr = nullptr; *n = 0; *lda = 0; return ESL_OK; }
  *lda = c->S_lda;
  int rc = slam_build_reduced(c, lambda, true, dev_ptr, n);
  if (rc) return rc;
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  return ESL_OK;
}

// Mapping mode on one GPU: the whole LM run is enqueued ahead of the device.  One trial = two launches:
//   k_lm_step              decide the previous trial (accept / reject, lambda, stop test -- on the device), then solve
//                          per ellipsoid for the new lambda -> next trial state
//   k_chunk_linearize_*    linearisation AT the trial state: its chi2 sum is the trial's chi2 (no separate residual
//                          pass) and, if the trial gets accepted, its H, b are already the next iteration's system
// The host keeps a few trials queued, watches the progress counter in mapped memory and stops enqueueing when the
// device reports `done`; launches already queued behind a finished run exit at their first instruction.
static int optimize_mapping_device(esl_ctx* c, const esl_lm_params* p, esl_lm_report* out) {
  int rc;
  const DevGraph& g = c->g;
  LmHostView* hv = (LmHostView*)c->lm_host;
  LmCore* core = (LmCore*)c->lm_dev;   // [2]
  const bool sharded = c->comm != nullptr && !c->comm_replicated;   // collective run: every rank issues the same sequence of all-gathers
  if (!sharded && (g.n_objs == 0 || (g.n_bbox == 0 && g.n_e3d == 0 && c->n_grav_edges == 0))) {   // empty graph
    out->stop_reason = 3;
    return ESL_OK;
  }
  hv->trace_len = 0;
  __atomic_store_n(&hv->seq, 0, __ATOMIC_RELAXED);
  __atomic_store_n(&hv->done, 0, __ATOMIC_RELEASE);
  // linearisation of the start state + chi2, max diag, LM state initialisation (computeLambdaInit) into core[0]
  c->prof_gate = false;
  rc = map_launch_linearize(c, false, nullptr, nullptr, nullptr, g.n_bbox > 0 && (p->drop_nan_bbox != 0 || g.check_vis != 0));
  c->prof_gate = true;
  if (rc) return rc;
  {
    ProfScope ps(c, 4);
    robust_dispatch(c->robust_on, [&](auto robust) {
      hipLaunchKernelGGL(k_chunk_finalize_rows<decltype(robust)::value>, dim3(std::max(1, (g.n_objs + kStepWaves - 1) / kStepWaves)), dim3(64 * kStepWaves), 0,
                         c->stream, g, chunk_table(c), c->chunk_out, c->objs, c->lm.p.jacobian_mode, c->lm.p.numeric_delta, c->blk_part, c->tickets,
                         c->dev_scal, (LmScalars*)c->host_scal_dev, p->tau, sharded ? (LmCore*)nullptr : core, c->chol_info + 2, c->n_grav_edges,
                         (LmHostView*)c->lm_host_dev);
    });
    ESL_HIP_TRY(hipGetLastError());
  }
  if (sharded && (rc = comm_gather_scalars_device(c))) return rc;   // collective: every rank's {chi2, max diag, has_edges}
  if (p->max_iters <= 0) {   // nothing to iterate: report the start state
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    const LmScalars* h = (const LmScalars*)c->host_scal;
    out->chi2_initial = out->chi2_final = h->chi2_lin;
    out->n_bbox_dropped = hv->n_dropped;
    out->n_bbox_valid = g.n_bbox_edges - hv->n_dropped;
    if (hv->done) out->stop_reason = hv->core.stop_reason;
    return ESL_OK;
  }
  const bool sample_run = c->prof_on && c->prof_level == 1 && (c->prof_runs++ % 4 == 0);
  const int max_total = p->max_iters * std::max(1, p->max_trials);
  const int depth = 2;   // trials kept in flight ahead of the device's progress counter
  const int n_step_blocks = std::max(1, (g.n_objs + kStepWaves - 1) / kStepWaves);
  const int batch = 4;   // sharded: trials enqueued per round (a fixed number, so that all ranks issue the same collectives)
  const int n_lin_blocks = (c->n_ids_e3 + 2 * kLinWaves - 1) / (2 * kLinWaves) + (c->n_ids_bb + kLinWaves - 1) / kLinWaves;
  // launch k carries trial k's solve and trial k-1's decision: one launch more than there are trials
  int enq = 0, seen = 0;
  bool done = false;
  while (!done) {
    const int enq_limit = sharded ? enq + batch : max_total + 1;
    if (sharded && enq > max_total + batch) { set_error("device-side LM did not terminate"); return ESL_ERR_STATE; }
    while (enq < enq_limit && (sharded || enq - seen < depth)) {
      const LmCore* in = core + (enq & 1);
      LmCore* nxt = core + ((enq + 1) & 1);
      {
        ProfScope ps(c, 1);
        robust_dispatch(c->robust_on, [&](auto robust) {
          hipLaunchKernelGGL(k_lm_step_rows<decltype(robust)::value>, dim3(n_step_blocks), dim3(64 * kStepWaves), 0, c->stream, g, chunk_table(c), c->chunk_out,
                             c->chunk_out2, c->objs, c->objs_trial, in, nxt, c->blk_chi, n_lin_blocks, c->solve_part + 4 * n_step_blocks * (enq & 1),
                             c->solve_part + 4 * n_step_blocks * ((enq + 1) & 1), enq == 0 ? (sharded ? 2 : 1) : 0, p->max_iters, p->max_trials,
                             (LmHostView*)c->lm_host_dev, c->lm.p.jacobian_mode, c->lm.p.numeric_delta, c->xo,
                             sharded ? c->dev_gather : (const double*)nullptr, sharded ? c->comm_ranks : 0, p->tau);
        });
        ESL_HIP_TRY(hipGetLastError());
      }
      // the second trial's linearisation (always a live launch when it exists) of every FOURTH run is the sampled one: an event
      // pair splits two back-to-back dispatches and costs that trial ~20 us -- one per run was 10 % of a 0.2 ms run
      c->prof_gate = (enq == 1) && (sample_run);
      rc = map_launch_linearize(c, false, nullptr, nullptr, nxt);
      c->prof_gate = true;
      if (rc) return rc;
      if (sharded) {   // this rank's share of the trial's scalars, then everybody's (one small all-gather on the stream)
        hipLaunchKernelGGL(k_lm_partials, dim3(1), dim3(256), 0, c->stream, c->blk_chi, n_lin_blocks,
                           c->solve_part + 4 * n_step_blocks * ((enq + 1) & 1), n_step_blocks, c->dev_scal);
        ESL_HIP_TRY(hipGetLastError());
        ProfScope ps(c, 6);
        if ((rc = comm_gather_scalars_device(c))) return rc;
      }
      ++enq;
    }
    // wait for the device to decide at least one more trial (sharded: all but the last of the trials enqueued so far --
    // a condition every rank evaluates on the same sequence of decisions): spin on the mapped counter, fall back to a
    // stream sync
    const int want = sharded ? enq - 1 : seen + 1;
    int s = seen;
    for (int spin = 0; spin < 400000; ++spin) {
      s = __atomic_load_n(&hv->seq, __ATOMIC_ACQUIRE);
      if (s >= want || __atomic_load_n(&hv->done, __ATOMIC_ACQUIRE)) break;
    }
    if (s < want && !__atomic_load_n(&hv->done, __ATOMIC_ACQUIRE)) {
      ESL_HIP_TRY(hipStreamSynchronize(c->stream));
      s = __atomic_load_n(&hv->seq, __ATOMIC_ACQUIRE);
      if (s < want && !hv->done) { set_error("device-side LM made no progress"); return ESL_ERR_STATE; }
    }
    seen = s;
    done = __atomic_load_n(&hv->done, __ATOMIC_ACQUIRE) != 0;
  }
  // `done` was stored with release semantics after the results: they are visible without draining the stream (the
  // one or two no-op launches still queued touch nothing the caller can see)
  if (sharded) ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // leave no collective in flight behind the caller's back
  if (std::getenv("ESL_LM_TIMING")) {
    (void)hipStreamSynchronize(c->stream);
    fprintf(stderr, "[k_lm_step, workgroup 0, last live launch, us] decision=%.2f gather=%.2f solve=%.2f\n",
            (double)(hv->dbg_clk[1] - hv->dbg_clk[0]) * 0.01, (double)(hv->dbg_clk[2] - hv->dbg_clk[1]) * 0.01,
            (double)(hv->dbg_clk[3] - hv->dbg_clk[2]) * 0.01);
  }
  const LmCore& r = hv->core;
  out->n_bbox_dropped = hv->n_dropped;
  out->n_bbox_valid = g.n_bbox_edges - hv->n_dropped;
  if (r.cur) {   // the current estimate (and its system, for the inspection API) live in the second pair
    std::swap(c->objs, c->objs_trial);
    std::swap(c->chunk_out, c->chunk_out2);
  }
  c->sys_combined = false;
  c->lm.have_trial = false;
  out->iterations = r.it;
  out->total_trials = r.total_trials;
  out->stop_reason = r.stop_reason;
  out->chi2_initial = r.chi2_initial;
  out->chi2_final = r.currentChi;
  out->lambda_final = r.lambda;
  out->trace_len = hv->trace_len;
  for (int k = 0; k < hv->trace_len && k < ESL_MAX_TRACE; ++k) {
    out->trace_chi2[k] = hv->trace_chi2[k]; out->trace_lambda[k] = hv->trace_lambda[k]; out->trace_trials[k] = hv->trace_trials[k];
  }
  return ESL_OK;
}

int esl_optimize_resident(esl_ctx* c, const esl_lm_params* p, esl_lm_report* out) {
  if (!c || !p || !out) return ESL_ERR_INVALID;
  if (p->linear_solver != ESL_SOLVER_AUTO && p->linear_solver != ESL_SOLVER_REDUCED_CAMERA && p->linear_solver != ESL_SOLVER_REDUCED_ELLIPSOID &&
      p->linear_solver != ESL_SOLVER_CAMERA_CHAIN && p->linear_solver != ESL_SOLVER_PCG) {
    set_error("esl_lm_params::linear_solver: unknown solver"); return ESL_ERR_INVALID;
  }
  if (p->bbox_residual != ESL_BBOX_REPROJECTION && p->bbox_residual != ESL_BBOX_TANGENCY) { set_error("esl_lm_params::bbox_residual: unknown mode"); return ESL_ERR_INVALID; }
  if (p->e3d_half_turn != 0 && p->e3d_half_turn != 1) { set_error("esl_lm_params::e3d_half_turn: 0 (half turns not eligible) or 1 (as the reference writes it)"); return ESL_ERR_INVALID; }
  std::memset(out, 0, sizeof(*out));
  if (c->graph_loaded) { const int rcr = comm_check_replicated(c); if (rcr) return rcr; }
  if (c->graph_loaded && c->g.n_free_cams == 0) {   // mapping mode: the LM runs on the device, nothing waits on the host
    int rc0 = lm_begin_enqueue(c, p, true);
    if (rc0) return rc0;
    return optimize_mapping_device(c, p, out);
  }
  int32_t nv = 0, nd = 0;
  int rc = esl_lm_begin(c, p, &nv, &nd);
  if (rc) return rc;
  out->n_bbox_valid = nv;
  out->n_bbox_dropped = nd;
  const DevGraph& g = c->g;
  const bool any_edge = (nv > 0) || g.n_e3d > 0 || (g.n_odom > 0 && g.n_free_cams > 0) || (c->fx_on && c->fx.n_e3 > 0);
  bool any_grav = false;
  if (!any_edge) {  // gravity edges alone also make a graph
    std::vector<int> cnt((size_t)std::max(g.n_objs, 1));
    if (g.n_objs) ESL_HIP_TRY(hipMemcpy(cnt.data(), g.gr_cnt, (size_t)g.n_objs * sizeof(int), hipMemcpyDeviceToHost));
    for (int o = 0; o < g.n_objs; ++o) any_grav = any_grav || cnt[o] > 0;
  }
  if (!any_edge && !any_grav) { out->stop_reason = 3; return ESL_OK; }

  // SLAM mode (free cameras): host-driven LM over the step API -- each trial's dense factorisation dwarfs the host
  // round trip (optimization_algorithm_levenberg.cpp:69-141, statement for statement)
  double lambda = -1, ni = 2;
  int nBad = 0, it = 0, total_trials = 0;
  bool ok_outer = true;
  double currentChi = 0;
  for (it = 0; it < p->max_iters && ok_outer; ++it) {
    esl_lm_partials lin;
    if ((rc = esl_lm_linearize(c, &lin))) return rc;
    currentChi = lin.chi2;
    const double iniChi = currentChi;
    if (it == 0) {
      out->chi2_initial = currentChi;
      lambda = p->tau * lin.max_diag;  // computeLambdaInit
      ni = 2;
      nBad = 0;
    }
    double rho = 0;
    int qmax = 0;
    do {
      esl_lm_partials tr;
      if ((rc = esl_lm_try_step(c, lambda, &tr))) return rc;
      double tempChi = tr.solve_ok ? tr.chi2 : DBL_MAX;
      rho = (currentChi - tempChi) / (tr.scale + 1e-3);
      if (rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - std::pow((2 * rho - 1), 3);
        alpha = std::min(alpha, 2. / 3.);
        lambda *= std::max(1. / 3., alpha);
        ni = 2;
        currentChi = tempChi;
        if ((rc = esl_lm_commit(c, 1))) return rc;
      } else {
        lambda *= ni;
        ni *= 2;
        if ((rc = esl_lm_commit(c, 0))) return rc;
      }
      qmax++;
    } while (rho < 0 && qmax < p->max_trials);
    total_trials += qmax;
    if (it < ESL_MAX_TRACE) {
      out->trace_chi2[it] = currentChi; out->trace_lambda[it] = lambda; out->trace_trials[it] = qmax;
      out->trace_len = it + 1;
    }
    if (qmax == p->max_trials || rho == 0) { ok_outer = false; out->stop_reason = 1; }
    else {
      if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
      if (nBad >= 3) { ok_outer = false; out->stop_reason = 2; }
    }
  }
  out->iterations = it;
  out->total_trials = total_trials;
  out->chi2_final = currentChi;
  out->lambda_final = lambda;
  return ESL_OK;
}

int esl_optimize(esl_ctx* c, const esl_graph* g, double* cams_io, double* objs_io, const esl_lm_params* p,
                 esl_lm_report* out) {
  if (!c || !g || !p || !out) return ESL_ERR_INVALID;
  int rc;
  if ((rc = esl_graph_upload(c, g))) return rc;
  if ((rc = esl_states_upload(c, cams_io, objs_io))) return rc;
  if ((rc = esl_optimize_resident(c, p, out))) return rc;
  return esl_states_download(c, cams_io, objs_io);
}

int esl_optimize_fixed(esl_ctx* c, const esl_graph* g, const uint8_t* obj_fixed, double* cams_io, double* objs_io, const esl_lm_params* p,
                       esl_lm_report* out) {
  if (!c || !g || !p || !out) return ESL_ERR_INVALID;
  int rc;
  if ((rc = esl_graph_upload_fixed(c, g, obj_fixed))) return rc;
  if ((rc = esl_states_upload(c, cams_io, objs_io))) return rc;
  if ((rc = esl_optimize_resident(c, p, out))) return rc;
  return esl_states_download(c, cams_io, objs_io);
}

int esl_profile_enable(esl_ctx* c, int enable) {
  if (!c) return ESL_ERR_INVALID;
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (c->prof_on) prof_drain(c);
  c->prof_on = enable != 0;
  c->prof_level = enable;
  c->prof_runs = 0;
  for (int k = 0; k < ESL_PROF_KINDS; ++k) { c->prof_count[k] = 0; c->prof_ms[k] = 0; }
  return ESL_OK;
}

int esl_profile_get(esl_ctx* c, int64_t count[ESL_PROF_KINDS], double total_ms[ESL_PROF_KINDS]) {
  if (!c || !count || !total_ms) return ESL_ERR_INVALID;
  ESL_HIP_TRY(hipSetDevice(c->device));
  int rc = prof_drain(c);
  if (rc) return rc;
  for (int k = 0; k < ESL_PROF_KINDS; ++k) { count[k] = c->prof_count[k]; total_ms[k] = c->prof_ms[k]; }
  return ESL_OK;
}

int esl_lm_set_robust(esl_ctx* c, const esl_robust_params* p) {
  if (!c) return ESL_ERR_INVALID;
  esl_robust_params r = {{0, 0, 0, 0}, {1, 1, 1, 1}};
  if (p) {
    for (int k = 0; k < ESL_EDGE_CLASSES; ++k) {
      if (p->kind[k] < ESL_ROBUST_NONE || p->kind[k] > ESL_ROBUST_TUKEY) { set_error("esl_lm_set_robust: unknown kernel kind"); return ESL_ERR_INVALID; }
      if (p->kind[k] != ESL_ROBUST_NONE && !(std::isfinite(p->delta[k]) && p->delta[k] > 0)) {
        set_error("esl_lm_set_robust: delta must be finite and > 0"); return ESL_ERR_INVALID;
      }
    }
    r = *p;
  }
  c->robust = r;
  return ESL_OK;
}

void esl_pcg_params_default(esl_pcg_params* p) {
  p->max_iters = 1000;
  p->check_every = 8;
  p->rel_tol = 1e-10;
}

int esl_lm_set_pcg(esl_ctx* c, const esl_pcg_params* p) {
  if (!c) return ESL_ERR_INVALID;
  esl_pcg_params r;
  esl_pcg_params_default(&r);
  if (p) {
    if (p->max_iters < 1) { set_error("esl_lm_set_pcg: max_iters must be >= 1"); return ESL_ERR_INVALID; }
    if (p->check_every < 1) { set_error("esl_lm_set_pcg: check_every must be >= 1"); return ESL_ERR_INVALID; }
    if (!(std::isfinite(p->rel_tol) && p->rel_tol > 0)) { set_error("esl_lm_set_pcg: rel_tol must be finite and > 0"); return ESL_ERR_INVALID; }
    r = *p;
  }
  c->pcg = r;
  return ESL_OK;
}

static int edge_chi2_plain(esl_ctx* c, int32_t edge_class, double* chi2, double* weight, int64_t count);
// flagged graph: the free ellipsoids' edges from the ordinary path, the fixed ellipsoids' from k_anch_edge_chi2, merged in caller order
static int edge_chi2_fixed(esl_ctx* c, int32_t edge_class, double* chi2, double* weight, int64_t count) {
  const bool grav = edge_class == ESL_EDGE_GRAVITY;
  const std::vector<int>& map = edge_class == ESL_EDGE_BBOX ? c->fx_bb_map : c->fx_e3_map;
  const int64_t n_caller = grav ? (int64_t)c->fx_grav_obj.size() : (int64_t)map.size();
  if (count != n_caller) { set_error("esl_edge_chi2: count is not the class's edge count"); return ESL_ERR_INVALID; }
  if (count == 0) return ESL_OK;
  const size_t n_sub = grav ? c->h_grav_obj.size() : edge_class == ESL_EDGE_BBOX ? c->h_bb_slot_of.size() : c->h_e3_slot_of.size();
  std::vector<double> sc(n_sub), sw(n_sub);
  int rc = edge_chi2_plain(c, edge_class, sc.data(), sw.data(), (int64_t)n_sub);
  if (rc) return rc;
  DevGraph g = c->g;
  for (int k = 0; k < ESL_EDGE_CLASSES; ++k) { g.rk_kind[k] = c->robust.kind[k]; g.rk_delta[k] = c->robust.kind[k] ? c->robust.delta[k] : 1.0; }
  const int n_x = grav ? g.n_objs : edge_class == ESL_EDGE_BBOX ? c->fx.n_bb_all : c->fx.n_e3_all;
  std::vector<double> h((size_t)n_x * 2);
  if (n_x) {
    double* d = nullptr;
    ESL_HIP_TRY(hipMalloc((void**)&d, (size_t)n_x * 2 * sizeof(double)));
    hipLaunchKernelGGL(k_anch_edge_chi2, dim3((n_x + 255) / 256), dim3(256), 0, c->stream, g, c->fx, (int)edge_class, c->cams, c->objs, d, d + n_x);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) { set_error(std::string("esl_edge_chi2: ") + hipGetErrorString(e)); return ESL_ERR_HIP; }
  }
  size_t j = 0;
  for (int64_t i = 0; i < count; ++i) {
    double cv, wv;
    if (grav) {
      const int o = c->fx_grav_obj[(size_t)i];
      if (c->fx_flags[(size_t)o]) { cv = h[(size_t)o]; wv = 0; }
      else { cv = sc[j]; wv = sw[j]; ++j; }
    } else {
      const int m = map[(size_t)i];
      if (m >= 0) { cv = sc[(size_t)m]; wv = sw[(size_t)m]; }
      else { cv = h[(size_t)(-m - 1)]; wv = h[(size_t)n_x + (size_t)(-m - 1)]; }
    }
    if (chi2) chi2[i] = cv;
    if (weight) weight[i] = wv;
  }
  return ESL_OK;
}
int esl_edge_chi2(esl_ctx* c, int32_t edge_class, double* chi2, double* weight, int64_t count) {
  if (!c || edge_class < 0 || edge_class >= ESL_EDGE_CLASSES || count < 0) return ESL_ERR_INVALID;
  if (!c->graph_loaded || !c->states_loaded) { set_error("esl_edge_chi2: upload graph and states first"); return ESL_ERR_STATE; }
  if (c->fx_on && edge_class != ESL_EDGE_ODOM) { ESL_HIP_TRY(hipSetDevice(c->device)); return edge_chi2_fixed(c, edge_class, chi2, weight, count); }
  return edge_chi2_plain(c, edge_class, chi2, weight, count);
}
static int edge_chi2_plain(esl_ctx* c, int32_t edge_class, double* chi2, double* weight, int64_t count) {
  DevGraph g = c->g;   // the context's robust setting (the one its runs apply), residual settings of the last run
  for (int k = 0; k < ESL_EDGE_CLASSES; ++k) { g.rk_kind[k] = c->robust.kind[k]; g.rk_delta[k] = c->robust.kind[k] ? c->robust.delta[k] : 1.0; }
  const std::vector<int>* slot_of = edge_class == ESL_EDGE_BBOX ? &c->h_bb_slot_of : edge_class == ESL_EDGE_E3D ? &c->h_e3_slot_of
                                  : edge_class == ESL_EDGE_GRAVITY ? &c->h_grav_obj : nullptr;
  const int64_t n_caller = slot_of ? (int64_t)slot_of->size() : (int64_t)c->h_od_i.size();
  if (count != n_caller) { set_error("esl_edge_chi2: count is not the class's edge count"); return ESL_ERR_INVALID; }
  if (count == 0) return ESL_OK;
  const int n_slots = edge_class == ESL_EDGE_BBOX ? g.n_bbox : edge_class == ESL_EDGE_E3D ? g.n_e3d : edge_class == ESL_EDGE_GRAVITY ? g.n_objs : g.n_odom;
  ESL_HIP_TRY(hipSetDevice(c->device));
  const size_t need = (size_t)n_slots * 2;
  // grow-only: a query per frame allocates nothing once the graph has stopped growing
  if (const int rc = c->eq_buf.grow(c, 0, need * sizeof(double))) return rc;
  double* d = c->eq_buf.at<double>(0);
  std::vector<double> h(need);
  hipLaunchKernelGGL(k_edge_chi2, dim3((n_slots + 255) / 256), dim3(256), 0, c->stream, g, (int)edge_class, c->cams, c->objs, d, d + n_slots);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d, (size_t)n_slots * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { set_error(std::string("esl_edge_chi2: ") + hipGetErrorString(e)); return ESL_ERR_HIP; }
  for (int64_t i = 0; i < count; ++i) {   // slot -> caller order
    const int sl = slot_of ? (*slot_of)[(size_t)i] : (int)i;
    if (chi2) chi2[i] = h[(size_t)sl];
    if (weight) weight[i] = h[(size_t)n_slots + sl];
  }
  return ESL_OK;
}

int esl_lm_download(esl_ctx* c, int32_t which, double* dst, int64_t count) {
  if (!c || !dst || count < 0) return ESL_ERR_INVALID;
  if (!c->graph_loaded) { set_error("esl_lm_download: no graph"); return ESL_ERR_STATE; }
  const DevGraph& g = c->g;
  const double* src = nullptr;
  int64_t n = 0;
  switch (which) {
    case 0: src = c->Hoo; n = (int64_t)g.n_objs * 45; break;
    case 1: src = c->bo; n = (int64_t)g.n_objs * 9; break;
    case 2: src = c->xo; n = (int64_t)g.n_objs * 9; break;
    case 3: src = c->Hcc; n = (int64_t)g.n_free_cams * 36; break;
    case 4: src = c->bc; n = (int64_t)g.n_free_cams * 6; break;
    case 5: src = c->xc; n = (int64_t)g.n_free_cams * 6; break;
    case 6: src = c->S; n = c->S_lda * c->S_n; break;
    case 7: src = c->objs_trial; n = (int64_t)g.n_objs * 10; break;
    case 8: src = c->cams_trial; n = (int64_t)g.n_cams * 7; break;
    case 9:
      if (c->fx_on) { set_error("esl_lm_download: the W records are not available on a graph with fixed ellipsoids"); return ESL_ERR_STATE; }
      src = c->lm.slam ? c->Wbb : nullptr; n = ((int64_t)g.n_bbox + g.n_e3d) * 54; break;
    case 10:
      if (c->lm_solver_used != ESL_SOLVER_PCG || !c->pcg_M) { set_error("esl_lm_download: the last trial step did not run ESL_SOLVER_PCG"); return ESL_ERR_STATE; }
      src = c->pcg_M; n = (int64_t)g.n_free_cams * 36; break;
    default: set_error("esl_lm_download: unknown array"); return ESL_ERR_INVALID;
  }
  if (!src || count < n) { set_error("esl_lm_download: array not available or buffer too small"); return ESL_ERR_INVALID; }
  ESL_HIP_TRY(hipSetDevice(c->device));
  if ((which == 0 || which == 1) && !c->lm.slam && c->lm.begun) { int rc = map_combine(c); if (rc) return rc; }
  if (n) ESL_HIP_TRY(hipMemcpyAsync(dst, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  return ESL_OK;
}

// host-only: balanced partition of ellipsoids by edge count (greedy longest-processing-time)
int esl_partition_objects(const esl_graph* g, int32_t n_parts, int32_t* part_of_obj) {
  if (!g || n_parts <= 0 || (!part_of_obj && g->n_objs > 0)) return ESL_ERR_INVALID;
  int rc = validate_graph(g);
  if (rc) return rc;
  const int N = g->n_objs;
  std::vector<int64_t> load((size_t)N, 1);
  for (int i = 0; i < g->n_bbox; ++i) load[g->bbox_obj[i]] += 4;
  for (int i = 0; i < g->n_e3d; ++i) load[g->e3d_obj[i]] += 9;
  std::vector<int> order((size_t)N);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return load[a] > load[b]; });
  std::vector<int64_t> tot((size_t)n_parts, 0);
  for (int k = 0; k < N; ++k) {
    int best = 0;
    for (int q = 1; q < n_parts; ++q)
      if (tot[q] < tot[best]) best = q;
    part_of_obj[order[k]] = best;
    tot[best] += load[order[k]];
  }
  return ESL_OK;
}

}  // extern "C"

#ifdef ESL_ISA_PROBE
// scripts/isa_count.py compiles this TU with -DESL_ISA_PROBE to get the per-edge-type instruction streams of the
// fused linearisation kernel as separate symbols (analysis only; never part of libesl_hip.so).
namespace esl {
template __global__ void k_chunk_linearize<ESL_JAC_ANALYTIC, 0, false>(DevGraph, ChunkTable, const int*, int, const double*, const double*,
                                                                       const double*, double, double*, double*, double*, int,
                                                                       const LmCore*, int*);
template __global__ void k_chunk_linearize<ESL_JAC_ANALYTIC, 1, false>(DevGraph, ChunkTable, const int*, int, const double*, const double*,
                                                                       const double*, double, double*, double*, double*, int,
                                                                       const LmCore*, int*);
// and their robust twins (esl_lm_set_robust)
template __global__ void k_chunk_linearize<ESL_JAC_ANALYTIC, 0, 0, false, true>(DevGraph, ChunkTable, const int*, int, const double*, const double*,
                                                                                const double*, double, double*, double*, double*, int,
                                                                                const LmCore*, int*);
template __global__ void k_chunk_linearize<ESL_JAC_ANALYTIC, 1, 0, false, true>(DevGraph, ChunkTable, const int*, int, const double*, const double*,
                                                                                const double*, double, double*, double*, double*, int,
                                                                                const LmCore*, int*);
}  // namespace esl
#endif
