// esl_slam.hip — host orchestration of SLAM mode (free cameras): linearise, Schur complement onto the
// cameras, dense FP64-MFMA Cholesky of the reduced camera system, back-substitution, trial states.
// See esl_kernels_slam.hpp for the maths and the reference citations.
#include "esl_slam.hpp"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "esl_cf.hpp"
#include "esl_cf_sweep.hpp"
#include "esl_chol.hpp"
#include "esl_fixed.hpp"
#include "esl_kernels_slam.hpp"
#include "esl_pcg.hpp"

namespace esl {

// trial ellipsoids AND trial cameras of the camera-first form in one launch (round 6): blocks [0, nb_obj) are k_cf_obj_update's, the
// rest k_slam_cam_update's
static __global__ __launch_bounds__(256) void k_cf_updates(DevGraph g, int nb_obj, double lambda, const double* __restrict__ objs, const double* __restrict__ bo,
                                                           const double* __restrict__ xo, double* __restrict__ objs_trial, double* __restrict__ obj_part,
                                                           const double* __restrict__ cams, const double* __restrict__ xc, const double* __restrict__ bc,
                                                           double* __restrict__ cams_trial, double* __restrict__ cam_part) {
  if ((int)blockIdx.x < nb_obj) cf_obj_update_one(g, lambda, objs, bo, xo, objs_trial, obj_part, blockIdx.x * 256 + threadIdx.x);
  else slam_cam_update_one(g, lambda, cams, xc, bc, cams_trial, cam_part, ((int)blockIdx.x - nb_obj) * 256 + threadIdx.x);
}

template <class T>
static int al(T** dst, size_t n) {
  if (*dst) { (void)hipFree(*dst); *dst = nullptr; }
  ESL_HIP_TRY(hipMalloc((void**)dst, std::max<size_t>(n, 1) * sizeof(T)));
  return ESL_OK;
}

// ---- grow-only blobs of SLAM mode (round 4) -------------------------------------------------------------------------------
// Rounds 2-3 gave every table and work buffer of SLAM mode its own hipFree + hipMalloc + pageable copy at every upload (~40 of
// them) and freed the solver's multi-GB buffers with the graph: 21 ms per esl_graph_upload at BASELINE configs[3], paid by every
// esl_optimize call of the drop-in adapter.  Now BlobArenas (esl_ctx.hpp): arena_slam holds what slam_alloc makes at upload,
// arena_solve what the first camera-first trial step needs (tables + slabs + T), arena_S the reduced camera system (round 5: a blob
// of its own, so that esl_lm_reduced_system beside a camera-first run no longer re-lays out that form).  A BlobStage plans a layout
// (256-byte aligned items, uploads first), grows the arena and its pinned staging blob when needed, lets the caller build the
// uploaded tables IN the staging blob, and ships them with one copy.  Pointers handed out are interior pointers: never hipFree()d,
// only forgotten (slam_forget) -- the arenas live until the context is destroyed (slam_release).
namespace {
struct BlobStage {
  struct Item { void** dst; size_t bytes, off; bool upload; };
  std::vector<Item> items;
  size_t total = 0, up_end = 0;
  BlobArena* a = nullptr;
  template <class T> int up(T** dst, size_t n) { return add((void**)dst, n * sizeof(T), true); }      // -> item index
  template <class T> int work(T** dst, size_t n) { return add((void**)dst, n * sizeof(T), false); }
  int add(void** dst, size_t bytes, bool upload) {
    const size_t off = (total + 255) / 256 * 256;
    items.push_back({dst, bytes, off, upload});
    total = off + std::max<size_t>(bytes, 8);
    if (upload) up_end = total;
    return (int)items.size() - 1;
  }
  // grows the arena / the staging blob; afterwards host<T>(i) is where item i's table is to be built
  int reserve(BlobArena& arena) {
    a = &arena;
    if (a->ev) ESL_HIP_TRY(hipEventSynchronize(a->ev));   // the previous blob's copy still reads the staging memory
    else ESL_HIP_TRY(hipEventCreateWithFlags(&a->ev, hipEventDisableTiming));
    if (up_end > a->host_cap) {
      if (a->host) { (void)hipHostFree(a->host); a->host = nullptr; a->host_cap = 0; }
      const size_t want = up_end + up_end / 2 + 4096;
      ESL_HIP_TRY(hipHostMalloc((void**)&a->host, want, hipHostMallocDefault));
      a->host_cap = want;
    }
    if (total > a->cap) {
      if (a->dev) { (void)hipFree(a->dev); a->dev = nullptr; a->cap = 0; }
      // growth slack only where it is cheap: 12.5 % of the 28.8 GB reduced camera system of BASELINE configs[3] is 3.6 GB that can turn
      // a fit into an out-of-memory; blobs of that size are sized by ONE graph shape, not by a growing sequence of them
      const size_t want = total + (total < ((size_t)1 << 30) ? total / 8 : 0) + 4096;
      ESL_HIP_TRY(hipMalloc((void**)&a->dev, want));
      a->cap = want;
    }
    for (const Item& it : items) *it.dst = a->dev + it.off;
    return ESL_OK;
  }
  template <class T> T* host(int i) const { return (T*)(a->host + items[(size_t)i].off); }
  int ship(hipStream_t st) {
    if (up_end) ESL_HIP_TRY(hipMemcpyAsync(a->dev, a->host, up_end, hipMemcpyHostToDevice, st));
    ESL_HIP_TRY(hipEventRecord(a->ev, st));
    return ESL_OK;
  }
};
double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

static void cf_forget(esl_ctx* c);
// the graph goes away: every interior pointer is forgotten, the arenas stay (esl_graph.hip free_graph)
void slam_forget(esl_ctx* c) {
  DevGraph& g = c->g;
  g.ue_start = g.ue_id = g.ue_slot = g.cu_start = g.cu_obj = g.cu_id = nullptr;
  c->Hcc = c->bc = c->xc = c->Wbb = c->Abb = c->Aod = c->Dinv = c->Yb = c->Wt = c->Tb = c->cam_part = c->od_part = c->z_ws = nullptr;
  c->cf_od_start = c->cf_od_edge = nullptr;
  c->S = c->Linv_ws = nullptr;
  c->pcg_M = nullptr;   // (sized by the graph that goes away: esl_lm_download(10) needs a PCG trial on the new one)
  cf_forget(c);
  c->cf_chain_ok = false; c->cf_unavailable = false; c->chain_ok = false;
  c->h_ue_start.clear(); c->h_ue_id.clear(); c->h_ue_slot.clear();
  c->h_cu_start = c->h_cu_obj = c->h_cu_id = nullptr;
}
static void blob_release(BlobArena& a) {
  if (a.dev) (void)hipFree(a.dev);
  if (a.host) (void)hipHostFree(a.host);
  if (a.ev) (void)hipEventDestroy(a.ev);
  a = BlobArena{};
}
static void pcg_release(esl_ctx* c) {
  if (c->pcg_ws) (void)hipFree(c->pcg_ws);
  if (c->pcg_host) (void)hipHostFree(c->pcg_host);
  c->pcg_ws = c->pcg_st = c->pcg_M = c->pcg_host = nullptr; c->pcg_ws_cap = 0; c->pcg_ran = false;
}
void slam_release(esl_ctx* c) { slam_forget(c); blob_release(c->arena_slam); blob_release(c->arena_solve); blob_release(c->arena_S); pcg_release(c); }
// esl_ctx_trim: drop the solver blobs (tens of GB at BASELINE configs[3]); the next trial step that needs one builds it again.
// keep_lists: the resident graph has free cameras, so arena_slam (its lists, W, Y ...) is still in use.
void slam_trim(esl_ctx* c, bool keep_lists) {
  slam_sync_side(c);   // (every trial joins the side stream to the context's stream, which the callers have waited for: a host wait of its own
                       //  before what it reads is freed)
  cf_forget(c);
  c->S = c->Linv_ws = nullptr;
  c->cf_unavailable = false;
  blob_release(c->arena_solve); blob_release(c->arena_S);
  if (!keep_lists) { slam_forget(c); blob_release(c->arena_slam); }
}

// SLAM-mode lists of a freshly uploaded graph + its per-graph work buffers.  All lists come out of counting sorts (no comparison
// sort: the per-ellipsoid order "ascending u" falls out of walking the edge arrays in order, "ascending (slot, u)" out of walking
// the per-camera lists in slot order).
int slam_alloc(esl_ctx* c) {
  DevGraph& g = c->g;
  const int N = g.n_objs, F = g.n_cams, nf = g.n_free_cams;
  const bool timing = std::getenv("ESL_UPLOAD_HOST_TIMING") != nullptr;
  const double t0 = timing ? now_us() : 0;
  // unified per-ellipsoid list of edges whose camera is free (u = bounding-box edge i, or n_bbox + 3-D edge i), ascending u
  std::vector<int>& start = c->h_ue_start;
  std::vector<int>& id = c->h_ue_id;
  std::vector<int>& slot = c->h_ue_slot;
  start.assign((size_t)N + 1, 0);
  // (appendable layout, esl_graph_append in SLAM mode: the arrays have slack behind every ellipsoid's slice -- free slots carry obj = -1)
  for (int i = 0; i < g.n_bbox; ++i) if (c->h_bb_obj[i] >= 0 && c->h_cam_slot[c->h_bb_cam[i]] >= 0) ++start[(size_t)c->h_bb_obj[i] + 1];
  for (int i = 0; i < g.n_e3d; ++i) if (c->h_e3_obj[i] >= 0 && c->h_cam_slot[c->h_e3_cam[i]] >= 0) ++start[(size_t)c->h_e3_obj[i] + 1];
  for (int o = 0; o < N; ++o) start[(size_t)o + 1] += start[o];
  const size_t nue = (size_t)start[N];
  id.resize(nue); slot.resize(nue);
  {
    std::vector<int> cur(start.begin(), start.end() - 1);
    for (int i = 0; i < g.n_bbox; ++i) {
      if (c->h_bb_obj[i] < 0) continue;
      const int s = c->h_cam_slot[c->h_bb_cam[i]];
      if (s >= 0) { const int at = cur[c->h_bb_obj[i]]++; id[at] = i; slot[at] = s; }
    }
    for (int i = 0; i < g.n_e3d; ++i) {
      if (c->h_e3_obj[i] < 0) continue;
      const int s = c->h_cam_slot[c->h_e3_cam[i]];
      if (s >= 0) { const int at = cur[c->h_e3_obj[i]]++; id[at] = g.n_bbox + i; slot[at] = s; }
    }
  }
  g.n_ue = (int)nue;
  // odometry edges of every pair of neighbouring slots (the camera chain of esl_cf.hpp): the camera-first form applies when ALL
  // odometry edges between free cameras join neighbours.  (Its other tables are built by the first trial step that picks it.)
  std::vector<int> ods((size_t)std::max(nf, 1) + 1, 0), ode;
  bool chain = true;
  {
    std::vector<std::pair<int, int>> pe;   // (lower slot, 2 e + orientation)
    for (int e = 0; e < g.n_odom; ++e) {
      const int si = c->h_cam_slot[c->h_od_i[e]], sj = c->h_cam_slot[c->h_od_j[e]];
      if (si < 0 || sj < 0) continue;                       // a fixed end: the edge only adds to the free end's diagonal block
      if (si == sj + 1) pe.push_back({sj, e * 2});          // rows = first vertex = the higher slot: B as stored
      else if (sj == si + 1) pe.push_back({si, e * 2 + 1});
      else chain = false;                                   // (si == sj: a self edge; |si - sj| > 1: fill-in outside the band)
    }
    for (auto& p : pe) ++ods[(size_t)p.first + 1];
    for (int k = 0; k < nf; ++k) ods[(size_t)k + 1] += ods[k];
    ode.resize(pe.size());
    std::vector<int> cur(ods.begin(), ods.end() - 1);
    for (auto& p : pe) ode[(size_t)cur[p.first]++] = p.second;   // (edges of one pair stay in ascending e)
  }
  c->cf_chain_ok = chain && nf > 0 && N > 0;
  c->chain_ok = chain && nf > 0;
  const double t1 = timing ? now_us() : 0;
  // layout: uploads first, then the work buffers
  const size_t EU = (size_t)g.n_bbox + g.n_e3d;
  const int64_t n = 6 * (int64_t)nf;
  c->S_n = n;
  c->S_lda = ((n + 1 + 127) / 128) * 128;   // (whole 128-row tiles for the update kernels: chol_update_tile_v reads pad rows instead of guarding the last tile row)
  BlobStage st;
  const int i_ust = st.up(&g.ue_start, start.size()), i_uid = st.up(&g.ue_id, nue), i_usl = st.up(&g.ue_slot, nue);
  const int i_cst = st.up(&g.cu_start, (size_t)nf + 1), i_cob = st.up(&g.cu_obj, nue), i_cid = st.up(&g.cu_id, nue);
  const int i_ods = st.up(&c->cf_od_start, ods.size()), i_ode = st.up(&c->cf_od_edge, ode.size());
  st.work(&c->Hcc, (size_t)nf * 36); st.work(&c->bc, (size_t)nf * 6);
  st.work(&c->Wbb, EU * 54);    // unified W  [54][EU]
  st.work(&c->Abb, EU * 27);    // unified A  [EU][27] (per-edge records)
  st.work(&c->Yb, EU * 54);     // unified Y  [EU][54]
  st.work(&c->Wt, EU * 54);     // W once more as per-edge records [EU][9][6]: what k_slam_schur_pull gathers
  st.work(&c->Tb, EU * 6);      // Y_e b_o    [6][EU]
  st.work(&c->Aod, (size_t)g.n_odom * 90); st.work(&c->Dinv, (size_t)N * 81);
  st.work(&c->cam_part, (size_t)F * 4); st.work(&c->od_part, (size_t)g.n_odom);
  st.work(&c->xc, (size_t)n); st.work(&c->z_ws, (size_t)kNB);
  if (int rc = st.reserve(c->arena_slam)) return rc;
  std::memcpy(st.host<int>(i_ust), start.data(), start.size() * sizeof(int));
  if (nue) { std::memcpy(st.host<int>(i_uid), id.data(), nue * sizeof(int)); std::memcpy(st.host<int>(i_usl), slot.data(), nue * sizeof(int)); }
  std::memcpy(st.host<int>(i_ods), ods.data(), ods.size() * sizeof(int));
  if (!ode.empty()) std::memcpy(st.host<int>(i_ode), ode.data(), ode.size() * sizeof(int));
  // the same edges per free camera, sorted by (ellipsoid, u): two of these lists are intersected per block of S.  Walking the
  // unified list in order (ellipsoids ascending, u ascending inside one) keeps every camera's list sorted.
  {
    int* cstart = st.host<int>(i_cst); int* cobj = st.host<int>(i_cob); int* cid = st.host<int>(i_cid);
    c->h_cu_start = cstart; c->h_cu_obj = cobj; c->h_cu_id = cid;   // (staging memory: valid until the next upload; cf_ensure_impl reads them)
    std::fill(cstart, cstart + nf + 1, 0);
    for (size_t k = 0; k < nue; ++k) ++cstart[(size_t)slot[k] + 1];
    g.cu_max = 0;
    for (int s = 0; s < nf; ++s) { g.cu_max = std::max(g.cu_max, cstart[(size_t)s + 1]); cstart[(size_t)s + 1] += cstart[s]; }
    std::vector<int> cur(cstart, cstart + nf);
    for (int o = 0; o < N; ++o)
      for (int k = start[o]; k < start[(size_t)o + 1]; ++k) { const int at = cur[slot[k]]++; cobj[at] = o; cid[at] = id[k]; }
  }
  if (int rc = st.ship(c->stream)) return rc;
  // W / A of edges that are never written (fixed camera) must not hold NaN garbage where they are summed
  ESL_HIP_TRY(hipMemsetAsync(c->Abb, 0, std::max<size_t>(EU, 1) * 27 * sizeof(double), c->stream));
  ESL_HIP_TRY(hipMemsetAsync(c->Wbb, 0, std::max<size_t>(EU, 1) * 54 * sizeof(double), c->stream));
  if (timing) {
    const double t2 = now_us();
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    fprintf(stderr, "[slam_alloc host, us] lists %.0f  layout + per-camera lists + enqueue %.0f  wait %.0f  (blob %.1f MB uploaded, %.1f MB in all)\n",
            t1 - t0, t2 - t1, now_us() - t2, st.up_end / 1e6, st.total / 1e6);
  }
  return ESL_OK;
}

static CholRuntime& chol_rt(esl_ctx* c);
static __global__ void k_info_to_double(const int* __restrict__ info, double* __restrict__ d) { d[0] = info[0] ? 1.0 : 0.0; }
static __global__ void k_double_to_info(const double* __restrict__ d, int* __restrict__ info) { if (d[0] > 0.5) info[0] |= 1; }
// the reduced camera system S (28.8 GB at C4) lives in a grow-only blob of its own, kept from graph to graph (esl_ctx_trim drops
// it); the pointer esl_lm_reduced_system hands out stays valid until the next graph upload, trim or context destroy -- its
// CONTENT only until the next trial step that factors S in place
static int slam_ensure_S(esl_ctx* c) {
  if (c->S) return ESL_OK;
  const size_t n = (size_t)c->S_n, np = (n + kNB - 1) / kNB;
  BlobStage st;
  st.work(&c->S, (size_t)c->S_lda * n); st.work(&c->Linv_ws, np * kNB * kNB);
  const int rc = st.reserve(c->arena_S);
  if (rc) { c->S = c->Linv_ws = nullptr; return rc; }
  return st.ship(c->stream);
}

// ---- camera-first elimination: host side (kernels and the maths: esl_cf.hpp) ---------------------------------------------
// staging buffer of the distributed factorisation (one message per outer panel: esl_chol.hpp CholDist::pack)
static int chol_pack_ensure(esl_ctx* c, int n) {
  const size_t need = chol_pack_len(n);
  if (c->chol_pack && c->chol_pack2 && c->chol_pack_len >= need) return ESL_OK;
  int rc = al(&c->chol_pack, need);
  if (rc) return rc;
  if ((rc = al(&c->chol_pack2, need))) return rc;
  c->chol_pack_len = need;
  return ESL_OK;
}
// CholDist of this context: one packed message per outer panel, on its own stream unless switched off (ESL_CHOL_DIST_OVERLAP=0)
static int chol_dist_fill(esl_ctx* c, int n, CholDist& d) {
  d.rank = c->comm_rank; d.n_ranks = c->comm_ranks; d.user = c;
  d.bcast = [](void* u, double* dev, size_t count, int root) { return comm_bcast((esl_ctx*)u, dev, count, root); };
  const int rc = chol_pack_ensure(c, n);
  if (rc) return rc;
  d.pack = c->chol_pack;
  if (c->sw_chol_overlap) {
    d.pack2 = c->chol_pack2;
    d.bcast_on = [](void* u, double* dev, size_t count, int root, hipStream_t st) { return comm_bcast((esl_ctx*)u, dev, count, root, st); };
  }
  return ESL_OK;
}
static bool cf_applicable(const esl_ctx* c) { return c->cf_chain_ok && (!c->comm || c->comm_replicated); }
// replicated-graph communicator (esl_comm_set_replicated): the reduced ellipsoid system's outer panels are dealt to the ranks
static bool cf_dist(const esl_ctx* c) {
  if (!c->comm || !c->comm_replicated || c->comm_ranks < 2) return false;
  if (c->sw_chol_dist >= 0) return c->sw_chol_dist == 1;
  return 9L * c->g.n_objs >= 8192;
}
// esl_lm_params::linear_solver -> the form this trial runs with; < 0: the request cannot be served
// ESL_SOLVER_CAMERA_CHAIN: W is structurally empty (no edge of a free ellipsoid at a free camera) and the odometry edges chain
static bool chain_applicable(const esl_ctx* c) { return c->chain_ok && c->g.n_ue == 0 && !c->comm; }
static int slam_pick_solver(const esl_ctx* c) {
  const int want = c->lm.p.linear_solver;
  if (want == ESL_SOLVER_PCG) return c->comm ? -3 : ESL_SOLVER_PCG;
  if (want == ESL_SOLVER_CAMERA_CHAIN) return chain_applicable(c) ? ESL_SOLVER_CAMERA_CHAIN : -2;
  if (want == ESL_SOLVER_AUTO && c->fx_on && chain_applicable(c)) return ESL_SOLVER_CAMERA_CHAIN;   // (only graphs uploaded with a flag set)
  if (want == ESL_SOLVER_REDUCED_CAMERA) return ESL_SOLVER_REDUCED_CAMERA;
  if (want == ESL_SOLVER_REDUCED_ELLIPSOID) return cf_applicable(c) ? ESL_SOLVER_REDUCED_ELLIPSOID : -1;
  if (!cf_applicable(c) || c->cf_unavailable) return ESL_SOLVER_REDUCED_CAMERA;
  const double nc = (double)c->S_n, no = 9.0 * c->g.n_objs;
  return (no * no * nc + no * no * no / 3.0 < nc * nc * nc / 3.0) ? ESL_SOLVER_REDUCED_ELLIPSOID : ESL_SOLVER_REDUCED_CAMERA;
}
// everything cf_ensure hands out (interior pointers of the solver arena: forgotten, not freed), and the plan they were laid out by
static void cf_forget(esl_ctx* c) {
  c->cf_oe_start = c->cf_oe_u = c->cf_oe_slot = c->cf_oe_cst = nullptr;
  c->cf_seg_start = c->cf_seg_obj = c->cf_seg_first = c->cf_cmap = c->cf_xld = c->cf_fwork = c->cf_twork = nullptr;
  c->cf_mask = nullptr; c->cf_xoff = c->cf_boff = c->cf_roff = nullptr;
  c->cf_Linv = c->cf_M = c->cf_N = c->cf_V = c->cf_B = c->cf_Lfac = c->cf_G = c->cf_vy = c->cf_z = nullptr;
  c->cf_T = c->cf_Linv_ws = c->cf_part = nullptr;
  c->cf_Zt = c->cf_Hs = c->cf_Bs = c->cf_LfacS = c->cf_GS = c->cf_LiS = c->cf_MS = c->cf_NS = c->cf_R = nullptr;
  c->cf_Xc = c->cf_Xs = c->cf_P = c->cf_Prhs = c->cf_Xt = c->cf_Y = c->cf_Yr = nullptr;
  c->cf_os_start = nullptr; c->cf_os_cnt = c->cf_os_pairs = c->cf_os_run = c->cf_os_heads = nullptr; c->cf_Vm = nullptr;
  c->cf_Pm = c->cf_Qm = c->cf_XL = nullptr; c->cf_sl_ent = nullptr;
  c->cf_rank = c->cf_unrank = c->cf_kfirst = nullptr; c->cf_xo_t = nullptr;
  c->cf_plan = CfPlan{};
  c->cf_ready = false;
}
static int cf_ensure_impl(esl_ctx* c);
// The tables and buffers of the camera-first form exist and are initialised <=> cf_ready.  A failed allocation (dense X alone is
// 8.6 GB at BASELINE configs[3]) forgets the set again: the next trial step starts from scratch instead of launching on null
// pointers.
static int cf_ensure(esl_ctx* c) {
  if (c->cf_ready) return ESL_OK;
  const int rc = cf_ensure_impl(c);
  if (rc) { cf_forget(c); (void)hipGetLastError(); return rc; }
  c->cf_ready = true;
  return ESL_OK;
}
static_assert(kCfKC == kKC, "esl_cf_plan.hpp pads K to the rank-K update's chunk");
// Built by the FIRST trial step that picks the camera-first form -- not at upload (a graph whose trials run the reduced
// camera system, or that is sharded over ranks, never pays for them).  What is built and why is the plan's (esl_cf_plan.hpp,
// cf_plan_build: every ellipsoid's free-camera edges sorted by (slot, u); with X kept SPARSE over runs of cameras the segments'
// tables; T's order and staircase); here the plan is staged and shipped, the dense index tables (entry ranges, column map, tile
// lists, the one-sided assembly's pair list) are generated on the device, and what must be zero is zeroed.
static int cf_ensure_impl(esl_ctx* c) {
  const DevGraph& g = c->g;
  const int N = g.n_objs, nfi = g.n_free_cams;
  const size_t nf = (size_t)nfi, EU = (size_t)g.n_bbox + g.n_e3d, n_o = (size_t)9 * N;
  const bool timing = std::getenv("ESL_UPLOAD_HOST_TIMING") != nullptr;
  const double t0 = timing ? now_us() : 0;
  // the switches: three read at every layout (the tests set them between uploads), ESL_CF_ND_MIN once per process, two with the context
  CfSwitches sw;
  { const char* e = std::getenv("ESL_CF_SPARSE"); sw.sparse = e ? (int)(unsigned char)e[0] : -1; }
  { const char* e = std::getenv("ESL_CF_TPERM"); sw.tperm_off = e && e[0] == '0'; }
  sw.no_nd = std::getenv("ESL_CF_NO_ND") != nullptr;
  static const int nd_min = [] { const char* e = std::getenv("ESL_CF_ND_MIN"); return e ? std::atoi(e) : 48; }();
  sw.nd_min = nd_min; sw.stride = c->sw_cf_stride; sw.os_kernel = c->sw_cf_os_kernel; sw.os_list = c->sw_cf_os_list;
  sw.sweep = c->sw_cf_sweep;
  size_t free_b = 0, total_b = 0;   // (the TOTAL decides between forms 1 and 2, never what happens to be free)
  if (nfi >= kCfSparseMinCams) ESL_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  CfPlan& pl = c->cf_plan;
  if (!cf_plan_build(N, nfi, EU, c->h_ue_start, c->h_cu_start, c->h_cu_obj, c->h_cu_id, c->cf_chain_ok, c->comm != nullptr, total_b, sw, pl)) {
    set_error("camera-first elimination: the (ellipsoid, camera chunk) range table of this graph exceeds 1 GB");
    return ESL_ERR_ALLOC;
  }
  const bool sp = pl.sparse, os3 = sp && pl.form == 3, osm = os3 && pl.os_list;   // (osm: twins merged, shorter side)
  const bool swp = os3 && pl.sweep;   // Y in one sweep per segment: no interior slab (esl_cf_sweep.hpp)
  const int nch = pl.n_chunks, nseg = pl.nseg, nw = pl.nw, N1 = N + 1;
  const size_t n_inc = pl.p.size();
  const size_t y_recs = std::max<size_t>(n_inc, 1) * (size_t)(pl.S - 1), nb = (size_t)N * (N + 1) / 2 + N;   // (Y's records; blocks of T's lower triangle + the b row)
  const double t1 = timing ? now_us() : 0;
  // ---- layout: what the host ships first, then the device-generated tables (esl_cf.hpp k_cf_make_*), then the buffers ----
  BlobStage st;
  struct Up { int item; const void* src; size_t bytes; };
  std::vector<Up> ups;   // the plan's vectors, copied into the staging blob once it is reserved
  auto ship = [&](auto** dst, const auto& v) { ups.push_back({st.up(dst, v.size()), v.data(), v.size() * sizeof(v[0])}); };
  ship(&c->cf_oe_start, c->h_ue_start); ship(&c->cf_oe_u, pl.ou); ship(&c->cf_oe_slot, pl.os);
  int* d_inc = nullptr; int* d_fw_off = nullptr; long long* d_tw_off = nullptr;
  int i_inc = -1;
  if (pl.tperm) { ship(&c->cf_rank, pl.rank); ship(&c->cf_unrank, pl.unrank); ship(&c->cf_kfirst, pl.kfirst); }
  if (sp) {
    i_inc = st.up(&d_inc, 4 * n_inc); ship(&c->cf_seg_start, pl.seg_start); ship(&c->cf_xld, pl.xld);
    ship(&c->cf_xoff, pl.xoff); ship(&c->cf_boff, pl.boff); ship(&c->cf_roff, pl.roff); ship(&d_fw_off, pl.fw_off); ship(&d_tw_off, pl.tw_off);
  }
  if (osm) { ship(&c->cf_os_run, pl.os_run); ship(&c->cf_os_heads, pl.os_heads); }
  if (swp) ship(&c->cf_sl_ent, pl.sl_ent);
  st.work(&c->cf_oe_cst, (size_t)std::max(N, 1) * (nch + 1));
  if (sp) {
    st.work(&c->cf_cmap, (size_t)nseg * N1); st.work(&c->cf_mask, (size_t)N1 * nw); st.work(&c->cf_seg_obj, n_inc); st.work(&c->cf_seg_first, n_inc);
    st.work(&c->cf_fwork, 2 * (size_t)pl.n_fwork); st.work(&c->cf_twork, 3 * (size_t)pl.n_twork);
  }
  st.work(&c->cf_Linv, nf * 36); st.work(&c->cf_M, nf * 36); st.work(&c->cf_N, nf * 36); st.work(&c->cf_V, EU * 54);
  st.work(&c->cf_B, nf * 36); st.work(&c->cf_Lfac, nf * 21); st.work(&c->cf_G, nf * 36); st.work(&c->cf_vy, nf * 6); st.work(&c->cf_z, nf * 6);
  st.work(&c->cf_T, (size_t)pl.ldt * n_o); st.work(&c->cf_Linv_ws, ((n_o + kNB - 1) / kNB) * kNB * kNB);
  if (pl.tperm) st.work(&c->cf_xo_t, n_o);
  if (n_o <= 1024) st.work(&c->cf_part, (size_t)kCholMaxSplit * (size_t)pl.ldt * n_o);   // split-K workspace of small systems
  if (pl.nd) {
    const size_t ns = (size_t)std::max(pl.n_sep, 1);
    st.work(&c->cf_Zt, nf * 36); st.work(&c->cf_Hs, ns * 36); st.work(&c->cf_Bs, ns * 36); st.work(&c->cf_LfacS, ns * 21);
    st.work(&c->cf_GS, ns * 36); st.work(&c->cf_LiS, ns * 36); st.work(&c->cf_MS, ns * 36); st.work(&c->cf_NS, ns * 36);
    st.work(&c->cf_R, ns * 6 * (size_t)pl.ldx);
  }
  if (sp) {
    if (!swp) st.work(&c->cf_Xc, pl.xc_len);
    st.work(&c->cf_Xs, (size_t)pl.ldx * (size_t)pl.kpad_s);
    if (pl.form == 1) { st.work(&c->cf_P, pl.p_blocks * 81); st.work(&c->cf_Prhs, pl.prhs_len); }
    if (pl.form == 3) {
      st.work(&c->cf_Y, y_recs * 54); st.work(&c->cf_Yr, std::max<size_t>(nf, 1) * 6);
      st.work(&c->cf_os_start, nb + 1); st.work(&c->cf_os_cnt, nb); st.work(&c->cf_os_pairs, 2 * std::max<size_t>(pl.os_list_npairs, 1));
      if (osm) st.work(&c->cf_Vm, EU * 54);
      if (swp) { st.work(&c->cf_Pm, nf * 36); st.work(&c->cf_Qm, nf * 36); st.work(&c->cf_XL, std::max<size_t>(pl.xl_len, 1)); }
    }
  } else {
    st.work(&c->cf_Xt, (size_t)pl.ldx * (size_t)pl.kpad);
  }
  if (int rc = st.reserve(c->arena_solve)) return rc;
  // ---- fill the staging blob, ship it, generate the dense tables ----
  for (const Up& u : ups) if (u.bytes) std::memcpy(st.host<char>(u.item), u.src, u.bytes);
  if (sp && n_inc) {
    int* inc = st.host<int>(i_inc);   // the incidences: segment, ellipsoid, first camera, place in the column order (they are in it already)
    std::memcpy(inc, pl.p.data(), n_inc * sizeof(int)); std::memcpy(inc + n_inc, pl.o.data(), n_inc * sizeof(int));
    std::memcpy(inc + 2 * n_inc, pl.first.data(), n_inc * sizeof(int));
    for (size_t q = 0; q < n_inc; ++q) inc[3 * n_inc + q] = (int)q;
  }
  if (int rc = st.ship(c->stream)) return rc;
  if (N > 0) {
    const long nt = (long)N * (nch + 1);
    hipLaunchKernelGGL(k_cf_make_cst, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream, N, nch, c->cf_oe_start, c->cf_oe_slot, c->cf_oe_cst);
  }
  if (sp) {
    ESL_HIP_TRY(hipMemsetAsync(c->cf_cmap, 0xFF, (size_t)nseg * N1 * sizeof(int), c->stream));
    ESL_HIP_TRY(hipMemsetAsync(c->cf_mask, 0, (size_t)N1 * nw * sizeof(unsigned long long), c->stream));
    if (n_inc)
      hipLaunchKernelGGL(k_cf_make_cmap, dim3((unsigned)((n_inc + 255) / 256)), dim3(256), 0, c->stream, (int)n_inc, d_inc, N1, nw, c->cf_seg_start, c->cf_cmap,
                         c->cf_mask, c->cf_seg_obj, c->cf_seg_first);
    hipLaunchKernelGGL(k_cf_make_work, dim3((unsigned)nseg), dim3(64), 0, c->stream, nseg, N, nw, c->cf_seg_start, d_fw_off, d_tw_off, c->cf_cmap, c->cf_mask,
                       c->cf_fwork, c->cf_twork);
  }
  if (os3) {
    // the one-sided assembly's pair list (esl_cf.hpp): count per block, offsets on the host, fill.  Once per layout.
    const dim3 grid((unsigned)(N + 1), (unsigned)((N + kCfTPer - 1) / kCfTPer));
    ESL_HIP_TRY(hipMemsetAsync(c->cf_os_cnt, 0, nb * sizeof(int), c->stream));
    hipLaunchKernelGGL(k_cf_os_list<false>, grid, dim3(256), 0, c->stream, N, nw, nch, pl.S / kCfFwdCh, c->cf_mask, c->cf_cmap, c->cf_seg_start, c->cf_oe_cst, c->cf_oe_slot,
                       (const int*)c->cf_unrank, (const long long*)nullptr, c->cf_os_cnt, (int2*)nullptr, 0, (const int*)c->cf_os_run, (const int*)c->cf_os_heads);
    std::vector<int> h_cnt(nb);
    std::vector<long long> h_start(nb + 1);
    ESL_HIP_TRY(hipMemcpyAsync(h_cnt.data(), c->cf_os_cnt, nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    h_start[0] = 0;
    for (size_t b = 0; b < nb; ++b) h_start[b + 1] = h_start[b] + h_cnt[b];
    if ((size_t)h_start[nb] != pl.os_list_npairs) {
      set_error("camera-first elimination: the one-sided assembly's pair list does not have the length the host counted");
      return ESL_ERR_STATE;
    }
    ESL_HIP_TRY(hipMemcpyAsync(c->cf_os_start, h_start.data(), (nb + 1) * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_cf_os_list<true>, grid, dim3(256), 0, c->stream, N, nw, nch, pl.S / kCfFwdCh, c->cf_mask, c->cf_cmap, c->cf_seg_start, c->cf_oe_cst, c->cf_oe_slot,
                       (const int*)c->cf_unrank, (const long long*)c->cf_os_start, c->cf_os_cnt, (int2*)c->cf_os_pairs, pl.os_offsets ? 1 : 0,
                       (const int*)c->cf_os_run, (const int*)c->cf_os_heads);
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // (h_start is read by the copy until here)
  }
  // ---- what must be zero ----
  if (pl.nd) ESL_HIP_TRY(hipMemsetAsync(c->cf_Zt, 0, nf * 36 * sizeof(double), c->stream));
  if (sp) {
    // slabs: pad columns and rows 90 .. 95 stay zero; Xs: rows 6 n_sep .. kpad_s (the K padding of the rank-K update) stay zero;
    // T: the blocks above the diagonal are never written
    if (!swp) ESL_HIP_TRY(hipMemsetAsync(c->cf_Xc, 0, std::max<size_t>(pl.xc_len, 1) * sizeof(double), c->stream));
    ESL_HIP_TRY(hipMemsetAsync(c->cf_Xs, 0, (size_t)pl.ldx * (size_t)pl.kpad_s * sizeof(double), c->stream));
    ESL_HIP_TRY(hipMemsetAsync(c->cf_T, 0, (size_t)pl.ldt * n_o * sizeof(double), c->stream));
    if (pl.form == 3) {   // (the records of slots behind a short last segment's end are never written and never read)
      ESL_HIP_TRY(hipMemsetAsync(c->cf_Y, 0, y_recs * 54 * sizeof(double), c->stream));
      ESL_HIP_TRY(hipMemsetAsync(c->cf_Yr, 0, std::max<size_t>(nf, 1) * 6 * sizeof(double), c->stream));
    }
  } else {
    // rows 6 nf .. kpad of X (the K padding of the rank-K update) and the columns of never-written edges stay zero
    ESL_HIP_TRY(hipMemsetAsync(c->cf_Xt, 0, (size_t)pl.ldx * (size_t)pl.kpad * sizeof(double), c->stream));
  }
  ESL_HIP_TRY(hipMemsetAsync(c->cf_V, 0, std::max<size_t>(EU, 1) * 54 * sizeof(double), c->stream));
  if (timing)
    fprintf(stderr, "[cf_ensure host, us] sorts + structure %.0f  layout + tables + enqueue %.0f  (blob %.1f MB uploaded, %.1f MB in all; sparse %d form %d)\n",
            t1 - t0, now_us() - t1, st.up_end / 1e6, st.total / 1e6, (int)sp, pl.form);
  return ESL_OK;
}

// ---- one LM trial with the cameras eliminated first: x_c, x_o, trial states, chi2 of the trial (same outputs as the other form) ----
namespace {
// side-stream work not yet waited for by the main stream when the trial is left (an ESL_HIP_TRY failure): joined here, so that EVERY
// way out of a trial leaves the side stream joined to the main one
struct CfSideJoin {
  CholRuntime& rt; hipStream_t main; bool armed;
  hipError_t wait(hipEvent_t ev) { const hipError_t e = hipStreamWaitEvent(main, ev, 0); armed = e != hipSuccess; return e; }
  ~CfSideJoin() {
    if (!armed) return;
    if (hipEventRecord(rt.cf_ev_p, rt.cf_side) != hipSuccess || hipStreamWaitEvent(main, rt.cf_ev_p, 0) != hipSuccess) (void)hipStreamSynchronize(rt.cf_side);
  }
};
// What the schedules of one trial share: the context, the plan, the dimensions and the launches that more than one of them enqueues.
// A schedule (build_*) is the reduced-system build of one form -- factor of the camera block, X = L^-1 [W | b_c], T = D - X^T X --
// written top to bottom in the order it enqueues; back_substitute is the same for all of them.
struct CfTrial {
  esl_ctx* c; CholRuntime& rt; const CfPlan& pl; const DevGraph& g; const double lambda;
  const int N, nf, n_o; const long ldx, ldt;
  const int st, ns, nseg;   // dissection: stride, separators, segments
  const bool nd, dist;      // dist: replicated-graph communicator, this rank builds its outer panels of T only
  const unsigned cg;        // groups of 64 columns of [X | y]
  const bool swp;           // form 3 without the interior slab (esl_cf_sweep.hpp)
  const hipStream_t main;
  CfSideJoin join;
  CfTrial(esl_ctx* c_, CholRuntime& rt_, double lambda_)
      : c(c_), rt(rt_), pl(c_->cf_plan), g(c_->g), lambda(lambda_), N(g.n_objs), nf(g.n_free_cams), n_o(9 * N), ldx((long)pl.ldx), ldt((long)pl.ldt),
        st(pl.stride), ns(pl.n_sep), nseg(pl.n_seg), nd(st > 0 && ns > 0), dist(cf_dist(c_)), cg((unsigned)((n_o + 1 + 63) / 64)), swp(pl.sparse && pl.form == 3 && pl.sweep), main(c_->stream),
        join{rt_, c_->stream, false} {}
  CfSegs segs() const { return CfSegs{c->cf_fwork, c->cf_seg_start, c->cf_seg_obj, c->cf_xoff, c->cf_xld, c->cf_rank, c->cf_unrank}; }
  int edge_blocks() const { return (int)(((long)pl.n_list * 9 + nf + 255) / 256); }
  // this rank's columns of T: everything, or with the replicated-graph communicator its outer panels (dealt cyclically, as the
  // distributed factorisation expects them)
  template <class F> void my_columns(F f) const {
    if (!dist) { f(0L, (long)n_o); return; }
    const int Wp = chol_outer_panels(n_o), n_outer = ((n_o + kNB - 1) / kNB + Wp - 1) / Wp;
    for (int op = c->comm_rank; op < n_outer; op += c->comm_ranks) f((long)op * Wp * kNB, std::min<long>((long)(op + 1) * Wp * kNB, (long)n_o));
  }
  // grid of a T-block kernel over the ellipsoids [o2b, o2e) of these columns (a block that straddles a panel boundary: on both sides)
  dim3 block_grid(long c_begin, long c_end, int& o2b, int& o2e) const {
    o2b = (int)(c_begin / 9); o2e = (int)((c_end + 8) / 9);
    return dim3((unsigned)(N + 1), (unsigned)((o2e - o2b + kCfTPer - 1) / kCfTPer));
  }
  // X sparse: V = Li W, vy = Li b_c of the list entries of class cls (esl_cf.hpp -- 0 all, 1 / 2 those of interior / separator slots)
  void edge_scale(int cls, hipStream_t s) const {
    hipLaunchKernelGGL(k_cf_edge_scale, dim3((unsigned)edge_blocks()), dim3(256), 0, s, g, pl.n_list, c->cf_oe_u, c->cf_oe_slot, c->Wbb, c->cf_Linv, c->bc,
                       c->cf_V, c->cf_vy, cls, st);
  }
  // nested dissection (esl_cf.hpp), first half: the segments' chains in parallel and the separators' system assembled from them
  // after_chain: enqueued straight behind the chains' launch (the sweep's per-slot matrices need L_ii and G alone)
  template <class F> void segment_chains(F after_chain) const {
    hipLaunchKernelGGL(k_cf_chain, dim3((unsigned)nseg), dim3(64), 0, main, nf, c->Hcc, c->cf_B, lambda, c->cf_Lfac, c->cf_G, c->chol_info, st, st - 1);
    after_chain();
    hipLaunchKernelGGL(k_cf_factor_blocks, dim3((unsigned)((nf + 63) / 64)), dim3(64), 0, main, nf, c->cf_Lfac, c->cf_G, c->cf_Linv, c->cf_M, c->cf_N, st);
    if (nseg > 1) hipLaunchKernelGGL(k_cf_zt, dim3((unsigned)(nseg - 1)), dim3(64), 0, main, nf, st, c->cf_Linv, c->cf_M, c->cf_B, c->cf_Zt);
    hipLaunchKernelGGL(k_cf_sep_assemble, dim3((unsigned)((ns * 36 + 255) / 256)), dim3(256), 0, main, nf, st, ns, c->Hcc, lambda, c->cf_G, c->cf_Zt,
                       c->cf_Hs, c->cf_Bs);
  }
  // second half: the separators' own short chain (one wave, n_sep steps) and its blocks
  void sep_chain(hipStream_t s) const {
    hipLaunchKernelGGL(k_cf_chain, dim3(1), dim3(64), 0, s, ns, c->cf_Hs, c->cf_Bs, 0.0, c->cf_LfacS, c->cf_GS, c->chol_info, ns, ns);
    hipLaunchKernelGGL(k_cf_factor_blocks, dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, s, ns, c->cf_LfacS, c->cf_GS, c->cf_LiS, c->cf_MS, c->cf_NS, 0,
                       c->cf_Linv, st);   // (+ the separators' L_ii^-1 into the per-slot array: was k_cf_sep_scatter)
  }
  // X sparse, the head of every schedule: the segments' chains, the separators' chain, V and vy, the interior rows into the segments'
  // compact slabs (sums for the separators into R).  beside: the separators' chain on the side stream -- enqueued FIRST: a small grid is
  // resident at once and a full grid on the other stream fills the rest of the GPU (two full grids do not share it: esl_chol.hpp,
  // cf_overlap_init) -- beside V and vy of the INTERIOR slots, which need L_ii^-1 of the segments' chains alone; the separator slots'
  // are then left to the caller, behind cf_ev_s (the separators' blocks exist)
  int slabs(bool beside) {
    // no slab (esl_cf_sweep.hpp): P and Q of the backward direction, one wave per segment and stride - 1 serial steps -- on the side
    // stream beside the rest of the chains' launches and V (cf_ev_c -> cf_ev_t), else in stream order
    auto twist = [&](hipStream_t s) {
      hipLaunchKernelGGL(k_cf_twist, dim3((unsigned)nseg), dim3(64), 0, s, nf, st, c->Hcc, lambda, c->cf_Lfac, c->cf_G, c->cf_Pm, c->cf_Qm, c->chol_info);
    };
    hipError_t e_tw = hipSuccess;
    segment_chains([&] {
      if (!swp) return;
      if (!beside) { twist(main); return; }
      e_tw = hipEventRecord(rt.cf_ev_c, main);
      if (e_tw == hipSuccess) e_tw = hipStreamWaitEvent(rt.cf_side, rt.cf_ev_c, 0);
      if (e_tw != hipSuccess) return;
      join.armed = true;
      twist(rt.cf_side);
      e_tw = hipEventRecord(rt.cf_ev_t, rt.cf_side);
    });
    ESL_HIP_TRY(e_tw);
    if (beside) {
      ESL_HIP_TRY(hipEventRecord(rt.cf_ev_a, main));
      ESL_HIP_TRY(hipStreamWaitEvent(rt.cf_side, rt.cf_ev_a, 0));
      join.armed = true;
    }
    sep_chain(beside ? rt.cf_side : main);
    if (beside) ESL_HIP_TRY(hipEventRecord(rt.cf_ev_s, rt.cf_side));
    if (swp) {   // Y, the sums in R and the last slot's rows in one sweep
      edge_scale(beside ? 1 : 0, main);
      if (beside) ESL_HIP_TRY(hipStreamWaitEvent(main, rt.cf_ev_t, 0));
      auto sweep = [&](auto parts) {
        hipLaunchKernelGGL((k_cf_sweep<decltype(parts)::value>), dim3((unsigned)pl.n_fwork), dim3(64), 0, main, nf, n_o, pl.n_chunks, c->cf_oe_cst, c->cf_oe_slot,
                           c->cf_V, c->cf_vy, c->cf_M, (const double*)c->cf_Zt, c->cf_Pm, c->cf_Qm, c->cf_R, ldx, st, segs(), c->cf_Y, c->cf_Yr, c->cf_XL,
                           (long long)(st == kCfFwdCh ? kCfSegRows : 6 * (st - 1)));
      };
      if (c->sw_cf_fwd_parts == 8) sweep(std::integral_constant<int, 8>{});
      else if (c->sw_cf_fwd_parts == 4) sweep(std::integral_constant<int, 4>{});
      else sweep(std::integral_constant<int, 2>{});
      return ESL_OK;
    }
    edge_scale(beside ? 1 : 0, main);
    auto forward = [&](auto parts) {   // (the parts of a chunk, ESL_CF_FWD_PARTS: LDS per workgroup, so the waves in flight; same bits)
      hipLaunchKernelGGL((k_cf_forward<2, decltype(parts)::value>), dim3((unsigned)pl.n_fwork), dim3(64), 0, main, nf, n_o, pl.n_chunks, c->cf_oe_cst, c->cf_oe_slot,
                         c->cf_V, c->cf_vy, c->cf_M, c->cf_Xc, ldx, st, st - 1, (const double*)c->cf_Zt, c->cf_R, st, segs());
    };
    if (c->sw_cf_fwd_parts == 8) forward(std::integral_constant<int, 8>{});
    else if (c->sw_cf_fwd_parts == 4) forward(std::integral_constant<int, 4>{});
    else forward(std::integral_constant<int, 2>{});
    return ESL_OK;
  }
  // the separators' right-hand sides from the slabs (sp; else from the dense X), the sums and their own V ...
  void sep_rhs(hipStream_t s, bool sp = true) const {
    hipLaunchKernelGGL(k_cf_sep_rhs, dim3(cg, (unsigned)ns), dim3(64), 0, s, nf, n_o, st, pl.n_chunks, c->cf_oe_cst, c->cf_oe_slot, c->cf_V, c->cf_vy,
                       c->cf_G, c->cf_LiS, sp ? c->cf_Xc : c->cf_Xt, ldx, c->cf_R, sp ? (const int*)c->cf_cmap : nullptr, sp ? segs() : CfSegs{},
                       (const double*)(sp && swp ? c->cf_XL : nullptr), (long long)(st == kCfFwdCh ? kCfSegRows : 6 * (st - 1)));
  }
  // ... and the separators' dense rows: into Xs (row block k = separator k), else into X at their slots; one wave per 64 columns
  void sep_forward(hipStream_t s, bool sp = true) const {
    hipLaunchKernelGGL(k_cf_forward<1>, dim3(cg), dim3(64), 0, s, ns, n_o, pl.n_chunks, c->cf_oe_cst, c->cf_oe_slot, c->cf_V, c->cf_vy,
                       c->cf_MS, sp ? c->cf_Xs : c->cf_Xt, ldx, ns, ns, (const double*)nullptr, c->cf_R, sp ? 0 : st, CfSegs{});
  }
  void products(hipStream_t s) const {   // form 1: the segments' products P_p = Xc_p^T Xc_p and their right-hand sides' rows
    hipLaunchKernelGGL(k_cf_seg_syrk, dim3((unsigned)pl.n_twork), dim3(256), 0, s, c->cf_twork, c->cf_seg_start, c->cf_seg_first, c->cf_xoff,
                       c->cf_xld, c->cf_Xc, c->cf_boff, c->cf_P);
    hipLaunchKernelGGL(k_cf_seg_rhs, dim3((unsigned)pl.n_fwork), dim3(64), 0, s, c->cf_fwork, c->cf_seg_start, c->cf_xoff, c->cf_xld, c->cf_Xc,
                       c->cf_roff, c->cf_Prhs);
  }
  void gather_products(long c_begin, long c_end, int accumulate) const {   // form 1: T = D - sum of the stored products, block by block
    int o2b, o2e;
    const dim3 grid = block_grid(c_begin, c_end, o2b, o2e);
    hipLaunchKernelGGL(k_cf_T_gather, grid, dim3(256), 0, main, N, pl.nw, c->cf_mask, c->cf_cmap, c->cf_boff, c->cf_roff, c->cf_P, c->cf_Prhs,
                       c->Hoo, c->bo, lambda, c->cf_T, ldt, o2b, o2e, (const int*)c->cf_unrank, accumulate);
  }
  // T -= X^T X over the rows of X that are dense: all of them, or (X sparse) the separators' under the staircase
  void update() const {
    ProfScope pk(c, 7);   // the rank-K update alone (nested in class 2): the MFMA roofline kernel of this form
    const double* Xf = pl.sparse ? c->cf_Xs : c->cf_Xt;
    const int K = (int)(pl.sparse ? pl.kpad_s : pl.kpad);
    if (!dist && K <= 0) return;
    my_columns([&](long c_begin, long c_end) {
      chol_launch_update(rt.sw, c->cf_T, ldt, (long)n_o + 1, main, 0, K, c_begin, c_end, Xf, ldx, dist ? nullptr : c->cf_part, pl.sparse ? c->cf_kfirst : nullptr);
    });
  }

  // ---- dense X (plain chain or nested dissection), in stream order ----
  int build_dense() {
    // V = Li W, vy = Li b_c of every list entry; the same launch writes the whole of T (D's lower blocks, b_o's row, zeros) -- nothing
    // reads T before the rank-K update
    auto edge_scale_T = [&] {
      const int nb_es = edge_blocks();
      hipLaunchKernelGGL(k_cf_edge_scale_T, dim3((unsigned)(nb_es + (int)((ldt * (long)n_o + 255) / 256))), dim3(256), 0, main, g, nb_es, pl.n_list, c->cf_oe_u,
                         c->cf_oe_slot, c->Wbb, c->cf_Linv, c->bc, c->cf_V, c->cf_vy, c->Hoo, c->bo, lambda, c->cf_T, ldt, (long)n_o);
    };
    if (!nd) {
      hipLaunchKernelGGL(k_cf_chain, dim3(1), dim3(64), 0, main, nf, c->Hcc, c->cf_B, lambda, c->cf_Lfac, c->cf_G, c->chol_info, nf, nf);
      hipLaunchKernelGGL(k_cf_factor_blocks, dim3((unsigned)((nf + 63) / 64)), dim3(64), 0, main, nf, c->cf_Lfac, c->cf_G, c->cf_Linv, c->cf_M, c->cf_N, 0);
      edge_scale_T();
      hipLaunchKernelGGL(k_cf_forward<0>, dim3(cg), dim3(64), 0, main, nf, n_o, pl.n_chunks, c->cf_oe_cst, c->cf_oe_slot, c->cf_V, c->cf_vy,
                         c->cf_M, c->cf_Xt, ldx, nf, nf, (const double*)nullptr, (double*)nullptr, 0, CfSegs{});
    } else {   // segments in parallel, then the separators' own short chain
      segment_chains([] {});
      sep_chain(main);
      edge_scale_T();
      hipLaunchKernelGGL(k_cf_forward<0>, dim3(cg, (unsigned)nseg), dim3(64), 0, main, nf, n_o, pl.n_chunks, c->cf_oe_cst, c->cf_oe_slot, c->cf_V,
                         c->cf_vy, c->cf_M, c->cf_Xt, ldx, st, st - 1, (const double*)c->cf_Zt, c->cf_R, st, CfSegs{});
      sep_rhs(main, false);
      sep_forward(main, false);
    }
    ESL_HIP_TRY(hipGetLastError());
    update();
    return ESL_OK;
  }

  // ---- X sparse, forms 1 (stored products) and 2 (blocks straight from the slabs), every launch in stream order: ESL_CF_OVERLAP=0, and
  // the only schedule of a run with a communicator (the products on every rank, 3 % of a trial; gather and update over this rank's panels) ----
  int build_stored_serial() {
    if (int rc = slabs(false)) return rc;
    sep_rhs(main);
    sep_forward(main);
    {   // T = D - (interior rows)^T (interior rows), block by block (every block on and below the diagonal is written)
      ProfScope pk(c, 8);
      if (pl.form == 1) products(main);
      my_columns([&](long c_begin, long c_end) {
        if (pl.form == 1) { gather_products(c_begin, c_end, 0); return; }
        int o2b, o2e;
        const dim3 grid = block_grid(c_begin, c_end, o2b, o2e);
        hipLaunchKernelGGL(k_cf_T_sparse, grid, dim3(256), 0, main, N, pl.nw, c->cf_mask, c->cf_cmap, c->cf_xoff, c->cf_xld, c->cf_Xc, c->Hoo, c->bo,
                           lambda, c->cf_T, ldt, o2b, o2e, (const int*)c->cf_unrank);
      });
    }
    ESL_HIP_TRY(hipGetLastError());
    update();
    return ESL_OK;
  }

  // ---- X sparse, form 1 on a single rank with the side stream (ESL_CF_OVERLAP=ov, 1 to 4).  Two dependent chains meet only at k_cf_sep_rhs:
  //   interior    k_cf_edge_scale (interior slots) -> k_cf_forward<2> -> the segments' products (k_cf_seg_syrk, k_cf_seg_rhs)
  //   separators  k_cf_chain (one wave, n_sep steps) -> k_cf_factor_blocks -> V, vy of the separator slots -> [k_cf_forward<2>'s slabs
  //               and sums] -> k_cf_sep_rhs -> k_cf_forward<1> (one wave per 64 columns) -> the rank-K update
  // so (1) the separators' chain and its blocks run on the side stream beside the interior pipeline (ov != 3) and (2) the products,
  // which need the slabs alone, run there beside k_cf_forward<1> (ov != 2; each alone: A/B) and the update.
  // No arithmetic and no address changes, so every array has the bits of the serial order.
  // Across trials: the side chain of trial t + 1 writes cf_LfacS, cf_GS, cf_LiS, cf_MS, cf_NS and the separators' slots of cf_Linv,
  // which trial t's k_cf_edge_scale (separator slots), k_cf_sep_rhs, k_cf_forward<1>, k_cf_tridiag_back and k_cf_back_prep read: all of
  // them are on the main stream in front of trial t + 1's cf_ev_a, which the side chain waits for.  Trial t + 1's k_cf_forward<2>
  // writes the slabs trial t's products read: the main stream has waited for trial t's cf_ev_p.  cf_ensure's relayout, esl_ctx_trim
  // and everything else on the main stream are covered the same way, because every way out of a trial leaves the side stream joined
  // to the main one (CfSideJoin). ----
  int build_stored_side(int ov) {
    const bool side_chain = ov != 3, early_products = ov != 2;
    if (int rc = slabs(side_chain)) return rc;
    if (side_chain) {   // the separators' chain is needed from here on: their V and vy, then the right-hand sides
      ESL_HIP_TRY(join.wait(rt.cf_ev_s));
      edge_scale(2, main);
    }
    sep_rhs(main);
    // cf_ev_x, the products may start: the slabs were complete after k_cf_forward<2> and k_cf_sep_rhs only reads them, so in front
    // of k_cf_forward<1>'s 282 waves (C4), beside them -- or (ov == 2) behind them.  Measured at C4: the products start 1.4 ms
    // earlier, k_cf_forward<1> stretches from 0.61 to 1.08 ms beside them, the update starts 0.32 ms earlier
    if (early_products) ESL_HIP_TRY(hipEventRecord(rt.cf_ev_x, main));
    sep_forward(main);
    if (!early_products) ESL_HIP_TRY(hipEventRecord(rt.cf_ev_x, main));
    ESL_HIP_TRY(hipStreamWaitEvent(rt.cf_side, rt.cf_ev_x, 0));
    join.armed = true;
    products(rt.cf_side);
    ESL_HIP_TRY(hipEventRecord(rt.cf_ev_p, rt.cf_side));   // cf_ev_p: the products are stored
    if (chol_update_v_applies(rt.sw, ldt, (long)n_o + 1, 0, (long)n_o, true, ldx)) {
      // with the update on its k_chol_update_v path (the one with an assign form) the products also run beside the UPDATE (round 6): it
      // ASSIGNS T = -Xs^T Xs instead of updating what the gather wrote, and the gather, which then comes last, adds its D - sum to that --
      // (D - sum) + (-acc) is the same double as (D - sum) - acc, so T has the same bits
      {
        // ov == 4 (default): the update CAPPED to one workgroup per CU (chol_launch_update's `cap`).  At its two workgroups
        // per CU (252 registers a lane) every slot that frees goes to the next update workgroup and the products' waves (240) are
        // placed only when the update has nothing left to dispatch; capped, one products workgroup is resident on every CU beside it.
        // C4: the update stretches from 16.4 to 20.0 ms and the products end with it instead of 4.5 ms later
        ProfScope pk(c, 7);   // the rank-K update (assign form), with the products running beside it
        chol_launch_update(rt.sw, c->cf_T, ldt, (long)n_o + 1, main, 0, (int)pl.kpad_s, 0, (long)n_o, c->cf_Xs, ldx, nullptr, c->cf_kfirst, true, ov == 4);
      }
      ESL_HIP_TRY(join.wait(rt.cf_ev_p));
      ProfScope pk(c, 8);   // (what is left of the products' path on this stream: the gather)
      gather_products(0, (long)n_o, 1);
    } else {   // (the update has no assign form at this size: the products ran beside k_cf_forward<1> alone)
      ESL_HIP_TRY(join.wait(rt.cf_ev_p));
      {
        ProfScope pk(c, 8);
        gather_products(0, (long)n_o, 0);
      }
      ESL_HIP_TRY(hipGetLastError());
      update();
    }
    return ESL_OK;
  }

  // ---- X sparse, form 3 (one-sided assembly, esl_cf.hpp; single rank).  The assembly needs Y alone, which exists straight behind
  // k_cf_forward<2>, so with the side stream (`beside`: ESL_CF_OVERLAP != 0) the WHOLE separator path -- chain, V and vy of the
  // separator slots, k_cf_sep_rhs, k_cf_forward<1> -- runs there beside k_cf_seg_back and the assembly, and the update (uncapped, in
  // its accumulate form, with nothing beside it) waits for the assembly and Xs only.  One arithmetic order for T at either setting:
  // T = D - sum (assign), then T -= Xs^T Xs.  Hazards across trials: as in build_stored_side, with cf_ev_p = Xs is complete.
  // k_cf_v_merge reads cf_V on the main stream while edge_scale(2) may still write cf_V on the side stream: disjoint records -- a run
  // is an ellipsoid's entries of one INTERIOR slot (os_run is 0 elsewhere), class 2 writes the entries of separator slots only; the
  // interior ones were written by edge_scale(1) in front of it on the main stream.  cf_Vm is written and read on the main stream.
  // Without the interior slab (swp, esl_cf_sweep.hpp; ESL_CF_SWEEP != 0) slabs() leaves Y, the sums in R and the last interior slots'
  // rows (cf_XL, which k_cf_sep_rhs reads on the side stream: covered like the slabs were, by cf_ev_x and cf_ev_p) and no k_cf_seg_back
  // follows; k_cf_twist's cf_Pm / cf_Qm are written on the side stream behind cf_ev_c and read on the main one behind cf_ev_t. ----
  int build_onesided(bool beside) {
    const hipStream_t sst = beside ? rt.cf_side : main;   // the separators' stream
    if (int rc = slabs(beside)) return rc;
    if (beside) {   // the side stream, which holds the separators' chain, waits for the slabs and the sums in R (cf_ev_x)
      ESL_HIP_TRY(hipEventRecord(rt.cf_ev_x, main));
      ESL_HIP_TRY(hipStreamWaitEvent(rt.cf_side, rt.cf_ev_x, 0));
      edge_scale(2, rt.cf_side);
    }
    sep_rhs(sst);
    sep_forward(sst);
    if (beside) ESL_HIP_TRY(hipEventRecord(rt.cf_ev_p, rt.cf_side));
    {   // Y behind the slabs, T = D - sum from V and Y
      ProfScope pk(c, 8);
      auto seg_back = [&](auto mch) {   // (the segment's chunks: the kernel's register arrays want a compile-time length)
        hipLaunchKernelGGL(k_cf_seg_back<decltype(mch)::value>, dim3((unsigned)pl.n_fwork), dim3(64), 0, main, nf, c->cf_fwork, c->cf_seg_start, c->cf_xoff,
                           c->cf_xld, c->cf_Xc, c->cf_Linv, c->cf_G, c->cf_Y, c->cf_Yr);
      };
      if (!swp) {   // (else Y is the sweep's, written by slabs())
        if (st == 3 * kCfFwdCh) seg_back(std::integral_constant<int, 3>{});
        else if (st == 2 * kCfFwdCh) seg_back(std::integral_constant<int, 2>{});
        else seg_back(std::integral_constant<int, 1>{});
      }
      // twins merged (esl_cf.hpp k_cf_os_list): the runs' sums of V, which the list's pairs name; ESL_CF_OS_LIST=0: V itself
      if (pl.os_list && pl.n_list > 0)
        hipLaunchKernelGGL(k_cf_v_merge, dim3((unsigned)(((long)pl.n_list * 9 + 255) / 256)), dim3(256), 0, main, pl.n_list, (const int*)c->cf_os_run, c->cf_V, c->cf_Vm);
      const dim3 grid((unsigned)(N + 1), (unsigned)((N + kCfTPer - 1) / kCfTPer));
      // whole records through LDS, or the per-lane gather: same bits
      hipLaunchKernelGGL(pl.os_offsets ? k_cf_T_onesided_lds : k_cf_T_onesided, grid, dim3(256), 0, main, N, (const int2*)c->cf_os_pairs,
                         (const long long*)c->cf_os_start, (const int*)c->cf_os_cnt, pl.os_list ? c->cf_Vm : c->cf_V, c->cf_Y, c->cf_Yr, c->Hoo, c->bo, lambda, c->cf_T, ldt, 0, N,
                         (const int*)c->cf_unrank, 0);
    }
    ESL_HIP_TRY(hipGetLastError());
    if (beside) ESL_HIP_TRY(join.wait(rt.cf_ev_p));
    update();
    return ESL_OK;
  }

  // ---- every form: dense Cholesky of the reduced ellipsoid system, the camera back-substitution, trial states and their chi2 ----
  int back_substitute() const {
    {
      ProfScope ps(c, 3);
      double* xsol = (pl.sparse && pl.tperm) ? c->cf_xo_t : c->xo;   // the solver's x_o: in T's column order
      if (dist) {
        CholDist d;
        if (int rc = chol_dist_fill(c, n_o, d)) return rc;
        ESL_HIP_TRY(chol_factor_solve(c->cf_T, ldt, n_o, c->cf_Linv_ws, c->z_ws, xsol, c->chol_info, main, rt, &d));
      } else {
        ESL_HIP_TRY(chol_factor_solve(c->cf_T, ldt, n_o, c->cf_Linv_ws, c->z_ws, xsol, c->chol_info, main, rt));
      }
      if (xsol != c->xo) hipLaunchKernelGGL(k_cf_xo_unpermute, dim3((unsigned)((n_o + 255) / 256)), dim3(256), 0, main, N, c->cf_rank, xsol, c->xo);
      if (swp) {   // interior rows: d = vy - W_I x_o slot by slot, then the segments' forward recurrence on it; the separators' dense rows as ever
        hipLaunchKernelGGL(k_cf_wxo, dim3((unsigned)nf), dim3(64), 0, main, st, g.cu_start, (const int*)c->cf_sl_ent, g.cu_obj, c->cf_V, c->cf_vy, c->xo, c->cf_z);
        hipLaunchKernelGGL(k_cf_z_fwd, dim3((unsigned)nseg), dim3(64), 0, main, nf, st, c->cf_M, c->cf_z);
        if (ns > 0)
          hipLaunchKernelGGL(k_cf_z_sparse, dim3((unsigned)(6 * ns)), dim3(256), 0, main, n_o, c->cf_Xs, ldx, segs(), (const double*)nullptr, c->xo, xsol, c->cf_z, st, 1);
      } else if (pl.sparse)
        hipLaunchKernelGGL(k_cf_z_sparse, dim3((unsigned)(6 * nf)), dim3(256), 0, main, n_o, c->cf_Xs, ldx, segs(), c->cf_Xc, c->xo, xsol, c->cf_z, st);
      else
        hipLaunchKernelGGL(k_cf_z, dim3((unsigned)(6 * nf)), dim3(256), 0, main, c->cf_Xt, ldx, n_o, c->xo, c->cf_z);
      if (nd) {
        hipLaunchKernelGGL(k_cf_tridiag_back, dim3(1), dim3(64), 0, main, ns, c->cf_LiS, c->cf_NS, c->cf_z, c->xc, ns, ns, st);            // separators
        hipLaunchKernelGGL(k_cf_back_prep, dim3((unsigned)((6 * nf + 255) / 256)), dim3(256), 0, main, nf, st, ns, c->cf_Zt, c->cf_G, c->xc, c->cf_z);
        hipLaunchKernelGGL(k_cf_tridiag_back, dim3((unsigned)nseg), dim3(64), 0, main, nf, c->cf_Linv, c->cf_N, c->cf_z, c->xc, st, st - 1, 0);  // segments
      } else {
        hipLaunchKernelGGL(k_cf_tridiag_back, dim3(1), dim3(64), 0, main, nf, c->cf_Linv, c->cf_N, c->cf_z, c->xc, nf, nf, 0);
      }
      ESL_HIP_TRY(hipGetLastError());
    }
    ProfScope ps(c, 1);
    const int F = g.n_cams, nb_obj = (N + 255) / 256, nb_cam = (F + 255) / 256;
    hipLaunchKernelGGL(k_cf_updates, dim3((unsigned)(nb_obj + nb_cam)), dim3(256), 0, main, g, nb_obj, lambda, c->objs, c->bo, c->xo, c->objs_trial, c->obj_part,
                       c->cams, c->xc, c->bc, c->cams_trial, c->cam_part);
    const int nb_co = (N + kWavesPerBlock - 1) / kWavesPerBlock, nb_od = (g.n_odom + kWave * kWavesPerBlock - 1) / (kWave * kWavesPerBlock);
    robust_dispatch(c->robust_on, [&](auto robust) {
      hipLaunchKernelGGL(k_slam_chi2_all<decltype(robust)::value>, dim3((unsigned)(nb_co + nb_od)), dim3(kWave * kWavesPerBlock), 0, main, g, nb_co,
                         c->cams_trial, c->objs_trial, c->obj_part, c->od_part);
    });
    ESL_HIP_TRY(hipGetLastError());
    return ESL_OK;
  }
};
}  // namespace
static int slam_try_step_cf(esl_ctx* c, double lambda) {
  int rc = cf_ensure(c);
  if (rc) return rc;
  const CfPlan& pl = c->cf_plan;
  CfTrial t(c, chol_rt(c), lambda);
  {
    ProfScope ps(c, 2);   // "reduced-system build"
    ESL_HIP_TRY(hipMemsetAsync(c->chol_info, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_cf_gather_B, dim3((unsigned)(((long)t.nf * 36 + 255) / 256)), dim3(256), 0, c->stream, t.nf, c->Aod, c->cf_od_start, c->cf_od_edge, c->cf_B);
    ESL_HIP_TRY(chol_set_attributes(t.rt));   // (fills rt.sw)
    if (!pl.sparse) rc = t.build_dense();
    else if (!t.nd) {   // (ESL_CF_ND_MIN above this graph's free cameras with X forced sparse: there is no such schedule, and never was)
      set_error("camera-first elimination: sparse X needs the dissected camera chain");
      rc = ESL_ERR_STATE;
    }
    else {
      // the side stream: a single rank's forms 1 and 3, unless ESL_CF_OVERLAP was 0 when the context was created or the stream cannot be made
      const bool side = c->sw_cf_overlap != 0 && (pl.form == 1 || pl.form == 3) && !t.dist && pl.kpad_s > 0 && t.rt.cf_overlap_init() == hipSuccess;
      rc = pl.form == 3 ? t.build_onesided(side) : side ? t.build_stored_side(c->sw_cf_overlap) : t.build_stored_serial();
    }
    if (rc) return rc;
    ESL_HIP_TRY(hipGetLastError());
  }
  return t.back_substitute();
}

// Sharded runs: factor the reduced camera system distributed over the ranks (esl_chol.hpp, CholDist) instead of all-reducing
// it and factoring it on every rank.  Default from 8,192 unknowns (below that the chain of diagonal blocks is the whole cost and
// a broadcast per panel only adds to it); ESL_CHOL_DIST=1 / 0 forces it on / off.
static bool slam_dist_chol(esl_ctx* c) {
  if (!c->comm || c->comm_ranks < 2) return false;
  if (c->sw_chol_dist >= 0) return c->sw_chol_dist == 1;   // ESL_CHOL_DIST as read when the communicator was created
  return c->S_n >= 8192;
}
// event bracket around the dense FACTORISATION alone (class 9, nested in class 3): k_chol_persist, or the launch-per-step chain
static void chol_prof_mark(void* user, int begin) {
  esl_ctx* c = (esl_ctx*)user;
  if (begin) { if (!c->chol_prof_scope) c->chol_prof_scope = new ProfScope(c, 9); }
  else if (c->chol_prof_scope) { delete (ProfScope*)c->chol_prof_scope; c->chol_prof_scope = nullptr; }
}
static CholRuntime& chol_rt(esl_ctx* c) {
  if (!c->chol_rt) {
    CholRuntime* rt = new CholRuntime();
    rt->prof_mark = chol_prof_mark; rt->prof_user = c;
    c->chol_rt = rt;
  }
  return *(CholRuntime*)c->chol_rt;
}
void slam_sync_side(esl_ctx* c) {
  if (c->chol_rt && ((CholRuntime*)c->chol_rt)->cf_side) (void)hipStreamSynchronize(((CholRuntime*)c->chol_rt)->cf_side);
}
void slam_release_runtime(esl_ctx* c) {
  if (c->chol_prof_scope) { delete (ProfScope*)c->chol_prof_scope; c->chol_prof_scope = nullptr; }
  if (!c->chol_rt) return;
  ((CholRuntime*)c->chol_rt)->release();
  delete (CholRuntime*)c->chol_rt;
  c->chol_rt = nullptr;
  c->schur_attr_set = false;
}

// info: the dense solver's flag word, folded into the "ok" partial and handed on as out[4] (null: no fold -- linearisation, or a
// replicated-graph run, where the flag is only final after its collective: k_slam_fold_info there)
static int reduce_all(esl_ctx* c, const int* info = nullptr) {
  const DevGraph& g = c->g;
  hipLaunchKernelGGL(k_slam_reduce_all, dim3(1), dim3(256), 0, c->stream, c->obj_part, g.n_objs, c->cam_part, g.n_cams, c->od_part,
                     (g.n_odom && g.shard_rank == 0) ? g.n_odom : 0, c->dev_part, info);
  ESL_HIP_TRY(hipGetLastError());
  return ESL_OK;
}

int slam_linearize(esl_ctx* c) {
  c->parts_fresh = false;
  const DevGraph& g = c->g;
  const int N = g.n_objs, F = g.n_cams;
  const bool an = c->lm.p.jacobian_mode == ESL_JAC_ANALYTIC;
  const double delta = c->lm.p.numeric_delta;
  {
    ProfScope ps(c, 0);
    if (N > 0) {
      ChunkTable ct;
      ct.n_chunks = c->n_chunks; ct.obj = c->ck_obj; ct.type = c->ck_type; ct.begin = c->ck_begin; ct.end = c->ck_end; ct.ostart = c->ck_ostart;
      const dim3 block(64 * kLinWaves);
      const int nb_e3 = (c->n_ids_e3 + kLinWaves - 1) / kLinWaves, nb_bb = (c->n_ids_bb + kLinWaves - 1) / kLinWaves;
      // 3-D chunks first (the longer instruction stream), then the bbox chunks, then the per-ellipsoid sums
      robust_dispatch(c->robust_on, [&](auto robust) {
        constexpr bool R = decltype(robust)::value;
        if (an) {
          if (nb_e3) hipLaunchKernelGGL((k_slam_linearize_chunks<ESL_JAC_ANALYTIC, 1, R>), dim3(nb_e3), block, 0, c->stream, g, ct, c->ck_ids_e3, c->n_ids_e3, c->cams,
                                        c->objs, delta, c->chunk_out, c->Wbb, c->Abb);
          if (nb_bb) hipLaunchKernelGGL((k_slam_linearize_chunks<ESL_JAC_ANALYTIC, 0, R>), dim3(nb_bb), block, 0, c->stream, g, ct, c->ck_ids_bb, c->n_ids_bb, c->cams,
                                        c->objs, delta, c->chunk_out, c->Wbb, c->Abb);
          hipLaunchKernelGGL((k_slam_combine<ESL_JAC_ANALYTIC, R>), dim3((N + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kWave * kWavesPerBlock), 0, c->stream, g, ct,
                             c->chunk_out, c->objs, delta, c->Hoo, c->bo, c->obj_part);
        } else {
          if (nb_e3) hipLaunchKernelGGL((k_slam_linearize_chunks<ESL_JAC_NUMERIC, 1, R>), dim3(nb_e3), block, 0, c->stream, g, ct, c->ck_ids_e3, c->n_ids_e3, c->cams,
                                        c->objs, delta, c->chunk_out, c->Wbb, c->Abb);
          if (nb_bb) hipLaunchKernelGGL((k_slam_linearize_chunks<ESL_JAC_NUMERIC, 0, R>), dim3(nb_bb), block, 0, c->stream, g, ct, c->ck_ids_bb, c->n_ids_bb, c->cams,
                                        c->objs, delta, c->chunk_out, c->Wbb, c->Abb);
          hipLaunchKernelGGL((k_slam_combine<ESL_JAC_NUMERIC, R>), dim3((N + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kWave * kWavesPerBlock), 0, c->stream, g, ct,
                             c->chunk_out, c->objs, delta, c->Hoo, c->bo, c->obj_part);
        }
      });
    }
    if (g.n_odom) {
      const dim3 grid((g.n_odom + 127) / 128), block(128);
      robust_dispatch(c->robust_on, [&](auto robust) {
        constexpr bool R = decltype(robust)::value;
        if (an) hipLaunchKernelGGL((k_slam_odom<ESL_JAC_ANALYTIC, R>), grid, block, 0, c->stream, g, c->cams, delta, c->Aod, c->od_part);
        else hipLaunchKernelGGL((k_slam_odom<ESL_JAC_NUMERIC, R>), grid, block, 0, c->stream, g, c->cams, delta, c->Aod, c->od_part);
      });
    }
    hipLaunchKernelGGL(k_slam_cam_gather, dim3((F + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kWave * kWavesPerBlock), 0, c->stream, g, c->Abb, c->Aod,
                       c->Hcc, c->bc, c->cam_part);
    if (c->fx_on && c->fx.n_bb + c->fx.n_e3 > 0) {   // anchored edges (fixed ellipsoid, free camera): camera records, then their per-camera sums
      const AnchGraph& a = c->fx;
      robust_dispatch(c->robust_on, [&](auto robust) {
        constexpr bool R = decltype(robust)::value;
        const dim3 gb((a.n_bb + 63) / 64), ge((a.n_e3 + 63) / 64);
        if (an) {
          if (a.n_bb) hipLaunchKernelGGL((k_anch_linearize<ESL_JAC_ANALYTIC, 0, R>), gb, dim3(64), 0, c->stream, g, a, c->cams, c->objs, delta, c->fx_A, c->fx_chi);
          if (a.n_e3) hipLaunchKernelGGL((k_anch_linearize<ESL_JAC_ANALYTIC, 1, R>), ge, dim3(64), 0, c->stream, g, a, c->cams, c->objs, delta, c->fx_A, c->fx_chi);
        } else {
          if (a.n_bb) hipLaunchKernelGGL((k_anch_linearize<ESL_JAC_NUMERIC, 0, R>), gb, dim3(64), 0, c->stream, g, a, c->cams, c->objs, delta, c->fx_A, c->fx_chi);
          if (a.n_e3) hipLaunchKernelGGL((k_anch_linearize<ESL_JAC_NUMERIC, 1, R>), ge, dim3(64), 0, c->stream, g, a, c->cams, c->objs, delta, c->fx_A, c->fx_chi);
        }
      });
      hipLaunchKernelGGL(k_anch_gather, dim3((F + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kWave * kWavesPerBlock), 0, c->stream, g, a, c->fx_A, c->fx_chi,
                         c->Hcc, c->bc, c->cam_part);
    }
    if (c->comm && !c->comm_replicated) {   // camera blocks of all shards: every rank ends up with the TOTAL Hcc, b_c (3.4 MB at 10k cameras)
      int rc2 = comm_allreduce_sum(c, c->Hcc, (size_t)g.n_free_cams * 36);
      if (!rc2) rc2 = comm_allreduce_sum(c, c->bc, (size_t)g.n_free_cams * 6);
      if (rc2) return rc2;
      hipLaunchKernelGGL(k_slam_cam_maxdiag, dim3((F + 127) / 128), dim3(128), 0, c->stream, g, c->Hcc, c->cam_part);
    }
  }
  ESL_HIP_TRY(hipGetLastError());
  ProfScope ps2(c, 4);
  return reduce_all(c);
}

int slam_build_reduced(esl_ctx* c, double lambda, bool full_sum, void** dev_ptr, int64_t* n_out) {
  const DevGraph& g = c->g;
  const int N = g.n_objs;
  const long n = (long)c->S_n, lda = (long)c->S_lda;
  if (const int rcs = slam_ensure_S(c)) return rcs;
  {
    ProfScope ps(c, 2);
    ESL_HIP_TRY(hipMemsetAsync(c->S, 0, (size_t)lda * (size_t)n * sizeof(double), c->stream));
    const int tot = g.n_free_cams + g.n_odom;
    hipLaunchKernelGGL(k_slam_S_init, dim3((tot + 127) / 128), dim3(128), 0, c->stream, g, c->Hcc, c->bc, c->Aod, lambda, c->S,
                       lda, n);
    if (N > 0) {
      const dim3 grid((N + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
      hipLaunchKernelGGL(k_slam_prepare, grid, block, 0, c->stream, g, lambda, c->Hoo, c->bo, c->Wbb, c->Yb, c->Dinv, c->obj_part, c->Tb,
                         c->Wt);
      if (g.n_free_cams > 0) {
        // the row camera's Y blocks (54 doubles per edge, padded to 55), its list and its ellipsoid bitmap go through LDS when they
        // fit 64 KB; one workgroup per (row camera, group of 64 column cameras) on a 1-D grid (grid.y would cap the cameras at 65,535)
        const size_t ylds = schur_pull_lds_bytes(g.cu_max, g.n_objs);
        const unsigned groups = (unsigned)((g.n_free_cams + 63) / 64);
        const dim3 sgrid(groups * (unsigned)g.n_free_cams);
        if (ylds <= 65536) {
          if (!c->schur_attr_set) { ESL_HIP_TRY(hipFuncSetAttribute((const void*)k_slam_schur_pull<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536)); c->schur_attr_set = true; }
          hipLaunchKernelGGL(k_slam_schur_pull<true>, sgrid, dim3(64), ylds, c->stream, g, c->Wt, c->Yb, c->Tb, c->S, lda, n, groups);
        } else {
          hipLaunchKernelGGL(k_slam_schur_pull<false>, sgrid, dim3(64), 0, c->stream, g, c->Wt, c->Yb, c->Tb, c->S, lda, n, groups);
        }
      }
    }
  }
  ESL_HIP_TRY(hipGetLastError());
  if (c->comm && c->comm_replicated) {
    // whole graph on every rank: S is complete everywhere, nothing to sum
  } else if (c->comm && !full_sum && slam_dist_chol(c)) {
    // distributed factorisation: every outer panel of the summed system goes to its owner only (ncclReduce per panel)
    ProfScope ps(c, 6);
    const int W = chol_outer_panels((int)n), np = (int)((n + kNB - 1) / kNB), n_outer = (np + W - 1) / W;
    for (int o = 0; o < n_outer; ++o) {
      const long c_begin = (long)o * W * kNB, c_end = std::min<long>((long)(o + 1) * W * kNB, (long)n);
      const int rc2 = comm_reduce_sum_root(c, c->S + (size_t)c_begin * lda, (size_t)lda * (size_t)(c_end - c_begin), o % c->comm_ranks);
      if (rc2) return rc2;
    }
  } else if (c->comm) {   // sum of the shards' partial reduced systems (and b_s row): the RCCL all-reduce over xGMI of SURVEY.md §8 e
    ProfScope ps(c, 6);
    int rc2 = comm_allreduce_sum(c, c->S, (size_t)lda * (size_t)n);
    if (rc2) return rc2;
  }
  if (dev_ptr) *dev_ptr = c->S;
  if (n_out) *n_out = n;
  c->lm.lambda_used = lambda;
  return ESL_OK;
}

// chi2 of the anchored edges at the trial cameras (after the camera update of either form, before reduce_all)
static void anch_trial_chi2(esl_ctx* c) {
  if (!c->fx_on || c->fx.n_bb + c->fx.n_e3 == 0) return;
  robust_dispatch(c->robust_on, [&](auto robust) {
    hipLaunchKernelGGL(k_anch_chi2<decltype(robust)::value>, dim3((c->g.n_cams + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kWave * kWavesPerBlock), 0, c->stream,
                       c->g, c->fx, c->cams_trial, c->objs_trial, c->cam_part);
  });
}

// One LM trial of ESL_SOLVER_CAMERA_CHAIN (esl_fixed.hpp): the block-tridiagonal camera system by cyclic reduction, the free
// ellipsoids -- which hang on fixed cameras only -- by their own 9 x 9 solves.  Nothing of arena_solve / arena_S is touched.
static int slam_try_step_chain(esl_ctx* c, double lambda) {
  const DevGraph& g = c->g;
  const int N = g.n_objs, F = g.n_cams, nf = g.n_free_cams;
  if (const int rc = c->chain_ws.grow(c, 0, (size_t)nf * 192 * sizeof(double))) return rc;
  double* const ws = c->chain_ws.at<double>(0);
  double* D[2] = {ws, ws + (size_t)nf * 36};
  double* L[2] = {ws + (size_t)nf * 72, ws + (size_t)nf * 108};
  double* Di = ws + (size_t)nf * 144;
  double* R[2] = {ws + (size_t)nf * 180, ws + (size_t)nf * 186};
  {
    ProfScope ps(c, 3);
    ESL_HIP_TRY(hipMemsetAsync(c->chol_info, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_chain_init, dim3((unsigned)(((long)nf * 36 + 255) / 256)), dim3(256), 0, c->stream, nf, c->Hcc, c->bc, c->Aod, c->cf_od_start, c->cf_od_edge,
                       lambda, D[0], L[0], R[0]);
    int cur = 0;
    // (rows couple only when an odometry edge joins two free cameras; every such edge joins neighbours: chain_ok)
    bool coupled = false;
    for (size_t e = 0; e < c->h_od_i.size() && !coupled; ++e) coupled = c->h_cam_slot[c->h_od_i[e]] >= 0 && c->h_cam_slot[c->h_od_j[e]] >= 0;
    if (coupled)
      for (int d = 1; d < nf; d *= 2) {
        hipLaunchKernelGGL(k_chain_inv, dim3((unsigned)(((long)nf * 6 + 255) / 256)), dim3(256), 0, c->stream, nf, D[cur], Di, c->chol_info);
        hipLaunchKernelGGL(k_chain_step, dim3((unsigned)nf), dim3(64), 0, c->stream, nf, d, D[cur], L[cur], R[cur], Di, D[cur ^ 1], L[cur ^ 1], R[cur ^ 1]);
        cur ^= 1;
      }
    hipLaunchKernelGGL(k_chain_solve, dim3((unsigned)((nf + 63) / 64)), dim3(64), 0, c->stream, nf, D[cur], R[cur], c->xc, c->chol_info);
    ESL_HIP_TRY(hipGetLastError());
  }
  {
    ProfScope ps(c, 1);
    const dim3 grid((N + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
    if (N > 0) {   // x_o = (Hoo + lambda I)^-1 b_o: the ellipsoids' lists of free-camera edges are empty
      hipLaunchKernelGGL(k_slam_prepare, grid, block, 0, c->stream, g, lambda, c->Hoo, c->bo, c->Wbb, c->Yb, c->Dinv, c->obj_part, c->Tb, c->Wt);
      hipLaunchKernelGGL(k_slam_backsub, grid, block, 0, c->stream, g, lambda, c->objs, c->bo, c->Wbb, c->Dinv, c->xc, c->xo, c->objs_trial, c->obj_part);
    }
    hipLaunchKernelGGL(k_slam_cam_update, dim3((F + 127) / 128), dim3(128), 0, c->stream, g, lambda, c->cams, c->xc, c->bc, c->cams_trial, c->cam_part);
    const int nb_co = (N + kWavesPerBlock - 1) / kWavesPerBlock, nb_od = (g.n_odom + kWave * kWavesPerBlock - 1) / (kWave * kWavesPerBlock);
    if (nb_co + nb_od > 0)
      robust_dispatch(c->robust_on, [&](auto robust) {
        hipLaunchKernelGGL(k_slam_chi2_all<decltype(robust)::value>, dim3((unsigned)(nb_co + nb_od)), dim3(kWave * kWavesPerBlock), 0, c->stream, g, nb_co,
                           c->cams_trial, c->objs_trial, c->obj_part, c->od_part);
      });
    anch_trial_chi2(c);
    ESL_HIP_TRY(hipGetLastError());
  }
  return ESL_OK;
}

// ESL_SOLVER_PCG (esl_pcg.hpp): x_c of the reduced camera system by preconditioned conjugate gradients, S never formed.  Leaves Dinv
// and x_c where k_slam_backsub expects them and the verdict in bit 0 of the solver's flag word.  Touches none of arena_S / arena_solve.
static int slam_pcg_solve(esl_ctx* c, double lambda) {
  const DevGraph& g = c->g;
  const int N = g.n_objs, F = g.n_cams, nf = g.n_free_cams;
  const size_t EU = (size_t)g.n_bbox + g.n_e3d, n = (size_t)nf * 6;
  const int nb_obj = std::max(1, (N + kWavesPerBlock - 1) / kWavesPerBlock), nb_cam = (F + kWavesPerBlock - 1) / kWavesPerBlock;
  const int nb_upd = (nf + kPcgBlock - 1) / kPcgBlock;
  // layout of the workspace (doubles)
  size_t off = 0;
  auto take = [&](size_t cnt) { const size_t at = off; off += (cnt + 31) / 32 * 32; return at; };
  const size_t o_st = take(kPcgState), o_M = take((size_t)nf * 36), o_Mi = take((size_t)nf * 36), o_bs = take(n), o_r = take(n), o_z = take(n),
               o_p0 = take(n), o_p1 = take(n), o_q = take(n), o_dbo = take((size_t)N * 9), o_E = take(EU * 6), o_pq = take((size_t)nb_cam),
               o_rz = take(2 * (size_t)nb_upd), o_rr = take(2 * (size_t)nb_upd);
  if (off > c->pcg_ws_cap) {
    if (c->pcg_ws) { ESL_HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipFree(c->pcg_ws); c->pcg_ws = nullptr; c->pcg_ws_cap = 0; }
    const size_t want = off + off / 8;
    ESL_HIP_TRY(hipMalloc((void**)&c->pcg_ws, want * sizeof(double)));
    c->pcg_ws_cap = want;
    c->pcg_reset = true;   // (the counters lived in the old block)
  }
  if (!c->pcg_host) ESL_HIP_TRY(hipHostMalloc((void**)&c->pcg_host, 16 * sizeof(double), hipHostMallocDefault));
  double* ws = c->pcg_ws;
  double* st = ws + o_st;
  double* pbuf[2] = {ws + o_p0, ws + o_p1};
  c->pcg_st = st; c->pcg_M = ws + o_M;
  const esl_pcg_params pp = c->pcg_run;
  const double tol2 = pp.rel_tol * pp.rel_tol;
  const dim3 block(kWave * kWavesPerBlock);
  {
    ProfScope ps(c, 2);
    ESL_HIP_TRY(hipMemsetAsync(c->chol_info, 0, sizeof(int), c->stream));
    ESL_HIP_TRY(hipMemsetAsync(st, 0, kPcgSolves * sizeof(double), c->stream));
    ESL_HIP_TRY(hipMemsetAsync(pbuf[0], 0, std::max<size_t>(n, 1) * sizeof(double), c->stream));
    if (N > 0)
      hipLaunchKernelGGL(k_pcg_setup_obj, dim3((unsigned)((N + kWavesPerBlock - 1) / kWavesPerBlock)), block, 0, c->stream, g, lambda, c->Hoo, c->bo, c->Dinv,
                         ws + o_dbo, c->obj_part, c->chol_info);
    hipLaunchKernelGGL(k_pcg_setup_cam, dim3((unsigned)nb_cam), block, 0, c->stream, g, lambda, c->Hcc, c->bc, c->Wbb, c->Dinv, ws + o_dbo, ws + o_M, ws + o_Mi,
                       ws + o_bs, c->chol_info);
    hipLaunchKernelGGL(k_pcg_update, dim3((unsigned)nb_upd), dim3(kPcgBlock), 0, c->stream, nf, -1, st, c->chol_info, ws + o_pq, nb_cam, ws + o_Mi, ws + o_bs,
                       pbuf[0], ws + o_q, c->xc, ws + o_r, ws + o_z, ws + o_rz, ws + o_rr, nb_upd);
    ESL_HIP_TRY(hipGetLastError());
  }
  {
    ProfScope ps(c, 3);
    int k = 0;
    while (k < pp.max_iters) {
      hipLaunchKernelGGL(k_pcg_obj, dim3((unsigned)nb_obj), block, 0, c->stream, g, k, tol2, st, ws + o_rz, ws + o_rr, nb_upd, c->Wbb, c->Dinv, ws + o_z,
                         pbuf[k & 1], ws + o_E);
      hipLaunchKernelGGL(k_pcg_cam, dim3((unsigned)nb_cam), block, 0, c->stream, g, k, lambda, st, c->Hcc, c->Aod, ws + o_E, ws + o_z, pbuf[k & 1],
                         pbuf[(k + 1) & 1], ws + o_q, ws + o_pq);
      hipLaunchKernelGGL(k_pcg_update, dim3((unsigned)nb_upd), dim3(kPcgBlock), 0, c->stream, nf, k, st, c->chol_info, ws + o_pq, nb_cam, ws + o_Mi, ws + o_bs,
                         pbuf[(k + 1) & 1], ws + o_q, c->xc, ws + o_r, ws + o_z, ws + o_rz, ws + o_rr, nb_upd);
      ++k;
      if (k % pp.check_every == 0 && k < pp.max_iters) {   // the host's look at the done flag
        ESL_HIP_TRY(hipMemcpyAsync(c->pcg_host, st + kPcgDone, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        ESL_HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->pcg_host[0] != 0) break;
      }
    }
    hipLaunchKernelGGL(k_pcg_finish, dim3(1), dim3(kPcgBlock), 0, c->stream, k, tol2, st, ws + o_rr, nb_upd, c->chol_info, c->pcg_reset ? 1 : 0);
    ESL_HIP_TRY(hipGetLastError());
  }
  c->pcg_reset = false;
  c->pcg_ran = true;
  return ESL_OK;
}

int slam_try_step(esl_ctx* c, double lambda) {
  c->parts_fresh = false;
  const DevGraph& g = c->g;
  const int N = g.n_objs, F = g.n_cams;
  int solver = slam_pick_solver(c);
  if (solver == -2) {
    set_error("ESL_SOLVER_CAMERA_CHAIN needs a graph without an active edge between a free camera and a free ellipsoid, odometry edges "
              "that join neighbouring free cameras only, and no communicator");
    return ESL_ERR_INVALID;
  }
  if (solver == -3) {
    set_error("ESL_SOLVER_PCG runs on one GPU: this context has a communicator (multi-GPU PCG is not implemented)");
    return ESL_ERR_INVALID;
  }
  if (solver < 0) {
    set_error("ESL_SOLVER_REDUCED_ELLIPSOID needs odometry edges that join neighbouring free cameras only and, across GPUs, the "
              "replicated-graph communicator (esl_comm_set_replicated); a single GPU always qualifies");
    return ESL_ERR_INVALID;
  }
  int rc;
  if (solver == ESL_SOLVER_REDUCED_ELLIPSOID && c->lm.p.linear_solver == ESL_SOLVER_AUTO && (rc = cf_ensure(c)) != ESL_OK) {
    // AUTO: the camera-first form does not fit beside what else lives on the device -> the reduced camera system for this graph
    if (c->comm && c->comm_ranks > 1) return rc;   // (every rank must take the same form: no unilateral fall-back)
    c->cf_unavailable = true;
    solver = ESL_SOLVER_REDUCED_CAMERA;
  }
  c->lm_solver_used = solver;
  if (solver != ESL_SOLVER_PCG) c->pcg_M = nullptr;   // (esl_lm_download(10): the blocks of the LAST trial's preconditioner only)
  if (solver == ESL_SOLVER_CAMERA_CHAIN) {
    if ((rc = slam_try_step_chain(c, lambda))) return rc;
  } else if (solver == ESL_SOLVER_REDUCED_ELLIPSOID) {
    if ((rc = slam_try_step_cf(c, lambda))) return rc;
    anch_trial_chi2(c);
    ESL_HIP_TRY(hipGetLastError());
  } else {
  if (solver == ESL_SOLVER_PCG) {
    if ((rc = slam_pcg_solve(c, lambda))) return rc;
  } else {
    if ((rc = slam_build_reduced(c, lambda, false, nullptr, nullptr))) return rc;
    ProfScope ps(c, 3);
    ESL_HIP_TRY(hipMemsetAsync(c->chol_info, 0, sizeof(int), c->stream));
    if (c->comm && slam_dist_chol(c)) {
      CholDist d;
      { const int rcp = chol_dist_fill(c, (int)c->S_n, d); if (rcp) return rcp; }
      ESL_HIP_TRY(chol_factor_solve(c->S, (long)c->S_lda, (int)c->S_n, c->Linv_ws, c->z_ws, c->xc, c->chol_info, c->stream, chol_rt(c), &d));
    } else {
      ESL_HIP_TRY(chol_factor_solve(c->S, (long)c->S_lda, (int)c->S_n, c->Linv_ws, c->z_ws, c->xc, c->chol_info, c->stream, chol_rt(c)));
    }
  }
  {
    ProfScope ps(c, 1);
    const dim3 grid((N + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
    if (N > 0)
      hipLaunchKernelGGL(k_slam_backsub, grid, block, 0, c->stream, g, lambda, c->objs, c->bo, c->Wbb, c->Dinv, c->xc, c->xo,
                         c->objs_trial, c->obj_part);
    hipLaunchKernelGGL(k_slam_cam_update, dim3((F + 127) / 128), dim3(128), 0, c->stream, g, lambda, c->cams, c->xc, c->bc,
                       c->cams_trial, c->cam_part);
    const int nb_co = (N + kWavesPerBlock - 1) / kWavesPerBlock, nb_od = (g.n_odom + kWave * kWavesPerBlock - 1) / (kWave * kWavesPerBlock);
    if (nb_co + nb_od > 0)
      robust_dispatch(c->robust_on, [&](auto robust) {
        hipLaunchKernelGGL(k_slam_chi2_all<decltype(robust)::value>, dim3((unsigned)(nb_co + nb_od)), dim3(kWave * kWavesPerBlock), 0, c->stream, g, nb_co,
                           c->cams_trial, c->objs_trial, c->obj_part, c->od_part);
      });
    anch_trial_chi2(c);
  }
  ESL_HIP_TRY(hipGetLastError());
  }
  const bool info_by_collective = c->comm && c->comm_replicated && c->comm_ranks > 1;
  {
    ProfScope ps2(c, 4);
    if ((rc = reduce_all(c, info_by_collective ? nullptr : c->chol_info))) return rc;
  }
  if (info_by_collective) {
    // replicated-graph run: no LM scalars are exchanged, so the pivot check of the panels' OWNERS has to reach every rank here
    // (one 8-byte all-reduce per trial) -- otherwise the owner would reject the step on its flag and the others on the NaNs that
    // came with the broadcast panel, two different exits of the trial loop
    hipLaunchKernelGGL(k_info_to_double, dim3(1), dim3(1), 0, c->stream, c->chol_info, c->dev_scal + 6);
    if ((rc = comm_allreduce_sum(c, c->dev_scal + 6, 1))) return rc;
    hipLaunchKernelGGL(k_double_to_info, dim3(1), dim3(1), 0, c->stream, c->dev_scal + 6, c->chol_info);
    hipLaunchKernelGGL(k_slam_fold_info, dim3(1), dim3(1), 0, c->stream, (const int*)c->chol_info, c->dev_part);
    ESL_HIP_TRY(hipGetLastError());
  }
  // the trial's four scalars and the solver's flag in ONE copy and ONE wait (the flag is already folded into the "ok" partial on the
  // device); esl_lm_try_step's read_parts finds them in the pinned block (parts_fresh)
  ESL_HIP_TRY(hipMemcpyAsync(c->host_part, c->dev_part, 5 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  const int info = (int)c->host_part[4];
  c->parts_fresh = true;
  if (info & 2) {
    // A spin of the one-launch forms ran into its wall-clock bound (3 s): the kernel was preempted or time-sliced for that long
    // (two processes on one GPU, a debugger, a profiler) or a producer never became resident.  The factorisation itself is not
    // wrong, so the trial is redone ONCE with the launch-per-step factorisation and back-substitution, which have no device-side
    // waits, and the context keeps that form from then on.  Not in a multi-rank run: the other ranks would not redo
    // their collectives.
    CholRuntime& rt = chol_rt(c);
    const bool can_retry = !(c->comm && c->comm_ranks > 1) && !(rt.sw.persistent == 0 && rt.sw.backsub_launches);
    if (!can_retry) { set_error("dense solver: a device-side hand-off timed out (k_chol_backsub / persistent panel kernel)"); return ESL_ERR_HIP; }
    rt.sw.persistent = 0; rt.sw.backsub_launches = true; rt.fallbacks += 1;
    fprintf(stderr, "[libesl_hip] a device-side hand-off of the dense solver timed out; this context now uses the launch-per-step form\n");
    ESL_HIP_TRY(hipMemsetAsync(c->chol_info, 0, sizeof(int), c->stream));
    c->parts_fresh = false;
    return slam_try_step(c, lambda);
  }
  return ESL_OK;
}

// ---- diagnostic: residual of the reduced camera system ------------------------------------------------------------------
// y += S x for the LOWER-triangle storage of S (column-major, lda): workgroup = (row tile of 256, column panel of 64) with
// row tile >= column panel; loads run down the columns (coalesced); an entry S_ij (i > j) serves y_i and y_j.
static __global__ __launch_bounds__(256) void k_symv_lower(const double* __restrict__ M, long lda, long n, const double* __restrict__ x,
                                                           double* __restrict__ y) {
  __shared__ double ycol[64];
  __shared__ double xcol[64];
  const long j0 = (long)blockIdx.y * 64, i0 = (long)blockIdx.x * 256;
  if (i0 + 255 < j0) return;                         // tile entirely above the diagonal
  const long i = i0 + threadIdx.x;
  if (threadIdx.x < 64) { ycol[threadIdx.x] = 0; xcol[threadIdx.x] = (j0 + threadIdx.x < n) ? x[j0 + threadIdx.x] : 0.0; }
  __syncthreads();
  const double xi = i < n ? x[i] : 0.0;
  double acc = 0;
  if (i < n) {
    for (int jj = 0; jj < 64; ++jj) {
      const long j = j0 + jj;
      if (j >= n || j > i) break;
      const double a = M[i + j * lda];
      acc += a * xcol[jj];
      if (i > j) atomicAdd(&ycol[jj], a * xi);
    }
    if (acc != 0) atomicAdd(&y[i], acc);
  }
  __syncthreads();
  if (threadIdx.x < 64 && j0 + threadIdx.x < n && ycol[threadIdx.x] != 0) atomicAdd(&y[j0 + threadIdx.x], ycol[threadIdx.x]);
}
static __global__ __launch_bounds__(256) void k_resid_norms(const double* __restrict__ M, long lda, long n, const double* __restrict__ y,
                                                            double* __restrict__ out2) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  double r2 = 0, b2 = 0;
  if (j < n) { const double b = M[n + j * lda], r = y[j] - b; r2 = r * r; b2 = b * b; }
  r2 = wave_sum(r2); b2 = wave_sum(b2);
  if ((threadIdx.x & 63) == 0) { atomicAdd(&out2[0], r2); atomicAdd(&out2[1], b2); }
}

}  // namespace esl

extern "C" int esl_lm_reduced_residual(esl_ctx* c, double* rel_residual_out) {
  using namespace esl;
  if (!c || !rel_residual_out) return ESL_ERR_INVALID;
  if (!c->lm.begun || !c->lm.slam || !c->xc || c->S_n <= 0) { set_error("esl_lm_reduced_residual: needs a SLAM-mode trial step"); return ESL_ERR_STATE; }
  // (works after a step of either form: x_c of the camera-first elimination solves the same reduced camera system)
  ESL_HIP_TRY(hipSetDevice(c->device));
  const long n = (long)c->S_n, lda = (long)c->S_lda;
  // the factorisation overwrote S and b_s; full_sum: in a sharded run EVERY rank needs the summed system here (the per-panel
  // reduce of the distributed factorisation would leave unsummed partials outside a rank's own panels)
  int rc = slam_build_reduced(c, c->lm.lambda_used, true, nullptr, nullptr);
  if (rc) return rc;
  double* y = nullptr;
  ESL_HIP_TRY(hipMalloc((void**)&y, ((size_t)n + 2) * sizeof(double)));
  hipError_t e = hipMemsetAsync(y, 0, ((size_t)n + 2) * sizeof(double), c->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_symv_lower, dim3((unsigned)((n + 255) / 256), (unsigned)((n + 63) / 64)), dim3(256), 0, c->stream, c->S, lda, n,
                       c->xc, y);
    hipLaunchKernelGGL(k_resid_norms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->S, lda, n, y, y + n);
    e = hipGetLastError();
  }
  double h2[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(h2, y + n, sizeof(h2), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(y);
  if (e != hipSuccess) { set_error(std::string("esl_lm_reduced_residual: ") + hipGetErrorString(e)); return ESL_ERR_HIP; }
  *rel_residual_out = h2[1] > 0 ? std::sqrt(h2[0] / h2[1]) : 0.0;
  return ESL_OK;
}

// ---- dense-solver self test / micro-benchmark ------------------------------------------------------------------------
// A(i,j) = h(min,max) in [-1,1) off the diagonal (a hash, so the matrix never has to be kept), A(i,i) = n: strictly
// diagonally dominant, hence SPD.  b = A * 1 + known perturbation -> the solve must return x with A x = b.
namespace esl {
__device__ __forceinline__ double st_entry(long i, long j, long n) {
  if (i == j) return (double)n;
  const unsigned long long a = (unsigned long long)(i < j ? i : j), b = (unsigned long long)(i < j ? j : i);
  unsigned long long h = a * 0x9E3779B97F4A7C15ull ^ (b + 0x7F4A7C15ull) * 0xC2B2AE3D27D4EB4Full;
  h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
  return (double)(h >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}
__device__ __forceinline__ double st_rhs(long i) { return 1.0 + 0.001 * (double)(i % 97); }
static __global__ void k_selftest_fill(double* __restrict__ M, long lda, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i > n || j >= n) return;
  double v = 0;
  if (i == n) v = st_rhs(j);          // row n carries b^T
  else if (i >= j) v = st_entry(i, j, n);
  M[i + j * lda] = v;
}
// one workgroup per row: r_i = b_i - sum_j A(i,j) x_j ;  accumulates |r|^2 and |b|^2
static __global__ __launch_bounds__(256) void k_selftest_resid(const double* __restrict__ x, long n, double* __restrict__ out2) {
  __shared__ double red[256];
  const long i = blockIdx.x;
  double s = 0;
  for (long j = threadIdx.x; j < n; j += 256) s += st_entry(i, j, n) * x[j];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) { if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st]; __syncthreads(); }
  if (threadIdx.x == 0) {
    const double b = st_rhs(i), r = b - red[0];
    atomicAdd(&out2[0], r * r);
    atomicAdd(&out2[1], b * b);
  }
}
}  // namespace esl

extern "C" int esl_selftest_cholesky(esl_ctx* c, int32_t n, double* ms_out, double* rel_residual_out) {
  using namespace esl;
  if (!c || n < 1 || !ms_out || !rel_residual_out) return ESL_ERR_INVALID;
  ESL_HIP_TRY(hipSetDevice(c->device));
  const long lda = (((long)n + 1 + 127) / 128) * 128;
  double *M = nullptr, *Linv = nullptr, *z = nullptr, *x = nullptr, *out2 = nullptr;
  int* info = nullptr;
  const size_t np = (size_t)((n + kNB - 1) / kNB);
  int rc = ESL_OK;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto cleanup = [&]() {
    if (M) (void)hipFree(M); if (Linv) (void)hipFree(Linv); if (z) (void)hipFree(z); if (x) (void)hipFree(x);
    if (out2) (void)hipFree(out2); if (info) (void)hipFree(info);
    if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1);
  };
#define ST_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); cleanup(); return ESL_ERR_HIP; } } while (0)
  ST_TRY(hipMalloc((void**)&M, (size_t)lda * (size_t)n * sizeof(double)));
  ST_TRY(hipMalloc((void**)&Linv, np * kNB * kNB * sizeof(double)));
  ST_TRY(hipMalloc((void**)&z, kNB * sizeof(double)));
  ST_TRY(hipMalloc((void**)&x, (size_t)n * sizeof(double)));
  ST_TRY(hipMalloc((void**)&out2, 2 * sizeof(double)));
  ST_TRY(hipMalloc((void**)&info, sizeof(int)));
  ST_TRY(hipEventCreate(&e0)); ST_TRY(hipEventCreate(&e1));
  ST_TRY(hipMemsetAsync(out2, 0, 2 * sizeof(double), c->stream));
  ST_TRY(hipMemsetAsync(info, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(k_selftest_fill, dim3((unsigned)((n + 1 + 255) / 256), (unsigned)n), dim3(256), 0, c->stream, M, lda, (long)n);
  ST_TRY(hipEventRecord(e0, c->stream));
  ST_TRY(chol_factor_solve(M, lda, n, Linv, z, x, info, c->stream, chol_rt(c)));
  ST_TRY(hipEventRecord(e1, c->stream));
  if (chol_rt(c).sw.debug) {             // a stream created and destroyed while the factorisation runs: the disturbance that made the
    hipStream_t w2 = nullptr;             // scheduler time-slice the first (two-kernel) persistent form
    if (hipStreamCreateWithFlags(&w2, hipStreamNonBlocking) == hipSuccess) (void)hipStreamDestroy(w2);
  }
  hipLaunchKernelGGL(k_selftest_resid, dim3((unsigned)n), dim3(256), 0, c->stream, x, (long)n, out2);
  double h2[2] = {0, 0};
  int hinfo = 0;
  ST_TRY(hipMemcpyAsync(h2, out2, sizeof(h2), hipMemcpyDeviceToHost, c->stream));
  ST_TRY(hipMemcpyAsync(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  ST_TRY(hipStreamSynchronize(c->stream));
  float ms = 0;
  ST_TRY(hipEventElapsedTime(&ms, e0, e1));
#undef ST_TRY
  if (chol_rt(c).sw.timing) chol_print_timing(n);
  *ms_out = ms;
  *rel_residual_out = h2[1] > 0 ? std::sqrt(h2[0] / h2[1]) : 0.0;
  if (hinfo & 2) { set_error("self test: a device-side hand-off of the dense solver timed out"); rc = ESL_ERR_HIP; }
  else if (hinfo) { set_error("self test: non-positive pivot"); rc = ESL_ERR_STATE; }
  cleanup();
  return rc;
}


extern "C" int esl_lm_solver_stats(esl_ctx* c, double* st) {
  if (!c || !st) return ESL_ERR_INVALID;
  for (int k = 0; k < ESL_SOLVER_STATS; ++k) st[k] = 0;
  if (c->lm_solver_used != ESL_SOLVER_REDUCED_ELLIPSOID || !c->cf_ready) return ESL_OK;
  const esl::CfPlan& pl = c->cf_plan;
  st[0] = pl.sparse ? pl.form : 0;
  st[1] = pl.stride; st[2] = pl.n_sep; st[3] = pl.n_seg;
  if (pl.sparse) {
    st[4] = 2.0 * pl.sp_flops;   // (FMAs of the block lower triangles, rows from each block row's first camera on)
    st[5] = pl.form == 1 ? 8.0 * 81.0 * (double)pl.p_blocks : 0.0;
    if (pl.form == 3) { st[4] = pl.os_flops; st[5] = 8.0 * (double)pl.y_len; }   // (the one-sided assembly's products; bytes of Y)
    st[6] = 8.0 * (double)pl.xc_len;
  }
  st[7] = (double)(pl.sparse ? pl.kpad_s : pl.kpad);
  st[8] = pl.tperm ? pl.upd_flops : 0.0;   // (0: the whole lower triangle times K)
  st[9] = pl.tperm ? 1.0 : 0.0;
  return ESL_OK;
}
extern "C" int esl_lm_os_counts(esl_ctx* c, double* n) {
  if (!c || !n) return ESL_ERR_INVALID;
  for (int k = 0; k < ESL_OS_COUNTS; ++k) n[k] = 0;
  if (c->lm_solver_used != ESL_SOLVER_REDUCED_ELLIPSOID || !c->cf_ready) return ESL_OK;
  const esl::CfPlan& pl = c->cf_plan;
  if (!pl.sparse || pl.form != 3) return ESL_OK;
  n[0] = (double)pl.os_npairs; n[1] = (double)pl.osm_row_npairs; n[2] = (double)pl.osm_npairs;
  n[3] = (double)pl.os_list_npairs; n[4] = pl.os_list ? pl.osm_flops : pl.os_flops; n[5] = 8.0 * (double)pl.os_list_npairs;
  return ESL_OK;
}
extern "C" int esl_lm_pcg_stats(esl_ctx* c, double* st) {
  if (!c || !st) return ESL_ERR_INVALID;
  for (int k = 0; k < ESL_PCG_STATS; ++k) st[k] = 0;
  if (!c->pcg_ran || !c->pcg_st) return ESL_OK;
  ESL_HIP_TRY(hipSetDevice(c->device));
  double h[esl::kPcgState];
  ESL_HIP_TRY(hipMemcpyAsync(h, c->pcg_st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  st[0] = h[esl::kPcgIters];
  st[1] = h[esl::kPcgBb] > 0 ? std::sqrt(h[esl::kPcgRr] / h[esl::kPcgBb]) : 0.0;
  st[2] = h[esl::kPcgConv];
  if (!c->pcg_reset) { st[3] = h[esl::kPcgSolves]; st[4] = h[esl::kPcgIterSum]; }
  st[5] = c->pcg_run.max_iters; st[6] = c->pcg_run.rel_tol;
  return ESL_OK;
}
extern "C" int esl_lm_solver_used(esl_ctx* c, int32_t* solver_out) {
  if (!c || !solver_out) return ESL_ERR_INVALID;
  *solver_out = c->lm_solver_used;
  return ESL_OK;
}

// test / debug: the task list of the persistent dense factorisation (esl_chol.hpp) for an order-n system with outer panels of W
// 128-panels -- a pure host function (tests/test_chol_plan.py replays it on the CPU: order, dependency words, result)
extern "C" int esl_debug_chol_plan(int32_t n, int32_t W, int32_t filler, int32_t* tasks_out /* 4 per task */, int64_t cap_tasks,
                                   int32_t* ns_out /* np x nR */, int64_t cap_ns, int32_t meta_out[5] /* np, n_outer, nR, n_tasks, W */) {
  if (n < 1 || W < 1 || !meta_out) return ESL_ERR_INVALID;
  esl::CholPlan pl;
  esl::chol_plan_from_switches(esl::chol_switches_from_env(), n, W, filler, pl);   // (a fresh read per call: the tests change the plan switches between calls)
  meta_out[0] = pl.np; meta_out[1] = pl.n_outer; meta_out[2] = pl.nR; meta_out[3] = (int32_t)pl.tasks.size(); meta_out[4] = pl.W;
  if (tasks_out) {
    if ((int64_t)pl.tasks.size() > cap_tasks) return ESL_ERR_INVALID;
    for (size_t i = 0; i < pl.tasks.size(); ++i) { tasks_out[4 * i] = pl.tasks[i].type; tasks_out[4 * i + 1] = pl.tasks[i].a; tasks_out[4 * i + 2] = pl.tasks[i].b; tasks_out[4 * i + 3] = pl.tasks[i].c; }
  }
  if (ns_out) {
    if ((int64_t)pl.ns.size() > cap_ns) return ESL_ERR_INVALID;
    for (size_t i = 0; i < pl.ns.size(); ++i) ns_out[i] = pl.ns[i];
  }
  return ESL_OK;
}

// test / debug: would chol_launch_update run this region on k_chol_update_v, the tile with the assign form and the occupancy cap
// (esl_chol.hpp)?  A pure host function, the switches read per call
extern "C" int esl_debug_update_v_applies(int64_t lda, int64_t rows, int64_t base, int64_t col_limit, int32_t ext, int64_t ldp, int32_t* applies_out) {
  if (!applies_out) return ESL_ERR_INVALID;
  *applies_out = esl::chol_update_v_applies(esl::chol_switches_from_env(), (long)lda, (long)rows, (long)base, (long)col_limit, ext != 0, (long)ldp) ? 1 : 0;
  return ESL_OK;
}

// test / debug: the segment length the layout would choose for form 3 from these counts (esl_cf_plan.hpp, cf_stride_choose), and the
// model's ms per stride.  A pure host function
extern "C" int esl_debug_cf_stride_choose(int64_t n_o, const double upd_flops[3], const double pairs[3], const double slab[3], int32_t* stride_out,
                                          double ms_out[3]) {
  if (!upd_flops || !pairs || !slab || !stride_out) return ESL_ERR_INVALID;
  *stride_out = esl::cf_stride_choose((long)n_o, upd_flops, pairs, slab);
  if (ms_out) for (int m = 0; m < 3; ++m) ms_out[m] = esl::cf_stride_cost(upd_flops[m], pairs[m], slab[m]);
  return ESL_OK;
}
