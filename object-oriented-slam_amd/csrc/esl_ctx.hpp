// esl_ctx.hpp — context / device-resident graph shared by the translation units of libesl_hip.so
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/esl.h"
#include "esl_cf_plan.hpp"   // CfPlan (host only)
#include "esl_math.hpp"

namespace esl {

void set_error(const std::string& s);
#define ESL_HIP_TRY(expr)                                                                         \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      esl::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                          \
      return ESL_ERR_HIP;                                                                         \
    }                                                                                             \
  } while (0)

// Device-resident graph: edges sorted by ellipsoid (CSR), camera-side CSR for the SLAM-mode gather.
struct DevGraph {
  int n_cams = 0, n_objs = 0;
  int n_bbox = 0, n_e3d = 0, n_odom = 0;   // extents of the edge arrays (appendable layout: including the slack behind the slices)
  int n_bbox_edges = 0;                    // bbox edges that exist (= n_bbox unless the layout has slack)
  double K[4];
  double grav_n[3];
  double grav_w = 0;
  int check_vis = 0, img_rows = 0, img_cols = 0;   // esl_graph::check_visibility / image_rows / image_cols
  int bbox_mode = 0;   // esl_lm_params::bbox_residual of the current run (0 reprojection, 1 plane tangency)
  int rk_kind[ESL_EDGE_CLASSES] = {0, 0, 0, 0};       // esl_lm_set_robust of the current run, per esl_edge_class: read by the
  double rk_delta[ESL_EDGE_CLASSES] = {1, 1, 1, 1};   // ROBUST = true kernel instantiations only
  YawTable yt;
  // per ellipsoid
  int* bb_start = nullptr;   // n_objs + 1
  int* e3_start = nullptr;   // n_objs + 1
  int* gr_cnt = nullptr;     // n_objs : number of gravity-prior edges on this ellipsoid
  // bbox edges, sorted by ellipsoid (stable)
  int* bb_cam = nullptr; int* bb_obj = nullptr;
  double* bb_meas = nullptr; double* bb_w = nullptr;
  unsigned char* bb_valid = nullptr;
  // 3-D edges, sorted by ellipsoid (stable)
  int* e3_cam = nullptr; int* e3_obj = nullptr;
  double* e3_meas = nullptr; double* e3_w = nullptr;
  // odometry
  int* od_i = nullptr; int* od_j = nullptr; double* od_meas = nullptr; double* od_info = nullptr;
  // cameras
  unsigned char* cam_fixed = nullptr;  // n_cams
  int* cam_slot = nullptr;             // n_cams: index among free cameras or -1
  int n_free_cams = 0;
  // camera-side CSR over (bbox, e3d) edges for H_cc / b_c gathers (SLAM mode)
  int* cbb_start = nullptr; int* cbb_edge = nullptr;
  int* ce3_start = nullptr; int* ce3_edge = nullptr;
  int* cod_start = nullptr; int* cod_edge = nullptr;  // odometry edges touching each camera (edge*2 + side)
  // per ellipsoid: unified list of edges whose camera is free (u = bbox index, or n_bbox + 3-D index)
  int* ue_start = nullptr; int* ue_id = nullptr; int* ue_slot = nullptr;
  int n_ue = 0;
  // per free camera (slot): its edges sorted by (ellipsoid, u) -- the deterministic Schur complement walks two of these lists
  int* cu_start = nullptr; int* cu_obj = nullptr; int* cu_id = nullptr;
  int cu_max = 0;   // longest per-camera list (k_slam_schur_pull stages the row camera's Y blocks in LDS when they fit)
  // sharding (SLAM mode): odometry edges, the camera blocks' lambda and the camera part of the LM scale are
  // replicated on every rank and must enter the summed system once -> only shard_rank 0 contributes them
  int shard_rank = 0;
};

// doubles in the camera-side record of one edge: A = Jc^T w Jc (21 packed) and g = -Jc^T w r (6)
constexpr int kARec = 27;

// edges of FIXED ellipsoids (esl_graph_upload_fixed; kernels: esl_fixed.hpp)
struct AnchGraph {
  int n_bb = 0, n_e3 = 0;           // anchored edges: [0, n_bb) / [0, n_e3), sorted by camera slot (stable)
  int n_bb_all = 0, n_e3_all = 0;   // + the inactive edges behind them
  int* bb_cam = nullptr; int* bb_obj = nullptr; double* bb_meas = nullptr; double* bb_w = nullptr; unsigned char* bb_valid = nullptr;
  int* e3_cam = nullptr; int* e3_obj = nullptr; double* e3_meas = nullptr; double* e3_w = nullptr;
  int* bb_start = nullptr; int* e3_start = nullptr;   // n_free_cams + 1 each: the anchored edges of every camera slot
};

// robust kernel of edge class `cls` on an edge's raw chi2: chi <- rho0(chi), w <- rho1(chi) w (g2o robustInformation).  The compile-time
// switch keeps the default instantiations exactly what they were (a run-time flag costs registers and occupancy: esl_kernels_chunk.hpp).
template <bool ROBUST>
__device__ __forceinline__ void robust_edge(const DevGraph& g, int cls, double& chi, double& w) {
  if (ROBUST) {
    double r0, r1;
    robustify(g.rk_kind[cls], g.rk_delta[cls], chi, r0, r1);
    chi = r0; w *= r1;
  }
}
// the merged gravity prior of an ellipsoid with ng edges, residual rg: weight of its J^T J (in: grav_w ng) and its chi2 (in: wg rg^2)
// become ng rho1 grav_w and ng rho0(grav_w rg^2)
template <bool ROBUST>
__device__ __forceinline__ void robust_grav(const DevGraph& g, int ng, double rg, double& wg, double& chi) {
  if (ROBUST) {
    double r0, r1;
    robustify(g.rk_kind[ESL_EDGE_GRAVITY], g.rk_delta[ESL_EDGE_GRAVITY], g.grav_w * rg * rg, r0, r1);
    chi = ng * r0; wg = (g.grav_w * ng) * r1;
  }
}

// launch helper: f(std::true_type) when the run has a robust kernel on some edge class, f(std::false_type) otherwise
template <class F>
inline void robust_dispatch(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

struct HostImage;   // esl_graph.hip
// the map-side calls' buffers, each defined by the translation unit named after it (InitBatchState: esl_init.hip)
struct RelocState; struct AssocState; struct MergeState; struct RenderState; struct InitBatchState; struct DenseState;
struct LmState {
  bool begun = false;
  esl_lm_params p;
  bool slam = false;          // any free camera
  double lambda_used = 0;
  bool have_trial = false;
};

}  // namespace esl

#include "esl_scratch.hpp"   // ScratchSet: after set_error / ESL_HIP_TRY, ahead of esl_ctx

// device blob + its pinned staging twin + the event of the last staging -> device copy
struct BlobArena { char* dev = nullptr; size_t cap = 0; char* host = nullptr; size_t host_cap = 0; hipEvent_t ev = nullptr; };
struct esl_ctx;
namespace esl {
// RAII event bracket around a group of launches of one kernel class
struct ProfScope {
  esl_ctx* c; int slot;
  ProfScope(esl_ctx* ctx, int kind);
  ~ProfScope();
};
int prof_drain(esl_ctx* c);
void fit_graphs_clear(esl_ctx* c);
void fit_release(esl_ctx* c);
void plane_release(esl_ctx* c);
void reloc_release(esl_ctx* c);   // esl_reloc.hip
void assoc_release(esl_ctx* c);   // esl_assoc.hip
void merge_release(esl_ctx* c);   // esl_merge.hip
void render_release(esl_ctx* c);  // esl_render.hip
void dense_release(esl_ctx* c);   // esl_dense.hip: the map and its two extractors
void init_batch_release(esl_ctx* c);   // esl_init.hip
// esl_debug_scratch_allocs: each owner's counters, written only when its state exists
void reloc_scratch_stats(const esl_ctx* c, int64_t* allocs, int64_t* bytes);
void assoc_scratch_stats(const esl_ctx* c, int64_t* allocs, int64_t* bytes);
void merge_scratch_stats(const esl_ctx* c, int64_t* allocs, int64_t* bytes);
void render_scratch_stats(const esl_ctx* c, int64_t* allocs, int64_t* bytes);
void init_scratch_stats(const esl_ctx* c, bool robust, int64_t* allocs, int64_t* bytes);
void dense_scratch_stats(const esl_ctx* c, int64_t* allocs, int64_t* bytes);   // esl_debug_dense_allocs: no esl_scratch_owner of its own
// all-gather the 8-double dev_scal block of every rank into c->dev_gather (device), ordered on the context's stream
int comm_gather_scalars_device(esl_ctx* c);
// SLAM mode: in-place sum over ranks of a device buffer (RCCL all-reduce); no-op without a communicator
int comm_allreduce_sum(esl_ctx* c, double* dev_buf, size_t count, hipStream_t st = nullptr);
int comm_reduce_sum_root(esl_ctx* c, double* dev_buf, size_t count, int root);   // sum over the ranks, delivered to root
int comm_bcast(esl_ctx* c, double* dev_buf, size_t count, int root, hipStream_t st = nullptr);
// replicated-graph communicator: compare this graph's structure fingerprint across the ranks (once per upload); ESL_ERR_STATE on a mismatch
int comm_check_replicated(esl_ctx* c);
// {sum, max, sum, min} of 4 device scalars over ranks -> host
int comm_reduce4(esl_ctx* c, const double* dev_src4, double out[4]);
}  // namespace esl

struct esl_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  esl::DevGraph g;
  bool graph_loaded = false;
  bool states_loaded = false;
  // states: current and trial (pointer swap on accept)
  double* cams = nullptr; double* cams_trial = nullptr;   // n_cams x 7
  double* objs = nullptr; double* objs_trial = nullptr;   // n_objs x 10
  // mapping-mode system
  double* Hoo = nullptr;      // n_objs x 45 packed upper
  double* bo = nullptr;       // n_objs x 9
  double* xo = nullptr;       // n_objs x 9
  double* obj_part = nullptr; // n_objs x 4 : chi2, maxdiag, scale, ok
  // SLAM-mode system
  double* Hcc = nullptr;      // n_free_cams x 36 diagonal blocks
  double* bc = nullptr;       // n_free_cams x 6
  double* xc = nullptr;       // n_free_cams x 6 (solution of the reduced system)
  double* Wbb = nullptr;      // n_bbox x 54  (H_co blocks, 6x9 row-major)
  double* Abb = nullptr;      // n_bbox x 27 (per-edge camera contributions: 21 packed + 6)
  double* Aod = nullptr;      // n_odom x (2*27 + 36): per-edge Hii, bi, Hjj, bj packed, Hij full
  double* Dinv = nullptr;     // n_objs x 81
  double* Yb = nullptr;       // [EU][54] : W D^-1, one record per edge
  double* Wt = nullptr;       // [EU][9][6] : W as per-edge records (k_slam_schur_pull)
  double* Tb = nullptr;       // [6][EU] : Y_e b_o per edge (its share of b_s), summed per camera by the Schur kernel
  double* S = nullptr;        // n x (n+1) column-major reduced system [S | b_s], n = 6 n_free_cams
  int64_t S_n = 0;
  double* cam_part = nullptr; // n_cams x 4
  double* od_part = nullptr;  // n_odom : chi2 per odometry edge
  int* chol_info = nullptr;
  // reductions
  double* host_part = nullptr;  // pinned: 16 doubles
  double* dev_part = nullptr;
  esl::LmState lm;
  esl_robust_params robust = {{0, 0, 0, 0}, {1, 1, 1, 1}};   // esl_lm_set_robust; copied into g at the start of every run
  bool robust_on = false;                                     // the current run has a kernel on some class: ROBUST instantiations
  // caller order -> slot of the ellipsoid-sorted edge arrays (esl_edge_chi2), kept across esl_graph_append; gravity: caller's ellipsoids
  std::vector<int> h_bb_slot_of, h_e3_slot_of, h_grav_obj;
  esl::Scratch eq_buf;   // esl_edge_chi2: 2 doubles per slot
  double* cams_snap = nullptr; double* objs_snap = nullptr;
  // profiling (HIP events on this stream)
  bool prof_on = false;
  int prof_level = 0;   // 1: only kernel class 0 (linearise) is bracketed; 2: every class
  unsigned prof_runs = 0; // level 1: device-driven runs since esl_profile_enable (every 4th one carries the sampled launch)
  bool prof_gate = true; // level 1 inside a device-driven run: bracket ONE linearisation per run (event records break
                         // the back-to-back dispatch: bracketing all of them cost 13 % of the C4 run)
  std::vector<hipEvent_t> prof_ev;   // pairs
  std::vector<int> prof_kind;
  size_t prof_used = 0;
  int64_t prof_count[ESL_PROF_KINDS] = {0};
  double prof_ms[ESL_PROF_KINDS] = {0};
  // host copies kept from upload (edge -> camera after sorting by ellipsoid)
  std::vector<int> h_bb_cam, h_bb_obj, h_e3_cam, h_e3_obj, h_cam_slot, h_od_i, h_od_j;
  // chunked mapping-mode pipeline (esl_kernels_chunk.hpp)
  int n_chunks = 0;
  int *ck_obj = nullptr, *ck_type = nullptr, *ck_begin = nullptr, *ck_end = nullptr, *ck_ostart = nullptr;
  int *ck_ids_bb = nullptr, *ck_ids_e3 = nullptr; int n_ids_bb = 0, n_ids_e3 = 0;
  double* chunk_out = nullptr;   // n_chunks x 56
  double* chunk_out2 = nullptr;  // second buffer: speculative linearisation of the trial state
  hipEvent_t ev_try = nullptr;
  double* chunk_chi = nullptr;   // n_chunks
  double* blk_part = nullptr;    // per-workgroup partials of k_chunk_finalize
  double* solve_part = nullptr;  // per-workgroup partials of k_obj_solve / k_lm_step (4 each)
  double* blk_chi = nullptr;     // per-workgroup chi2 of the last linearisation
  unsigned int* tickets = nullptr;  // 2 arrival counters
  double* dev_scal = nullptr;    // {chi2_lin, max_diag}
  esl::HostImage* append_img = nullptr;   // host image of the appendable layout (esl_graph_append, esl_graph.hip)
  char* append_dev = nullptr; size_t append_dev_cap = 0;   // device scratch of an append's staged blob
  char* slam_tab_dev = nullptr; size_t slam_tab_cap = 0;   // SLAM-mode append: the camera-side tables + odometry arrays, rebuilt per append (esl_graph.hip)
  // grow-only arenas behind esl_graph_upload (esl_graph.hip)
  char* arena_graph = nullptr; size_t arena_graph_cap = 0;
  char* arena_work = nullptr;  size_t arena_work_cap = 0;
  char* stage_host = nullptr;  size_t stage_host_cap = 0;   // pinned staging blob
  // grow-only blobs of SLAM mode (esl_slam.hip BlobStage): what slam_alloc builds at upload / what the first trial's solver needs
  // arena_solve: the camera-first form's tables, slabs and T; arena_S: the reduced camera system S + its solver workspace.  Separate
  // blobs since round 5: a graph normally runs ONE form, but esl_lm_reduced_system / esl_lm_reduced_residual build S
  // beside a camera-first run, and with one shared blob that re-laid out (and memset) the camera-first set under the caller's feet.
  BlobArena arena_slam, arena_solve, arena_S;
  const int *h_cu_start = nullptr, *h_cu_obj = nullptr, *h_cu_id = nullptr;   // the per-camera lists in arena_slam's staging blob
  std::vector<int> h_ue_start, h_ue_id, h_ue_slot;   // host copy of the unified per-ellipsoid edge lists (the camera-first tables are built from it on first use)
  char* fit_slab = nullptr; size_t fit_slab_cap = 0;        // esl_fit_frame's device slab (esl_fit.hip)
  char* fit_in = nullptr;  size_t fit_in_cap = 0;           // pinned staging of its inputs / outputs
  char* fit_out = nullptr; size_t fit_out_cap = 0;
  esl::Scratch plane_slab;                                   // esl_extract_ground_plane / esl_extract_planes (esl_plane.hip)
  esl::RelocState* reloc = nullptr;                               // esl_reloc_set_map / esl_relocalize: the map and the search's buffers (esl_reloc.hip RelocState)
  esl::AssocState* assoc = nullptr;                               // esl_predict_boxes / esl_associate_boxes: their buffers (esl_assoc.hip AssocState)
  esl::MergeState* merge = nullptr;                               // esl_map_overlaps / esl_map_merge: their buffers (esl_merge.hip MergeState)
  esl::RenderState* render = nullptr;                             // esl_render_map: its buffers (esl_render.hip RenderState)
  esl::DenseState* dense = nullptr;                               // esl_dense_*: the map's tables and the calls' buffers (esl_dense_int.hpp DenseState)
  esl::InitBatchState* init_batch = nullptr;                     // esl_init_quadrics: its buffers (esl_init.hip InitBatchState)
  void* fit_graph_cache = nullptr;                         // captured launch sequences (std::vector<FitGraphEntry>)
  bool parts_fresh = false;      // host_part holds the last trial's scalars already (slam_try_step fetched them with the solver's flag)
  bool cams_match_snap = false;  // cameras untouched since the snapshot: esl_states_restore skips their copy
  int n_grav_edges = 0;
  void* lm_dev = nullptr;        // device-resident LM state (LmCore[2], esl_kernels_chunk.hpp)
  void* lm_host = nullptr;       // mapped pinned LmHostView the host polls
  void* lm_host_dev = nullptr;   // its device alias
  void* host_scal = nullptr;     // mapped pinned LmScalars
  void* host_scal_dev = nullptr; // its device alias
  bool sys_combined = false;
  // RCCL exchange (esl_comm.hip)
  void* comm = nullptr;          // ncclComm_t
  int comm_ranks = 1, comm_rank = 0;
  bool comm_replicated = false;  // esl_comm_set_replicated: every rank holds the whole graph; only the dense solve is divided
  esl_host_allreduce_fn host_allreduce = nullptr;   // host-staged transport (esl_comm_init_host)
  void* host_user = nullptr;
  double* host_stage = nullptr;
  double* dev_gather = nullptr;  // 8 x n_ranks
  double* host_gather = nullptr; // pinned
  double* Linv_ws = nullptr;  // ceil(n/NB) x NB x NB
  double* z_ws = nullptr;
  int64_t S_lda = 0;
  // camera-first elimination (esl_cf.hpp; SLAM mode, cameras chained by the odometry edges): per-ellipsoid edge lists sorted by
  // camera slot, the odometry edges of every consecutive slot pair, the block-bidiagonal factor (Linv, M, N), per-edge V = Linv W,
  // X^T = (L^-1 [W | b_c])^T, the reduced ellipsoid system T (+ b row) and its solver workspaces.  Big buffers on first use.
  bool cf_chain_ok = false;
  bool cf_ready = false;         // every buffer of cf_ensure exists and is initialised (esl_slam.hip)
  bool cf_unavailable = false;   // ESL_SOLVER_AUTO: the camera-first buffers did not fit; this graph runs the reduced camera system
  // every decision and length of the layout, member by member in esl_cf_plan.hpp; below, the device arrays it is shipped into
  // (interior pointers of arena_solve, named after the plan's members and the kernels' arguments: esl_cf.hpp)
  esl::CfPlan cf_plan;
  int *cf_oe_start = nullptr, *cf_oe_u = nullptr, *cf_oe_slot = nullptr, *cf_od_start = nullptr, *cf_od_edge = nullptr, *cf_oe_cst = nullptr;
  double *cf_Linv = nullptr, *cf_M = nullptr, *cf_N = nullptr, *cf_V = nullptr, *cf_vy = nullptr, *cf_z = nullptr;
  double *cf_B = nullptr, *cf_Lfac = nullptr, *cf_G = nullptr;
  double *cf_Zt = nullptr, *cf_Hs = nullptr, *cf_Bs = nullptr, *cf_LfacS = nullptr, *cf_GS = nullptr, *cf_LiS = nullptr, *cf_MS = nullptr,
         *cf_NS = nullptr, *cf_R = nullptr;   // nested dissection: the separators' system
  double *cf_Xt = nullptr, *cf_T = nullptr, *cf_Linv_ws = nullptr, *cf_part = nullptr;
  // sparse interior rows of X: the column map cmap[p (N + 1) + o] = first << 24 | index (-1: column o of X is zero over segment p;
  // entry N = the right-hand side), per ellipsoid the bitmap of its segments, the compact slabs Xc and the separators' dense rows Xs
  int *cf_seg_start = nullptr, *cf_seg_obj = nullptr, *cf_seg_first = nullptr, *cf_cmap = nullptr, *cf_xld = nullptr, *cf_fwork = nullptr, *cf_twork = nullptr;
  unsigned long long* cf_mask = nullptr;
  long long *cf_xoff = nullptr, *cf_boff = nullptr, *cf_roff = nullptr;
  double *cf_Xc = nullptr, *cf_Xs = nullptr, *cf_P = nullptr, *cf_Prhs = nullptr, *cf_Y = nullptr, *cf_Yr = nullptr;
  // form 3 without the interior slab (esl_cf_sweep.hpp): the per-slot matrices of the backward direction and of the combination, the
  // last interior slot's rows of x per segment, the entry of every place of the per-camera lists
  double *cf_Pm = nullptr, *cf_Qm = nullptr, *cf_XL = nullptr;
  int* cf_sl_ent = nullptr;
  // the one-sided assembly's pair list (k_cf_os_list): per block of T's lower triangle and of the b row where its (A record, B record)
  // pairs start and how many there are
  long long* cf_os_start = nullptr;
  int *cf_os_cnt = nullptr, *cf_os_pairs = nullptr;
  // twins merged, shorter side (esl_cf.hpp k_cf_os_list; null with ESL_CF_OS_LIST=0): the plan's os_run and os_heads, and Vm -- at
  // every run's head the sum of the run's V records (k_cf_v_merge, every trial; the arena's and the hazards' rules of cf_V)
  int *cf_os_run = nullptr, *cf_os_heads = nullptr;
  double* cf_Vm = nullptr;
  int *cf_rank = nullptr, *cf_unrank = nullptr, *cf_kfirst = nullptr;
  double* cf_xo_t = nullptr;   // x_o as the solver returns it (T's order)
  int lm_solver_used = 0;   // esl_linear_solver the last trial step ran with (1 reduced camera system, 2 reduced ellipsoid system, 3 camera chain)
  // fixed ellipsoids (esl_graph_upload_fixed, esl_fixed.hpp).  fx_on: the resident graph was uploaded with at least one flag set;
  // everything below is empty / unused otherwise and no kernel of esl_fixed.hpp runs
  bool fx_on = false;
  std::vector<uint8_t> fx_flags;            // n_objs flags (0 / 1) of the resident graph
  esl::AnchGraph fx;                        // device arrays of the anchored + inactive edges (interior pointers of fx_blob)
  char* fx_blob = nullptr; size_t fx_blob_cap = 0;   // grow-only
  double* fx_A = nullptr; double* fx_chi = nullptr;  // per anchored edge: the 27-double camera record, chi2
  // caller order -> where the edge went: >= 0: index in the caller order of the free-ellipsoid graph (h_bb_slot_of ...), < 0: -(k + 1),
  // k = index in the arrays of fx
  std::vector<int> fx_bb_map, fx_e3_map;
  std::vector<int> fx_grav_obj;             // the caller's gravity edges (all of them; h_grav_obj holds those of free ellipsoids)
  bool chain_ok = false;                    // the odometry edges between free cameras join neighbours only (slam_alloc)
  esl::Scratch chain_ws;                    // ESL_SOLVER_CAMERA_CHAIN: D, L, rhs (two sets) + the blocks' inverses
  // ESL_SOLVER_PCG (esl_pcg.hpp).  pcg: esl_lm_set_pcg, read when a run starts (pcg_run); pcg_ws: state block, M, M^-1, b_s, r, z, p (two),
  // q, D^-1 b_o, the edges' products, the partials -- O(edges + cameras), grow-only, freed by slam_release; pcg_M: the diagonal blocks of S
  // of the last PCG trial (interior pointer, null when the last trial ran another solver); pcg_host: pinned, the done flag's landing place
  esl_pcg_params pcg = {1000, 8, 1e-10};
  esl_pcg_params pcg_run = {1000, 8, 1e-10};
  double* pcg_ws = nullptr; size_t pcg_ws_cap = 0;
  double* pcg_st = nullptr; double* pcg_M = nullptr;
  double* pcg_host = nullptr;
  bool pcg_ran = false;            // a PCG trial has run on this context (esl_lm_pcg_stats reports zeros before)
  bool pcg_reset = true;           // the per-run counters restart with the next PCG trial (esl_lm_begin)
  // per-context runtime of the dense solver (esl_chol.hpp CholRuntime: look-ahead stream + events on THIS device, one-time
  // kernel attributes of this device) and of the Schur kernel; created on first use, released with the context
  void* chol_rt = nullptr;
  void* chol_prof_scope = nullptr;   // the open ProfScope (class 9) around a dense factorisation (esl_slam.hip chol_prof_mark)
  unsigned long long graph_fp = 0;   // order-independent fingerprint of the uploaded graph's structure (esl_graph_upload / _append; comm_check_replicated)
  bool repl_checked = false;         // replicated-graph communicator: this graph's fingerprint has been compared across the ranks
  double *chol_pack = nullptr, *chol_pack2 = nullptr;   // staging buffers of the distributed factorisation's panel messages (esl_chol.hpp CholDist)
  size_t chol_pack_len = 0;
  bool schur_attr_set = false;
  // switches resolved ONCE when the communicator is created (every rank must take the same collective sequence for the whole
  // run; an environment read per trial could change mid-run): ESL_CHOL_DIST = 1 / 0 forces the distributed factorisation
  // on / off, unset = by size
  int sw_chol_dist = -1;
  bool sw_chol_overlap = true;   // the distributed factorisation's messages on their own stream under the trailing updates
  // ESL_CF_OVERLAP as read when the CONTEXT was created (A/B; a serial and an overlapped context can live in one process): the
  // side-stream orders of slam_try_step_cf (esl_slam.hip).  0: every launch of a camera-first trial in stream order; 1: both
  // side-stream orders; 2: the separators' chain beside the interior rows only; 3: the products' early start only; 4 (default):
  // as 1, and the rank-K update capped to one workgroup per CU so that the products' waves are resident beside it (1: uncapped, A/B)
  int sw_cf_overlap = 4;
  // ESL_CF_OS_KERNEL as read when the context was created (A/B and tests): 1 (default) the one-sided assembly feeds whole records
  // through LDS (k_cf_T_onesided_lds), 0 the per-lane gather (k_cf_T_onesided).  Same bits either way.
  int sw_cf_os_kernel = 1;
  // ESL_CF_OS_LIST as read when the context was created (A/B and tests): 1 (default) the assembly's list holds one pair per run of
  // twins and walks the shorter side per block and segment; 0 the row side over every entry, from cf_V (the bits of that list)
  int sw_cf_os_list = 1;
  // ESL_CF_FWD_PARTS as read when the context was created (A/B and tests): 8 (default), 4 or 2 parts per chunk of the slab sweep
  // k_cf_forward<2> (esl_cf.hpp) and of k_cf_sweep (esl_cf_sweep.hpp): less LDS per one-wave workgroup, more waves per CU.  Same bits at
  // every value.
  int sw_cf_fwd_parts = 8;
  // ESL_CF_SWEEP as read when the context was created (A/B and tests): 1 (default) form 3 builds Y in one two-directional sweep per
  // segment and never stores the interior slab (esl_cf_sweep.hpp); 0 the parent's k_cf_forward<2> + k_cf_seg_back + slab z, its bits
  int sw_cf_sweep = 1;
  // ESL_CF_STRIDE as read when the context was created: 16, 32 or 48 forces the segment length of the sparse form where T is
  // assembled one-sided (form 3); 0 (unset) = chosen at layout time from the graph's counts (esl_cf_plan.hpp, cf_stride_cost)
  int sw_cf_stride = 0;
};
