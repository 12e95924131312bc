/*
 * esl.h — C-ABI of the MI355X-native EllipsoidSLAM hot-path backend.
 *
 * Drop-in boundary (SURVEY.md §8 b).  The reference has no FFI; its boundary is the public
 * surface of three C++ classes that `Tracking` instantiates directly.  Each entry point
 * below names the reference member it replaces:
 *
 *   esl_optimize*        <- EllipsoidSLAM::Optimizer::GlobalObjectGraphOptimization
 *                           (reference include/core/Optimizer.h:20-23, src/core/Optimizer.cpp:83-317)
 *                           + g2o::SparseOptimizer::optimize / OptimizationAlgorithmLevenberg::solve
 *                           (Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:354-419,
 *                            core/optimization_algorithm_levenberg.cpp:61-164)
 *   esl_lm_*  (step API) <- the pieces of the above that exchange scalars between shards:
 *                           computeActiveErrors/activeRobustChi2 (sparse_optimizer.cpp:61-114),
 *                           BlockSolver::buildSystem/setLambda/solve (core/block_solver.hpp:354-604),
 *                           computeLambdaInit/computeScale (optimization_algorithm_levenberg.cpp:166-189)
 *   esl_fit_frame        <- EllipsoidSLAM::EllipsoidExtractor::EstimateLocalEllipsoid
 *                           (reference src/pca/EllipsoidExtractor.h:57-58, .cpp:292-493)
 *   esl_init_quadric     <- EllipsoidSLAM::Initializer::initializeQuadric
 *                           (reference include/core/Initializer.h:47-50, src/core/Initializer.cpp:24-56)
 *
 * Conventions (identical to the reference's own vectors):
 *   SE3 7-vector      = x y z qx qy qz qw        (g2o::SE3Quat::toVector, types/se3quat.h:144-155)
 *   ellipsoid 10-vec  = x y z qx qy qz qw a b c  (g2o::ellipsoid::toVector, src/core/Ellipsoid.cpp:152-157)
 *   camera states are Tcw (world -> camera), ellipsoid poses are object -> world.
 * All arrays are caller-allocated, plain pointers and sizes; no exceptions cross this boundary;
 * every function returns an esl_status.  A context is bound to one HIP device and one stream and
 * is re-entrant per context (not thread-safe within one context).
 *
 * There is NO CPU fallback behind these symbols: without a usable HIP device the compute entry
 * points return ESL_ERR_NO_DEVICE.
 */
#ifndef ESL_H_
#define ESL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESL_ABI_VERSION 5   /* 2: esl_lm_params::bbox_residual, esl_fit_frame_ex, esl_init_from_qstar / esl_init_plane_error, esl_graph_append
                             * 3: esl_linear_solver gains ESL_SOLVER_REDUCED_CAMERA / ESL_SOLVER_REDUCED_ELLIPSOID, esl_lm_solver_used,
                             *    esl_lm_solver_stats, esl_comm_set_replicated, ESL_PROF_KINDS 9
                             * 4: ESL_PROF_KINDS 10 (class 9: the dense factorisation alone), esl_ctx_trim, esl_comm_set_replicated refuses a
                             *    mode change under a resident graph, esl_graph_append accepts SLAM-mode graphs (free cameras + odometry)
                             * 5: esl_lm_params::e3d_half_turn (1 = the yaw-hypothesis minimum exactly as Ellipsoid.cpp:92-117 writes it),
                             *    esl_plane_params::max_curvature (PCL's maximum_curvature_ model test; min_inliers is a strict >);
                             *    additive part of 5: robust kernels per edge class (esl_robust_params, esl_lm_set_robust, esl_edge_chi2) --
                             *    detect them by the symbol; likewise fixed ellipsoids (esl_graph_upload_fixed, esl_optimize_fixed,
                             *    esl_graph_obj_fixed) with ESL_SOLVER_CAMERA_CHAIN, and relocalisation against a fixed map
                             *    (esl_reloc_set_map, esl_relocalize), and 2-D data association against the projected map
                             *    (esl_predict_boxes, esl_associate_boxes), and the SVD initialisation of many ellipsoids in one call
                             *    (esl_init_quadrics) and its outlier-rejecting form (esl_init_quadrics_robust), and map maintenance
                             *    (esl_map_overlaps, esl_map_merge), and the per-pixel rendering of a map (esl_render_map), and the voxel-fused
                             *    dense map of many RGB-D frames (esl_dense_begin / _add_frames / _info_get / _extract / _end) with its
                             *    per-instance ellipsoids (esl_dense_objects) and its dominant planes and ground (esl_dense_planes), and
                             *    its exact de-integration (esl_dense_remove_frames / _move_frames / _purge / _slots_get), and its
                             *    view from any pose, checked against measured depth (esl_dense_render), and its per-voxel normals
                             *    (esl_dense_normals) and the poses refined against it (esl_dense_align_frames), and the carving of the
                             *    voxels that later frames see through (esl_dense_carve_frames), and the covisibility of the frames
                             *    through it with their redundancy (esl_dense_covis_frames) */
#define ESL_MAX_TRACE 32

typedef enum {
  ESL_OK = 0,
  ESL_ERR_NO_DEVICE = 1,   /* no HIP device / HIP runtime error on create */
  ESL_ERR_INVALID = 2,     /* bad argument (null pointer, negative size, index out of range) */
  ESL_ERR_HIP = 3,         /* HIP runtime call failed; see esl_last_error() */
  ESL_ERR_STATE = 4,       /* call sequence error (e.g. step API before esl_lm_begin) */
  ESL_ERR_ALLOC = 5
} esl_status;

typedef struct esl_ctx esl_ctx;

/* ---- graph description (SoA, host pointers) ------------------------------------------------
 * Mirrors what Optimizer.cpp:127-279 assembles into g2o objects. */
typedef struct {
  double fx, fy, cx, cy;          /* Kalib (EdgeSE3EllipsoidProj::setKalib, BasicEllipsoidEdges.cpp:114) */
  int32_t n_cams;                 /* VertexSE3Expmap count  (Optimizer.cpp:127-139) */
  int32_t n_objs;                 /* VertexEllipsoid count  (Optimizer.cpp:175-180) */
  const uint8_t* cam_fixed;       /* n_cams flags; NULL = all fixed (mapping mode, Optimizer.cpp:126,135) */

  /* EdgeSE3EllipsoidProj (Optimizer.cpp:201-245): information = weight * I4 */
  int32_t n_bbox;
  const int32_t* bbox_cam;
  const int32_t* bbox_obj;
  const double* bbox_meas;        /* n_bbox x 4 : x1 y1 x2 y2; entries < 5 are ignored (BasicEllipsoidEdges.cpp:109) */
  const double* bbox_weight;      /* n_bbox     : Observation::rate */

  /* EdgeSE3Ellipsoid9DOF (Optimizer.cpp:249-279): information = weight * I9
   * (the caller passes weight = Optimizer.Edges.3DEllipsoid.Scale * prob) */
  int32_t n_e3d;
  const int32_t* e3d_cam;
  const int32_t* e3d_obj;
  const double* e3d_meas;         /* n_e3d x 10 : local (camera-frame) ellipsoid */
  const double* e3d_weight;       /* n_e3d */

  /* EdgeEllipsoidGravityPlanePrior (Optimizer.cpp:183-196): information = grav_weight
   * (the caller passes GravityPrior.Scale^2) */
  int32_t n_grav;
  const int32_t* grav_obj;
  double grav_normal[4];          /* ground plane param; only [0..2] enter the residual */
  double grav_weight;

  /* EdgeSE3Expmap odometry (Optimizer.cpp:142-158; SLAM mode only): information = diag(odom_info) */
  int32_t n_odom;
  const int32_t* odom_i;          /* vertex 0 */
  const int32_t* odom_j;          /* vertex 1 */
  const double* odom_meas;        /* n_odom x 7 */
  const double* odom_info;        /* n_odom x 6 ; NULL = identity */

  /* the optional visibility test of the bbox edges (checkVisibility, Optimizer.cpp:35-81; argument check_visibility of
   * GlobalObjectGraphOptimization, false at the reference's only call site): an edge also needs the ellipsoid in front of its
   * camera, the camera outside the ellipsoid and the projected centre or a corner of the projected box inside the image.
   * Evaluated once at the start state together with the NaN test; failing edges count as dropped. */
  int32_t check_visibility;       /* 0 = off (as shipped) */
  int32_t image_rows, image_cols; /* Optimizer.h:20-23 rows, cols; only read when check_visibility != 0 */
} esl_graph;

typedef enum {
  ESL_JAC_NUMERIC = 0,   /* central differences, delta = numeric_delta (g2o base_binary_edge.hpp:147-197) */
  ESL_JAC_ANALYTIC = 1   /* closed-form Jacobians of the same residuals */
} esl_jacobian_mode;

typedef enum {
  /* All cameras fixed (mapping mode, the shipped setting): 9x9 blocks per ellipsoid.  Free cameras (SLAM mode): one of the two
   * block eliminations below -- both solve EXACTLY the system g2o's LinearSolverDense solves with one pivoted LDLT of the whole
   * free system (solvers/linear_solver_dense.h:65-113; that literal form exists only in the CPU checker, oracle/ ORACLE_DENSE,
   * which the tests compare against); which block is eliminated first is what BlockSolver's setMarginalized decides
   * (core/block_solver.hpp:367-486).  AUTO takes the one with fewer flops that applies. */
  ESL_SOLVER_AUTO = 0,
  /* Schur complement onto the CAMERAS: S = Hcc - sum_o W_o (Hoo + lambda I)^-1 W_o^T, dense FP64-MFMA Cholesky of order
   * 6 (F - 1) -- the reduced camera system of BASELINE.json's north star.  Always applicable; the form sharded runs use. */
  ESL_SOLVER_REDUCED_CAMERA = 1,
  /* Cameras first (round 3): in the reference's SLAM branch the camera block is block TRIDIAGONAL (odometry edges join
   * consecutive frames only, Optimizer.cpp:142-158), so it has a block-bidiagonal Cholesky factor L; the reduced system
   * T = (Hoo + lambda I) - (L^-1 W)^T (L^-1 W) over the ELLIPSOIDS (order 9 N) is formed with an FP64-MFMA rank-6(F-1) update and
   * factored densely.  (9N)^2 6F + (9N)^3/3 flops instead of (6F)^3/3 (C4: 2.1e13 vs 7.2e13); for long chains the camera chain is
   * dissected into 16-camera segments and X = L^-1 W kept sparse (per-segment MFMA products, the dense update only for the
   * separator cameras' rows: C4 3.3e12 flops; esl_lm_solver_stats reports the shape).  Needs every odometry edge to join two free
   * cameras that are neighbours in free-camera order, and either one GPU or the replicated-graph communicator
   * (esl_comm_set_replicated); ESL_ERR_INVALID otherwise. */
  ESL_SOLVER_REDUCED_ELLIPSOID = 2,
  /* The camera chain alone (additive part of ABI 5, with esl_graph_upload_fixed): no active edge joins a free camera to a free
   * ellipsoid (W is structurally empty -- localisation against a fixed map), and the odometry edges satisfy the chain condition
   * ESL_SOLVER_REDUCED_ELLIPSOID already requires.  (Hcc + lambda I + odometry blocks) x_c = b_c is then block tridiagonal (block
   * diagonal without odometry) and is solved as such, by cyclic reduction over 6 x 6 blocks -- no dense matrix is formed; free
   * ellipsoids, which can then only hang on fixed cameras, keep their 9 x 9 solves.  ESL_ERR_INVALID when requested on a graph that
   * does not qualify or on a context with a communicator.  ESL_SOLVER_AUTO picks it when it applies AND the graph was uploaded
   * with at least one obj_fixed flag set; requested explicitly it runs on any qualifying graph. */
  ESL_SOLVER_CAMERA_CHAIN = 3,
  /* Matrix-free preconditioned conjugate gradient on the reduced camera system (additive part of ABI 5, with esl_lm_set_pcg: detect
   * by the symbol; g2o's LinearSolverPCG, solvers/pcg/linear_solver_pcg.hpp, on the Schur complement).  S x_c = b_s is solved from
   * x_0 = 0 with the 6 x 6 diagonal blocks of S as the preconditioner and S never formed: one iteration is two passes over the
   * per-edge W blocks of the linearisation, so a trial costs O(edges) time and memory -- no dense matrix, any odometry topology
   * (loop closures included), robust kernels and fixed ellipsoids as in the other forms.  The iteration stops at the first k with
   * |r_k| <= rel_tol |b_s| (esl_pcg_params); a non-positive pivot in a preconditioner block or in an ellipsoid block, or no
   * convergence within max_iters, is reported exactly as a non-positive pivot of the dense factorisation is (solve_ok = 0: the LM
   * rejects the trial and raises lambda -- g2o's reaction to a failed _solver->solve).  Bit-reproducible from run to run.
   * ESL_SOLVER_AUTO never picks it.  One GPU: ESL_ERR_INVALID on a context with a communicator. */
  ESL_SOLVER_PCG = 4
} esl_linear_solver;

typedef enum {
  ESL_BBOX_REPROJECTION = 0,  /* r = bbox(Q*, P) - z, the reference's EdgeSE3EllipsoidProj (BasicEllipsoidEdges.cpp:90-112) */
  ESL_BBOX_TANGENCY = 1       /* OPTIONAL EXTRA, off for parity: r_k = pi_k^T Q* pi_k for the four planes pi_k = P^T l_k through the
                               * camera centre and the bbox lines (unit normals): the tangency constraint the reference only uses in
                               * its SVD initialiser (Initializer.cpp:147-164, 271-284) as an edge; same weight, same < 5 px rule */
} esl_bbox_residual;

typedef struct {
  int32_t max_iters;        /* 10  (Optimizer.cpp:291) */
  int32_t max_trials;       /* 10  (optimization_algorithm_levenberg.cpp:49) */
  double tau;               /* 1e-5 (optimization_algorithm_levenberg.cpp:45) */
  int32_t jacobian_mode;    /* esl_jacobian_mode */
  double numeric_delta;     /* 1e-9 */
  int32_t linear_solver;    /* esl_linear_solver (SLAM mode only; ignored when all cameras are fixed) */
  int32_t drop_nan_bbox;    /* 1: pre-evaluate bbox edges and drop those with NaN chi2 (Optimizer.cpp:234-243) */
  int32_t bbox_residual;    /* esl_bbox_residual; 0 = the reference */
  int32_t e3d_half_turn;    /* 3-D edge, choice among the four yaw hypotheses (Ellipsoid.cpp:92-117).  0 (default): a hypothesis whose relative
                             * rotation is within ~1.4e-6 rad of a HALF TURN is not eligible -- the reference's log has no branch for theta -> pi
                             * (se3quat.h:229-266: 0/0, decided by the last bit of the trace), its true norm is pi and never the minimum.
                             * 1: the minimum exactly as the reference writes it (minCoeff over the four norms, half turns included): bit-level
                             * faithful where the log is well defined, implementation-defined where the reference itself is (ABI 5) */
} esl_lm_params;

typedef struct {
  int32_t iterations;       /* outer iterations run (SparseOptimizer::optimize return value) */
  int32_t total_trials;     /* sum of inner LM trials */
  int32_t n_bbox_valid;
  int32_t n_bbox_dropped;
  int32_t stop_reason;      /* 0 max_iters, 1 Terminate(trials==max or rho==0), 2 Terminate(nBad>=3), 3 nothing to optimise */
  double chi2_initial;
  double chi2_final;
  double lambda_final;
  int32_t trace_len;
  double trace_chi2[ESL_MAX_TRACE];     /* chi2 after each outer iteration */
  double trace_lambda[ESL_MAX_TRACE];   /* lambda after each outer iteration */
  int32_t trace_trials[ESL_MAX_TRACE];  /* inner trials of each outer iteration */
} esl_lm_report;

/* Partial sums one shard contributes; summed (chi2, scale) or max-ed (max_diag) across shards. */
typedef struct {
  double chi2;
  double max_diag;
  double scale;      /* sum_j x_j (lambda x_j + b_j) */
  int32_t solve_ok;  /* 1 if every local factorisation had positive pivots (AND across shards) */
  int32_t pad;
} esl_lm_partials;

/* ---- context ---------------------------------------------------------------------------------*/
int esl_abi_version(void);
const char* esl_last_error(void);
int esl_device_count(void);
int esl_ctx_create(int device_id, esl_ctx** out);
int esl_ctx_destroy(esl_ctx* ctx);
int esl_ctx_synchronize(esl_ctx* ctx);
/* The context keeps its device buffers in grow-only blobs from graph to graph (no hipMalloc per esl_optimize: Optimizer.cpp:127,166,250
 * rebuilds its whole graph every frame).  esl_ctx_trim releases the SLAM-mode SOLVER blobs (camera-first set / reduced camera
 * system: tens of GB at 10k cameras) -- and the SLAM list blob when the resident graph has no free cameras; whatever a later
 * trial step needs is built again.  Uploading a graph WITHOUT free cameras over a SLAM-mode one trims by itself. */
int esl_ctx_trim(esl_ctx* ctx);
void esl_lm_params_default(esl_lm_params* p);

/* ---- robust kernels (g2o core/robust_kernel_impl.cpp; Optimizer.cpp:224 e->setRobustKernel) ---------------------------
 * Per edge CLASS: an edge with raw chi2 e = r^T Omega r contributes rho1(e) J^T Omega J to H, -rho1(e) J^T Omega r to b
 * (g2o's robustInformation; the rho2 term is left out, as in g2o) and rho0(e) to the chi2 the LM uses everywhere (initial,
 * trial, rho ratio, stop rule, trace, report); lambda_0 = tau * max diag of the weighted H.  Kernels, with e <= delta^2 the
 * inlier test: Huber, PseudoHuber, Cauchy, Tukey exactly as g2o writes them.  The bbox class includes the plane-tangency
 * residual; the gravity prior stays merged per ellipsoid (count * rho(grav_weight r^2)).  The NaN pre-check and the
 * visibility test keep deciding on the RAW chi2 (Optimizer.cpp:234-243). */
typedef enum { ESL_ROBUST_NONE = 0, ESL_ROBUST_HUBER = 1, ESL_ROBUST_PSEUDO_HUBER = 2, ESL_ROBUST_CAUCHY = 3, ESL_ROBUST_TUKEY = 4 } esl_robust_kind;
typedef enum { ESL_EDGE_BBOX = 0, ESL_EDGE_E3D = 1, ESL_EDGE_GRAVITY = 2, ESL_EDGE_ODOM = 3, ESL_EDGE_CLASSES = 4 } esl_edge_class;
typedef struct {
  int32_t kind[ESL_EDGE_CLASSES];    /* esl_robust_kind per esl_edge_class */
  double delta[ESL_EDGE_CLASSES];    /* kernel width; must be finite and > 0 where kind != ESL_ROBUST_NONE */
} esl_robust_params;                 /* 48 bytes */
/* The setting belongs to the context: it survives esl_graph_upload, esl_graph_append and esl_ctx_trim, and every run reads it at
 * its start (esl_optimize, esl_optimize_resident, esl_lm_begin).  p = NULL: every class ESL_ROBUST_NONE (the default).
 * ESL_ERR_INVALID for a kind out of range or a bad delta.  Sharded runs: every rank must set the same values. */
int esl_lm_set_robust(esl_ctx* ctx, const esl_robust_params* p);
/* ---- ESL_SOLVER_PCG (additive part of ABI 5) -------------------------------------------------------------------------
 * The setting belongs to the context exactly like esl_lm_set_robust: it survives esl_graph_upload, esl_graph_append and
 * esl_ctx_trim and is read when a run starts (esl_optimize, esl_optimize_resident, esl_lm_begin).  p = NULL restores the defaults.
 * ESL_ERR_INVALID for max_iters < 1, check_every < 1, or a rel_tol that is not finite or <= 0. */
typedef struct {
  int32_t max_iters;     /* 1000: iterations after which the solve counts as failed */
  int32_t check_every;   /* 8: the host looks at the device's done flag once per this many iterations (the iterations, alpha, beta
                          * and the stop test run on the device; launches behind a finished solve do nothing, so x_c, the iteration
                          * count and the residual do not depend on this value) */
  double rel_tol;        /* 1e-10: stop at |r_k|_2 <= rel_tol |b_s|_2 */
} esl_pcg_params;        /* 16 bytes */
void esl_pcg_params_default(esl_pcg_params* p);
int esl_lm_set_pcg(esl_ctx* ctx, const esl_pcg_params* p);
/* stats[0] iterations of the last PCG solve, [1] |r|_2 / |b_s|_2 at its exit (from the recurrence), [2] converged (0 / 1),
 * [3] PCG solves since esl_lm_begin / the start of the optimize call, [4] iterations summed over those solves, [5] max_iters and
 * [6] rel_tol in force, [7] 0.  All zeros before any PCG trial of this context. */
#define ESL_PCG_STATS 8
int esl_lm_pcg_stats(esl_ctx* ctx, double stats[ESL_PCG_STATS]);

/* Every edge of one class at the states the context holds (e.g. after an optimize call): chi2[i] = raw chi2 e, weight[i] = rho1(e)
 * as the solver applies it, in CALLER order (upload order, then append order).  Bbox edges dropped by the NaN pre-check or the
 * visibility test report weight 0; a class without a kernel reports weight 1.  Gravity edges report the value of their
 * ellipsoid's prior.  count must equal the class's edge count (ESL_ERR_INVALID otherwise); either array may be NULL. */
int esl_edge_chi2(esl_ctx* ctx, int32_t edge_class, double* chi2, double* weight, int64_t count);

/* ---- one-shot optimiser (host buffers in, host buffers out) ------------------------------------*/
int esl_optimize(esl_ctx* ctx, const esl_graph* g, double* cams_io /* n_cams x 7 */,
                 double* objs_io /* n_objs x 10 */, const esl_lm_params* p, esl_lm_report* out);

/* ---- resident / step API (graph + states stay in HBM; used by bench and by the sharded driver) --*/
int esl_graph_upload(esl_ctx* ctx, const esl_graph* g);
/* ---- fixed ellipsoids (g2o's setFixed on a VertexEllipsoid, Optimizer.cpp:178; additive part of ABI 5: detect by the symbol) -----
 * esl_graph_upload with per-ellipsoid flags (n_objs bytes, any non-zero value = fixed; NULL or all zeros = esl_graph_upload).  With
 * obj_fixed[o] set: (1) the state of ellipsoid o never changes -- esl_states_download returns it bit for bit as uploaded; (2) an
 * edge all of whose vertices are fixed is INACTIVE (sparse_optimizer.cpp allVerticesFixed): a bbox or 3-D edge between o and a fixed
 * camera and every gravity prior on o are not linearised and are part of no chi2, of lambda_0 and of n_bbox_valid / n_bbox_dropped
 * (which count the active bbox edges); with all cameras fixed o drops out entirely, and a run without any active edge ends with
 * stop_reason 3; (3) an edge between o and a FREE camera is active and camera-only: its chi2 counts (through the robust kernel of
 * its class), its Jacobian is taken wrt the camera alone (numeric or analytic per jacobian_mode), it adds Jc^T Omega Jc to H_cc and
 * -Jc^T Omega r to b_c; the NaN pre-check and the visibility test apply to it.  Everything else is untouched.
 * All ellipsoids fixed + free cameras = pose-only optimisation against a finished map (localisation); see ESL_SOLVER_CAMERA_CHAIN.
 * A plain esl_graph_upload clears the flags; they survive esl_states_upload, snapshot / restore and esl_ctx_trim.  The step API and
 * esl_lm_download work on a flagged graph (H_oo, b_o, x_o of a fixed ellipsoid read as zeros, H_cc / b_c include the camera-only
 * edges); esl_lm_download(which = 9) returns ESL_ERR_STATE on a flagged graph.  esl_edge_chi2 keeps reporting EVERY edge of the
 * caller's graph in caller order: camera-only edges with their raw chi2 and rho1, inactive edges with their raw chi2 at the resident
 * states and weight 0.  ESL_ERR_STATE: esl_graph_append on a graph with a flag set; a flag set on a context with a communicator. */
int esl_graph_upload_fixed(esl_ctx* ctx, const esl_graph* g, const uint8_t* obj_fixed);
/* one-shot: esl_optimize with the flags */
int esl_optimize_fixed(esl_ctx* ctx, const esl_graph* g, const uint8_t* obj_fixed, double* cams_io, double* objs_io,
                       const esl_lm_params* p, esl_lm_report* out);
/* the flags of the resident graph (count = n_objs bytes out, 0 / 1; all zero after a plain esl_graph_upload) */
int esl_graph_obj_fixed(esl_ctx* ctx, uint8_t* flags_out, int32_t count);
int esl_states_upload(esl_ctx* ctx, const double* cams, const double* objs);
int esl_states_download(esl_ctx* ctx, double* cams, double* objs);
int esl_optimize_resident(esl_ctx* ctx, const esl_lm_params* p, esl_lm_report* out);
/* device-side copy of the current states (snapshot) and back (restore): lets a caller re-run the
 * optimiser from the same initial estimate without touching PCIe (the reference re-optimises the
 * whole graph every frame, Optimizer.cpp:127,166,250). */
int esl_states_snapshot(esl_ctx* ctx);
int esl_states_restore(esl_ctx* ctx);

/* ---- streaming: extend the device-resident graph instead of rebuilding it (BASELINE configs[4]) --------------------------
 * The reference rebuilds every g2o vertex and edge for every frame (Optimizer.cpp:127, 166, 250).  esl_graph_append adds the
 * observations of a new frame to the graph that is already in HBM: new cameras get the indices n_cams.., new ellipsoids
 * n_objs.. (their states are given; the states of the existing vertices -- e.g. the ellipsoids the previous frame's run
 * optimised -- stay where they are), edge indices refer to the extended numbering.  The result is indistinguishable from
 * esl_graph_upload of the concatenated graph (edges of an ellipsoid keep their arrival order).  Edges are stored sorted by
 * ellipsoid with slack behind every ellipsoid's slice: an append writes the new edges into free slots (one staged copy + two
 * small launches, independent of the size of the graph) and re-lays the arrays out, with doubled slack, only when a slice or an
 * array is full.
 * SLAM mode (ABI 4; the reference's bSLAM_mode branch, Optimizer.cpp:126-158): a delta may bring FREE cameras (new_cam_fixed) and
 * odometry edges; the edge records and the states still go into the resident arrays in place, the camera-side index tables
 * (camera slots, per-camera edge lists, the odometry arrays: a few bytes per edge) are rebuilt from the host's mirror of the layout
 * and shipped as one blob, and the solver's lists follow on the next trial step -- no re-upload, no re-sort of the graph.  One GPU
 * (no communicator). */
typedef struct {
  int32_t n_new_cams; const double* new_cams;   /* n_new_cams x 7 (Tcw) */
  int32_t n_new_objs; const double* new_objs;   /* n_new_objs x 10 */
  int32_t n_bbox; const int32_t* bbox_cam; const int32_t* bbox_obj; const double* bbox_meas; const double* bbox_weight;
  int32_t n_e3d; const int32_t* e3d_cam; const int32_t* e3d_obj; const double* e3d_meas; const double* e3d_weight;
  int32_t n_grav; const int32_t* grav_obj;      /* gravity priors on (new or old) ellipsoids */
  /* ABI 4 -- SLAM mode, all optional (a zero-initialised tail = the mapping-mode delta of ABI 2/3): */
  const uint8_t* new_cam_fixed;                 /* n_new_cams flags; null: the new cameras are fixed */
  int32_t n_odom; const int32_t* odom_i; const int32_t* odom_j;   /* odometry edges (previous frame, current frame), extended numbering */
  const double* odom_meas;                      /* n_odom x 7: Z = Tcw_j * Tcw_i^-1 */
  const double* odom_info;                      /* n_odom x 6 diagonal information, or null = ones */
} esl_graph_delta;
int esl_graph_append(esl_ctx* ctx, const esl_graph_delta* d);
/* sizes of the resident graph (after uploads / appends) */
int esl_graph_sizes(esl_ctx* ctx, int32_t* n_cams, int32_t* n_objs, int32_t* n_bbox, int32_t* n_e3d, int32_t* relayouts);

/* per-kernel timing with HIP events recorded on the context's own stream.
 * kernel ids: 0 linearise, 1 LM trial (solve + retract + chi2), 2 reduced-system build (Schur complement / camera-first: factor of
 *             the camera block + X + the rank-K update), 3 dense Cholesky + solves, 4 reductions / misc, 5 single-frame fit,
 *             6 RCCL all-reduce of the reduced system (sharded SLAM), 7 the MFMA rank-K update T -= X^T X of the camera-first
 *             form alone (nested inside class 2), 8 the block products of the sparse interior rows of X (k_cf_T_sparse, nested
 *             inside class 2; with class 8 present class 7 is the dense update with the separators' rows only), 9 the dense
 *             FACTORISATION of the reduced system alone (nested inside class 3: one k_chol_persist launch from 4,096 unknowns on,
 *             the launch-per-step chain otherwise; class 3 minus class 9 = back-substitutions).
 * esl_profile_enable(ctx, 0) off; 1 = bracket only kernel class 0, and inside esl_optimize_resident's device-driven
 * mapping run only ONE linearisation launch per run (cheap enough to stay on inside a timed region: an event record
 * is a barrier packet between two otherwise back-to-back dispatches); 2 = bracket every launch of every class.
 * esl_profile_get drains the events: count[k] launches, total_ms[k] summed durations. */
#define ESL_PROF_KINDS 10
int esl_profile_enable(esl_ctx* ctx, int enable);
int esl_profile_get(esl_ctx* ctx, int64_t count[ESL_PROF_KINDS], double total_ms[ESL_PROF_KINDS]);

int esl_lm_begin(esl_ctx* ctx, const esl_lm_params* p, int32_t* n_valid, int32_t* n_dropped);
/* residuals at current states -> chi2 ; then H,b -> max_diag */
int esl_lm_linearize(esl_ctx* ctx, esl_lm_partials* out);
/* SLAM mode only: build this shard's reduced camera system for `lambda` and return its device pointer.
 * Layout: (n+1) x n doubles, column-major with leading dimension lda; rows 0..n-1 hold the LOWER
 * triangle of S = Hcc + lambda I - sum_o W_o (Hoo + lambda I)^-1 W_o^T, row n holds b_s^T.
 * A multi-GPU caller may sum the lda*n doubles across shards in place (SURVEY.md §8 e). */
int esl_lm_reduced_system(esl_ctx* ctx, double lambda, void** dev_ptr, int64_t* n, int64_t* lda);
/* SLAM mode diagnostic (tests at sizes no CPU checker reaches): re-builds the reduced camera system for the lambda of
 * the last esl_lm_try_step (the factorisation overwrote it) and returns |S x_c - b_s| / |b_s| for the x_c that step solved. */
int esl_lm_reduced_residual(esl_ctx* ctx, double* rel_residual_out);
/* backup states, solve (H + lambda I) x = b, apply x, recompute chi2; states stay updated */
int esl_lm_try_step(esl_ctx* ctx, double lambda, esl_lm_partials* out);
/* accept != 0: discard backup; accept == 0: restore states from backup */
int esl_lm_commit(esl_ctx* ctx, int accept);
/* which esl_linear_solver the last SLAM-mode trial step of this context ran with (ESL_SOLVER_REDUCED_CAMERA,
 * ESL_SOLVER_REDUCED_ELLIPSOID or ESL_SOLVER_CAMERA_CHAIN: what ESL_SOLVER_AUTO resolved to; ESL_SOLVER_PCG when it was requested);
 * 0 before any SLAM-mode step */
int esl_lm_solver_used(esl_ctx* ctx, int32_t* solver_out);
/* shape of the camera-first elimination of the resident graph as the last trial step ran it (zeros when it did not):
 * stats[0] form of X: 0 dense rows, 1 sparse with stored per-segment products, 2 sparse, blocks of T straight from the slabs,
 *     3 sparse, T's interior part assembled one-sided from the V records and the back-swept slabs Y (no product store; the form a
 *     single rank runs when ESL_CF_SPARSE is unset);
 * [1] dissection stride (0: plain chain), [2] separators, [3] segments, [4] flops of the per-segment products (lower block triangles, rows from a block row's first camera on;
 *     form 3: of the assembly's 9 x 6 . 6 x 9 record products),
 * [5] bytes of the stored products (form 3: of Y), [6] bytes of the compact slabs, [7] rows of the dense MFMA update (K, padded),
 * [8] flops that update executes when T's ellipsoids are ordered by first camera and the structurally zero rows above the
 *     staircase are skipped tile by tile (0: the closed form n (n + 1) K applies), [9] 1 if T is in that order. */
#define ESL_SOLVER_STATS 10
int esl_lm_solver_stats(esl_ctx* ctx, double stats[ESL_SOLVER_STATS]);
/* the pair list of the one-sided assembly (form 3) of the resident graph as the last trial step ran it (zeros otherwise), in record
 * pairs, the b row included: counts[0] the row side over every list entry (what stats[4] prices), [1] with a camera's bounding-box
 * and 3-D edge to one ellipsoid merged into one pair, [2] merged and, per block and shared segment, the side with fewer pairs;
 * [3] the length of the list that was built ([2], or [0] with ESL_CF_OS_LIST=0 when the context was created), [4] the flops of its
 * 9 x 6 . 6 x 9 products, [5] its bytes. */
#define ESL_OS_COUNTS 6
int esl_lm_os_counts(esl_ctx* ctx, double counts[ESL_OS_COUNTS]);

/* inspection (tests, debugging): copy one device array of the current linearisation to the host.
 * which: 0 Hoo (n_objs x 45 packed upper 9x9), 1 bo (n_objs x 9), 2 xo (n_objs x 9, last trial),
 *        3 Hcc (n_free_cams x 36), 4 bc (n_free_cams x 6), 5 xc (n_free_cams x 6, last trial),
 *        6 reduced system ((n+1) x n column-major, lda = round_up(n+1,16): lda*n doubles), 7 trial ellipsoids (n_objs x 10),
 *        8 trial cameras (n_cams x 7), 9 (SLAM mode) the per-edge camera-ellipsoid blocks W = Jc^T Omega Jo as [54][n_bbox + n_e3d]:
 *        entry (a, b) of edge u at [(a * 9 + b) * (n_bbox + n_e3d) + u], u = position of the edge after the stable sort by
 *        ellipsoid (bbox edges first, 3-D edges from n_bbox on); zero for edges of fixed cameras.
 *        10 the 6 x 6 diagonal blocks of S (n_free_cams x 36, row-major) exactly as the preconditioner of the last ESL_SOLVER_PCG
 *        trial used them, before inversion; ESL_ERR_STATE when the last trial ran another solver.
 *        An ellipsoid that takes no step -- fixed, or without any edge and gravity prior -- reads as zeros in 2 and as its state in 7.
 *        count = number of doubles the caller's buffer holds. */
int esl_lm_download(esl_ctx* ctx, int32_t which, double* dst, int64_t count);

/* ---- multi-GPU exchange inside the library (RCCL over xGMI) ---------------------------------------------------
 * One process per GPU.  Rank 0 creates an id (esl_comm_unique_id), the host language ships its 128 bytes to the
 * other ranks (torch.distributed / MPI / a file), every rank calls esl_comm_init.  Afterwards
 * esl_optimize_resident is COLLECTIVE: each rank optimises its own shard (its ellipsoids with all their edges,
 * cameras replicated) under g2o's single global LM control — the LM scalars of every linearisation / trial are
 * exchanged with one ncclAllGather on the context's stream and reduced in rank order on every rank, so all ranks
 * take bit-identical accept/reject decisions (SURVEY.md §8 e).  RCCL is dlopen()ed at esl_comm_init time.
 * SLAM mode (free cameras): the shards additionally ncclAllReduce(sum) the camera blocks Hcc, b_c once per
 * linearisation and the partial reduced camera system S (+ b_s row) once per trial; odometry edges, lambda I on
 * the camera blocks and the camera part of the LM scale are counted on rank 0 only, so the summed system equals
 * the single-GPU one up to summation order.  Every rank then factorises the same S (replicated Cholesky: it is
 * O(n^3) but 0.2-3 s at the C4 size, while the sharded part is the O(edges) linearise + Schur build). */
int esl_comm_unique_id(char out[128]);
int esl_comm_init(esl_ctx* ctx, int32_t n_ranks, int32_t rank, const char id[128]);
/* Same collective semantics over a transport the HOST supplies (MPI, gloo, a test harness): `fn` must sum
 * `count` doubles of `host_buf` in place over all ranks and return 0; every rank calls it in the same order with
 * the same count.  The library stages device buffers through pinned host memory in <= 64 MiB pieces.  Meant for
 * hosts without a GPU-aware transport and for tests; RCCL (esl_comm_init) is the fast path. */
typedef int (*esl_host_allreduce_fn)(void* user, double* host_buf, int64_t count);
int esl_comm_init_host(esl_ctx* ctx, int32_t n_ranks, int32_t rank, esl_host_allreduce_fn fn, void* user);
/* REPLICATED-GRAPH mode of a communicator (round 3; call after esl_comm_init / esl_comm_init_host, on every rank): every rank has
 * uploaded the WHOLE graph (the same esl_graph_upload everywhere: 15 MB at BASELINE configs[3]) instead of a shard of the
 * ellipsoids.  Nothing is summed over ranks then (every rank linearises everything -- 0.4 ms at configs[3] -- and takes the same LM
 * decisions by construction); the ranks divide the DENSE SOLVE of SLAM mode: the outer panels (512 columns) of the reduced system
 * are dealt cyclically, a rank forms only its own panels (camera-first elimination: its share of the rank-6(F-1) MFMA update;
 * reduced camera system: built everywhere, factored distributed), the owner factors a panel and ncclBroadcasts it, every rank
 * updates its own later panels (the broadcasts run on their own stream under those updates; ESL_CHOL_DIST_OVERLAP=0 puts them
 * back on the compute stream), the back-substitution runs replicated -- all ranks end with bit-identical states.  This is the
 * multi-GPU form of ESL_SOLVER_REDUCED_ELLIPSOID (the sharded form below sums shard contributions and uses the reduced camera
 * system).  Mapping-mode runs on such a communicator are simply replicated.
 * CONTRACT: the library cannot tell a shard from a whole graph -- the caller asserts that the graph resident on EVERY rank is the
 * same whole graph (switching the mode on over ellipsoid shards would leave every rank with its own partial sums, silently). */
int esl_comm_set_replicated(esl_ctx* ctx, int replicated);
int esl_comm_destroy(esl_ctx* ctx);

/* host-only helper: balanced partition of ellipsoids (with all their edges) over n_parts shards.
 * part_of_obj receives n_objs entries.  (SURVEY.md §8 e) */
int esl_partition_objects(const esl_graph* g, int32_t n_parts, int32_t* part_of_obj);

/* ---- single-frame fit -----------------------------------------------------------------------*/
typedef struct {
  int32_t stride;               /* 3  (PointCloudFilter.cpp:31-32) */
  double depth_scale;           /* 5000 (TUM3.yaml Camera.scale) */
  double depth_min, depth_max;  /* 0.1, 6 (PointCloudFilter.cpp:38; Config.cpp:29) */
  double voxel_leaf;            /* 0.01 (EllipsoidExtractor.cpp:98) */
  double plane_dist;            /* 0.05 (EllipsoidExtractor.cpp:570) */
  double cluster_tolerance;     /* 0.02 (TUM3.yaml:8) */
  int32_t min_cluster_size;     /* 100  (TUM3.yaml:9) */
  double center_dis;            /* 0.5  (TUM3.yaml:10) */
  int32_t symmetry_open;        /* 1 */
  double symmetry_grid;         /* 0.1 (TUM3.yaml:23) */
  double symmetry_sigma;        /* 0.1 (TUM3.yaml:26) */
  int32_t symmetry_lm_iters;    /* 5 in the reference; 0 = score the 9 hypotheses only */
} esl_fit_params;

void esl_fit_params_default(esl_fit_params* p);

int esl_fit_frame(esl_ctx* ctx, const uint16_t* depth, int32_t width, int32_t height,
                  const double* bboxes /* B x 4 */, const int32_t* labels /* B */, int32_t n_boxes,
                  const double Twc[7], const double intr[5] /* fx fy cx cy scale */,
                  const double ground[4], const esl_fit_params* p,
                  double* ellipsoids_out /* B x 10, camera frame */, double* prob_out /* B */,
                  int32_t* status_out /* B, mirrors miSystemState 0..4 */);

/* same, plus per-box stage counters for tests/profiling (16 doubles per box: [0] in-range samples, [1] voxels at
 * voxel_leaf, [2] after the supporting-plane filter, [3] clusters >= min_cluster_size, [4] chosen cluster size,
 * [5] voxels at symmetry_grid, [6..14] probability of the 9 symmetry hypotheses); debug_out may be NULL */
int esl_fit_frame_debug(esl_ctx* ctx, const uint16_t* depth, int32_t width, int32_t height, const double* bboxes,
                        const int32_t* labels, int32_t n_boxes, const double Twc[7], const double intr[5],
                        const double ground[4], const esl_fit_params* p, double* ellipsoids_out, double* prob_out,
                        int32_t* status_out, double* debug_out);

/* SymmetryOutputData (reference src/symmetry/Symmetry.h:16-32) as EstimateLocalEllipsoid fills it
 * (src/pca/EllipsoidExtractor.cpp:376-393, 415-423) and Tracking consumes it (src/core/Tracking.cpp:351-372):
 * result = 0 when no symmetry estimation ran for the box (symmetry closed, label without a symmetry type, fit failed);
 * planes are in the WORLD frame (A B C D of A x + B y + C z + D = 0, not normalised further), plane2 only for
 * symmetry_type 2 (dual reflection), prob = exp(-cost) of the winning hypothesis, center = centre of the completed
 * (mirrored) cloud in the world frame.  The point-cloud pointers of the reference struct stay on the device. */
typedef struct {
  int32_t result;
  int32_t symmetry_type;   /* 1 reflection, 2 dual reflection (EllipsoidExtractor::LoadSymmetryPrior, :52-79); -1 when result == 0 */
  double plane[4];
  double plane2[4];
  double prob;
  double center[3];
} esl_fit_symmetry;

/* esl_fit_frame + the symmetry outputs (what EllipsoidExtractor::GetSymmetryOutputData() returns, EllipsoidExtractor.h:61);
 * symmetry_out: n_boxes entries or NULL; debug_out as in esl_fit_frame_debug or NULL */
int esl_fit_frame_ex(esl_ctx* ctx, const uint16_t* depth, int32_t width, int32_t height, const double* bboxes,
                     const int32_t* labels, int32_t n_boxes, const double Twc[7], const double intr[5],
                     const double ground[4], const esl_fit_params* p, double* ellipsoids_out, double* prob_out,
                     int32_t* status_out, esl_fit_symmetry* symmetry_out, double* debug_out);

/* ---- ground plane -------------------------------------------------------------------------------*/
/* Replaces EllipsoidSLAM::PlaneExtractor (reference include/src/plane/PlaneExtractor.h:34-77, src/plane/PlaneExtractor.cpp):
 * SetParam's fields + the two constants extractPlanes passes to PCL's normal estimation (:57-58, :74). */
typedef struct esl_plane_params {
  int32_t min_size;               /* Plane.MinSize: smallest segment kept as a plane (PlaneExtractor.cpp:87) */
  double angle_threshold_deg;     /* Plane.AngleThreshold */
  double distance_threshold;      /* Plane.DistanceThreshold */
  int32_t normal_smoothing;       /* setNormalSmoothingSize(10) */
  double max_depth_change_factor; /* setMaxDepthChangeFactor(0.05) */
  int32_t min_inliers;            /* setMinInliers(100) */
  /* ABI 4: the second half of segmentAndRefine (PlaneExtractor.cpp:82) -- PCL's OrganizedMultiPlaneSegmentation::refine: two raster
   * passes in which a model (segment of > min_inliers pixels that passes the curvature test below) absorbs neighbouring pixels that belong to no model and lie within
   * refine_distance of its plane.  Grows the inlier lists (sizes, labels, which candidate is the largest), not the coefficients. */
  int32_t refine;                 /* 1 (default): as the reference; 0: segments only (the round 2-4 behaviour) */
  double refine_distance;         /* PlaneRefinementComparator's distance threshold: 0.02 m, not depth dependent */
  /* ABI 5: which segments PCL's segment() keeps as MODELS -- size > min_inliers (strict) and surface curvature
   * |lambda_min| / trace(cov) of the segment's points < maximum_curvature_ (PCL's default 0.001; the reference does not set it).  A
   * segment that fails either test is an "other" label, which the refinement pass lets neighbouring models absorb.  <= 0: no test. */
  double max_curvature;           /* 0.001 */
} esl_plane_params;
void esl_plane_params_default(esl_plane_params* p);
/* PlaneExtractor::extractGroundPlane(depth, plane) (PlaneExtractor.cpp:107-183): the largest plane segment of the depth image
 * whose normal is within 45 degrees of the camera's y axis, in the camera frame, normalised, camera centre on the positive
 * side.  *ok = 0 when no segment qualifies (the reference returns false).  n_planes (segments of >= min_size pixels) and
 * n_pixels (pixels of the returned segment) may be NULL.  The caller moves the plane to the world with the frame's pose as
 * Tracking::ProcessGroundPlaneEstimation does (src/core/Tracking.cpp:741-744). */
int esl_extract_ground_plane(esl_ctx* ctx, const uint16_t* depth, int32_t width, int32_t height, const double intr[5],
                             const esl_plane_params* p, double plane_out[4], int32_t* ok, int32_t* n_planes, int32_t* n_pixels);

/* PlaneExtractor::extractPlanes + GetCoefficients + GetPoints (PlaneExtractor.cpp:22-104, 113-123): every plane segment of
 * >= max(min_size, min_inliers) pixels, in raster order of each segment's first pixel.  planes_out: max_planes x 4 (camera
 * frame, normalised, d >= 0), sizes_out: pixels per plane; *n_planes = segments found (only the first max_planes are
 * written); labels_out: width x height plane index per pixel (-1: none; indices >= max_planes are reported as found) or NULL.
 * Labels with indices are what GetPoints() needs to rebuild the per-plane clouds on the host. */
int esl_extract_planes(esl_ctx* ctx, const uint16_t* depth, int32_t width, int32_t height, const double intr[5],
                       const esl_plane_params* p, int32_t max_planes, double* planes_out, int32_t* sizes_out,
                       int32_t* n_planes, int32_t* labels_out);

/* ---- SVD quadric initialisation -----------------------------------------------------------------*/
int esl_init_quadric(esl_ctx* ctx, const double* poses_Twc /* n x 7 */, const double* bboxes /* n x 4 */,
                     int32_t n, const double K[4], int32_t rows, int32_t cols, int32_t faithful,
                     double ellipsoid_out[10], double qstar_out[16], int32_t* ok);

/* Initializer::getEllipsoidFromQStar (reference include/core/Initializer.h:53, src/core/Initializer.cpp:186-248): pose and
 * half-axes from a dual quadric Q* (row-major 4x4).  faithful != 0 reproduces the reference's decomposition (4x4
 * eigenvalues for the half-axes), 0 the exact one through Q_33. */
int esl_init_from_qstar(esl_ctx* ctx, const double qstar[16], int32_t faithful, double ellipsoid_out[10], int32_t* ok);
/* Initializer::quadricErrorWithPlanes (include/core/Initializer.h:50, src/core/Initializer.cpp:271-284): sum over the
 * bbox tangent planes pi of (pi^T Q* pi)^2 for the given ellipsoid (10-vector, world frame). */
int esl_init_plane_error(esl_ctx* ctx, const double* poses_Twc /* n x 7 */, const double* bboxes /* n x 4 */, int32_t n,
                         const double K[4], int32_t rows, int32_t cols, const double ellipsoid[10], double* error_out);

/* ---- SVD quadric initialisation of many objects in one call (additive part of ABI 5: detect by the symbol) --------------------------
 * Initializer::initializeQuadric for many objects at once (Tracking::JudgeInitialization's loop, Tracking.cpp:581-608): one launch,
 * one wavefront per object, no allocation on a warm call.
 * Input.  The observations are an edge list: entry i says that frame obs_cam[i] saw object obs_obj[i] in the box obs_boxes[4 i ..].
 * esl_graph's bbox_cam / bbox_obj / bbox_meas can be passed as they are, and so can an assoc_out of esl_associate_boxes as obs_obj:
 * entries with obs_obj < 0 are skipped.  The observations of object o are the entries with obs_obj == o in list order; the list need
 * not be sorted.  Poses are Tcw (the graph's convention, NOT esl_init_quadric's Twc); the quaternion is normalised as the
 * SE3Quat(Vector7d) constructor does.
 * Per object the rules are esl_init_quadric's (Initializer.cpp:58-145): a detection with all four coordinates < 1 contributes
 * nothing; a line is kept iff its coordinate is > 0 and < cols - 1 (rows - 1 for y); the null vector of the plane matrix comes from
 * the one-sided Jacobi SVD on the matrix itself, signed so that Q*_33 > 0; faithful as in esl_init_from_qstar.
 * stats_out[4 o ..] = status, observations (all list entries of the object), planes (kept lines), spilled:
 *   status 0  initialised: every output written; plane_error_out[o] = quadricErrorWithPlanes (Initializer.cpp:271-284) of the
 *             returned ellipsoid over the object's own planes
 *   status 1  observations < min_observations (Tracking_MINIMUM_INITIALIZATION_FRAME, 15 in Config.cpp:29, or 0): every output of the
 *             object is zero, planes is 0
 *   status 2  otherwise, fewer than 9 planes: every output of the object is zero
 *   status 3  the decomposition rejected Q*: ellipsoid zero, qstar_out holds the SVD's Q* (as the single call does), plane error zero
 * The plane matrix of an object (320 bytes per observation) stays on chip up to T = 248 observations (objects of up to 96 use a
 * smaller tile of their own, so that more of them are resident); a larger object keeps its rows in a global slab, spilled = 1: the
 * same arithmetic through another pointer.  An object's outputs depend on its own observations alone, not on the rest of the batch.
 * ESL_ERR_INVALID: null or negative arguments (obs_* are needed whenever n_obs > 0, ellipsoids_out whenever N > 0), a non-skipped
 * entry with obs_cam outside [0, F) or obs_obj >= N, rows or cols < 1, n_obs >= 2^31, F differing from the resident graph's n_cams
 * when cams == NULL.  ESL_ERR_STATE: cams == NULL without a resident graph and states.  N = 0 and n_obs = 0 are valid.  The call
 * leaves the resident graph, its states and the solver blobs alone, keeps grow-only device buffers of its own (freed by
 * esl_ctx_destroy), runs on this context's GPU only and issues no collective.  With esl_profile_enable(ctx, 2) its launches are
 * bracketed as kernel class 4. */
int esl_init_quadrics(esl_ctx* ctx,
                      const double* cams /* F x 7 Tcw, NULL = resident camera states (F must equal n_cams) */, int32_t F,
                      int32_t N /* objects */,
                      const int32_t* obs_cam /* n_obs: frame index */, const int32_t* obs_obj /* n_obs: 0..N-1, < 0 = entry skipped */,
                      const double* obs_boxes /* n_obs x 4: x1 y1 x2 y2 */, int64_t n_obs,
                      const double K[4], int32_t rows, int32_t cols, int32_t faithful, int32_t min_observations,
                      double* ellipsoids_out /* N x 10 */, double* qstar_out /* N x 16 or NULL */,
                      double* plane_error_out /* N or NULL */, int32_t* stats_out /* N x 4 or NULL: status, observations, planes, spilled */);

/* ---- consensus SVD initialisation: esl_init_quadrics that rejects outlier boxes (additive part of ABI 5: detect by the symbol) -------
 * esl_init_quadrics takes the null vector of ALL tangent planes of an object: one box of a neighbouring object moves Q* far off or makes
 * the decomposition reject it.  esl_init_quadrics_robust fits small view subsets instead, scores every fit by the boxes it projects and
 * keeps the consensus: an exhaustive, totally ordered, bit-reproducible hypothesise-and-score search on the device.  Inputs, grouping,
 * conventions (Tcw poses, cams == NULL = the resident states, entries with obs_obj < 0 skipped), errors and resource behaviour are
 * esl_init_quadrics'.  Per object o with n list entries, local indices 0 .. n-1 in list order:
 *  1. Early statuses 1 (n < min_observations) and 2 (fewer than 9 kept lines over all entries) as in esl_init_quadrics.
 *  2. Hypotheses.  s = min(sample_size, n).  n <= sample_size: one hypothesis, h = 0, over all entries.  Otherwise h = 0 ..
 *     n_hypotheses - 1, and hypothesis h uses the s distinct indices of Floyd's sampling: for k = 0 .. s-1, j = n - s + k,
 *     t = (mix(seed, h, k) >> 11) % (j + 1); take t, or j if t was taken before.  mix = the splitmix64 finaliser (shifts 30, 27, 31,
 *     multipliers 0xBF58476D1CE4E5B9, 0x94D049BB133111EB) of seed ^ (0x9E3779B97F4A7C15 * (uint64)(32 h + k + 1)), all mod 2^64.  The
 *     indices are used in ascending order.  The stream depends on (seed, h, k, n) only: an object's result does not depend on the
 *     rest of the batch.
 *  3. Fit: the plane rows of the hypothesis's entries, the one-sided Jacobi SVD and the decomposition of esl_init_quadrics (the same
 *     line-keeping rule, sign convention, faithful and Tcw convention).  Invalid with fewer than 9 planes or a rejected Q*.
 *  4. Score over ALL n entries.  r_i = the largest |b_k - d_k| over entry i's kept lines, b the unclipped box of the projected outline
 *     as the bbox edge computes it; r_i = +inf when the bbox edge's visibility predicate (checkVisibility, Optimizer.cpp:35-81) fails,
 *     b is not finite, the entry has no kept line or all four of its coordinates are < 1.  Inlier iff r_i <= inlier_px; n_in = the
 *     inliers, cost = the sum of r_i^2 over them (a lane adds its entries i = lane, lane + 64, .. in rising order, then a fixed
 *     butterfly over the 64 lanes: the order depends on n alone).
 *  5. Winner: largest n_in, then smallest cost, then smallest h -- a total order.  No valid hypothesis: status 4.  A winner with
 *     n_in < min_inliers: status 5.
 *  6. refine != 0: esl_init_quadrics' own arithmetic over the winner's inlier entries (the same call, non-inliers skipped: small tile,
 *     large tile or slab by the inlier count), scored over all n entries, and kept iff it is valid and its (n_in, cost) is not worse.
 *     Then the final inlier set is the re-scored one and refined = 1; otherwise the winner's ellipsoid, Q* and set are returned.
 *  7. Outputs.  Status 0: the ellipsoid, its Q* (the SVD's) and quadricErrorWithPlanes over the planes of the final inlier entries.
 *     stats_out[8 o ..] = status, observations, planes (kept lines of ALL entries), spilled (the refit's), final inliers, valid
 *     hypotheses, winner h or -1, refined.  Statuses 1, 2, 4, 5: ellipsoid, Q* and plane error zero; 1 and 2 report status,
 *     observations and planes as esl_init_quadrics does, 0 valid hypotheses and winner -1; 4 adds planes; 5 also reports the winner,
 *     its inliers and the valid hypotheses.  inlier_out[i] = 1 / 0 and residual_out[i] = r_i under the RETURNED ellipsoid; 0 and NaN
 *     for skipped entries and for objects whose status is not 0.  hyp_out[(o n_hypotheses + h) 4 ..] = valid, planes, n_in, cost of
 *     hypothesis h, for tests and tuning; unused rows, and all rows of objects of status 1 or 2, are zero.
 * ESL_ERR_INVALID, beside esl_init_quadrics' cases: sample_size outside 3..16, n_hypotheses outside 1..1024, inlier_px not finite or
 * <= 0, min_inliers < 1, N * n_hypotheses >= 2^31.  The call keeps grow-only buffers of its own, allocates nothing when warm, issues no
 * collective, leaves the resident graph alone and brackets its launches as kernel class 4.  With refine it synchronises twice more than
 * esl_init_quadrics does: the host builds the refit's list from the winners' flags.
 * The defaults below are design choices, not values tuned on real data. */
typedef struct {
  int32_t sample_size;    /* 5: views per hypothesis, 3..16 */
  int32_t n_hypotheses;   /* 64: per object, 1..1024 */
  double  inlier_px;      /* 10: finite, > 0 */
  int32_t min_inliers;    /* 8: >= 1 */
  int32_t refine;         /* 1: re-fit on the winner's inliers, kept only when not worse */
  uint64_t seed;          /* 0 */
} esl_init_robust_params; /* 32 bytes */
void esl_init_robust_params_default(esl_init_robust_params* p);

int esl_init_quadrics_robust(esl_ctx* ctx, const double* cams /* F x 7 Tcw, NULL = resident camera states */, int32_t F, int32_t N,
                             const int32_t* obs_cam, const int32_t* obs_obj, const double* obs_boxes, int64_t n_obs,
                             const double K[4], int32_t rows, int32_t cols, int32_t faithful, int32_t min_observations,
                             const esl_init_robust_params* p /* NULL = defaults */,
                             double* ellipsoids_out /* N x 10 */, double* qstar_out /* N x 16 or NULL */, double* plane_error_out /* N or NULL */,
                             int32_t* stats_out /* N x 8 or NULL */, int32_t* inlier_out /* n_obs or NULL */, double* residual_out /* n_obs or NULL */,
                             double* hyp_out /* N x n_hypotheses x 4 or NULL: valid, planes, inliers, cost */);

/* ---- relocalisation: camera pose and detection -> map association with NO pose prior (additive part of ABI 5: detect by the symbol) ---
 * esl_optimize_fixed refines a pose that is already inside the basin of its edges and needs the edge lists, i.e. which detection is
 * which map ellipsoid.  esl_relocalize supplies both for one frame: from the frame's single-frame ellipsoids (esl_fit_frame's output,
 * camera frame), the ground plane seen from the camera and a fixed map with its ground plane, by an exhaustive, deterministic
 * hypothesise-and-score search on the device.  (The reference's only association, DataAssociationSolver, src/core/DataAssociation.cpp:
 * 16-135, takes the nearest map centre within 1 m GIVEN the pose; step 6 below is that rule.)
 *  1. Gravity frames.  A plane (n, d) is normalised by |n|; e_k = the coordinate axis with the smallest |n_k| (lowest k on ties),
 *     u = normalise(e_k x n), v = n x u, G(x) = [u; v; n] x + (0, 0, d): third coordinate = height above ground.  Map centres give
 *     p_m = G_w(C_m), detection centres q_d = G_c(c_d); the pose sought is x_w = G_w^-1(Z(yaw, t) G_c(x_c)), Z = rotation by yaw about
 *     z + (tx, ty, 0).
 *  2. Candidates: pairs (d, m) that pass the label, height and sorted-size gates of esl_reloc_params, in (d, m) lexicographic order;
 *     P of them.
 *  3. Hypotheses: candidate pairs i < j with different detections and different map objects, |q_dj - q_di|_xy >= min_baseline and
 *     | |q_dj - q_di|_xy - |p_mj - p_mi|_xy | <= 2 center_tol.  yaw = atan2 of the map difference - atan2 of the detection difference,
 *     t = midpoint(p) - R(yaw) midpoint(q).
 *  4. Score: every detection takes its nearest candidate by planar distance after the motion and is an inlier when that distance is
 *     <= center_tol; n = inliers, cost = sum of their squared distances.  Winner: max n, then min cost, then min key i P + j -- a total
 *     order, so the result does not depend on the order the hypotheses are processed in; runs are bit-reproducible.
 *  5. refine: closed-form 2-D rigid fit over the winner's inlier pairs (centred; yaw = atan2(sum cross, sum dot), t = mean p -
 *     R mean q), rescored once and kept only when its (n, cost) is not worse.  Runs from 3 inliers on: two pairs already are their fit.
 *  6. Association under the final pose: detections in index order, each takes its nearest UNCLAIMED candidate within center_tol.
 *     n_inliers and cost of the result are those of this association.
 * The defaults below are design choices, not values tuned on real data. */
typedef struct {
  double center_tol;      /* 0.25 m: planar distance below which a moved detection centre matches a map centre */
  double height_tol;      /* 0.25 m: |height above ground of detection - of map object| for a candidate */
  double size_ratio;      /* 1.5: candidate needs max_k |log(s_det[k] / s_map[k])| <= log(size_ratio), half-axes SORTED per ellipsoid; <= 1: no size gate */
  double min_baseline;    /* 0.5 m: smallest planar distance between the two detections of a hypothesis */
  int32_t min_inliers;    /* 3 */
  int32_t max_candidates; /* 4096 (at most 1048576) */
  int32_t match_labels;   /* 1: candidate needs equal labels; 0: labels ignored */
  int32_t refine;         /* 1: closed-form planar re-fit over the winner's inliers */
} esl_reloc_params;       /* 48 bytes */
void esl_reloc_params_default(esl_reloc_params* p);

/* The map: M x 10 world ellipsoids, M labels, the world ground plane.  objs == NULL: take the resident graph's current ellipsoid states
 * device-to-device (M must equal its n_objs; ESL_ERR_STATE without a graph and states).  The map lives in grow-only device buffers of
 * its own: it survives esl_graph_upload, esl_graph_append and esl_ctx_trim, and a later change of the resident states does not reach
 * it.  ESL_ERR_INVALID: null or negative arguments, a plane normal shorter than 1e-12. */
int esl_reloc_set_map(esl_ctx* ctx, const double* objs, const int32_t* labels, int32_t M, const double ground_world[4]);

typedef struct {
  int32_t status;         /* 0 found; 1 fewer than 2 candidates or no hypothesis passed the gates; 2 best hypothesis below min_inliers; 3 candidates > max_candidates, nothing scored */
  int32_t n_candidates;
  int64_t n_hypotheses;   /* pairs that passed every gate and were scored */
  int64_t best_key;       /* i * P + j of the winner (candidate indices i < j), -1 when none */
  int32_t n_inliers;      /* associated detections under the returned pose (status 2: the best hypothesis's inliers) */
  int32_t refined;        /* 1 if the re-fit pose was kept */
  double cost;            /* sum of squared planar distances of the associated detections (status 2: of the best hypothesis's inliers) */
  double yaw, tx, ty;     /* the planar motion in the gravity frames, yaw in (-pi, pi]; zeros unless status 0 */
  double Twc[7];          /* camera -> world, x y z qx qy qz qw, qw >= 0 */
} esl_reloc_result;

/* ESL_ERR_INVALID: null or negative arguments, a plane normal shorter than 1e-12, D > 64, non-finite tolerances, max_candidates above
 * 1048576.  ESL_ERR_STATE: no esl_reloc_set_map before.  Statuses 1-3 are results, not errors: the call returns ESL_OK, Twc holds the
 * identity (0 0 0 0 0 0 1) and assoc_out is -1 everywhere.  The call leaves the resident graph, its states and its solver blobs alone
 * and runs on this context's GPU only (on a context with a communicator too: no collective is issued). */
int esl_relocalize(esl_ctx* ctx, const double* det_objs /* D x 10, camera frame */, const int32_t* det_labels, int32_t D,
                   const double ground_cam[4], const esl_reloc_params* p /* NULL = defaults */,
                   esl_reloc_result* out, int32_t* assoc_out /* D: map index or -1; may be NULL */);

/* ---- 2-D data association: detection boxes against the projected map, GIVEN the poses (additive part of ABI 5: detect by the symbol) ---
 * The reference's association (DataAssociationSolver::Solve, src/core/DataAssociation.cpp:16-135) is 3-D only; its mb3D == false branch
 * is empty, so a detection without a depth ellipsoid gets -1 and its bbox edge is lost.  esl_associate_boxes fills that branch: it
 * predicts the box of every map ellipsoid in every frame with the projection the bbox edge evaluates, and assigns detections to
 * predictions by the reference's greedy rule (SolveCostMat, DataAssociation.cpp:90-135) with cost 1 - IoU.  Everything runs in FP64;
 * every choice is a total order, so the result does not depend on the order in which threads meet the candidates, and runs are
 * bit-reproducible.
 *  1. Prediction of map object m in frame f.  Eligible iff the bbox edge's visibility predicate holds (checkVisibility, Optimizer.cpp:
 *     35-81: centre in front of the camera, camera outside the ellipsoid, projected centre or a box corner inside the image), the box b
 *     of the projected outline is finite, and the clipped box c = (max(b0, 0), max(b1, 0), min(b2, cols), min(b3, rows)) is at least
 *     min_box_px wide AND high.  z_m = the camera-frame z of the centre.
 *  2. Occlusion (occlusion != 0).  An eligible m is occluded iff ONE other eligible m' is nearer (z_m' < z_m, or z_m' == z_m and
 *     m' < m) and covers it: area(c_m n c_m') >= occl_ratio * area(c_m).  An occluder may itself be occluded; there is no union of
 *     occluders (esl_render_map below counts, per pixel, what any number of nearer objects hide).  O(V^2) per frame over the V eligible
 *     predictions, exact.
 *  3. Assignment.  The detections of a frame are taken in index order.  The candidates of a detection are the eligible, non-occluded,
 *     unclaimed predictions, of equal label if match_labels.  It takes the candidate with the largest IoU(detection box as given, c_m),
 *     ties to the lowest m; if that IoU is >= min_iou and > 0 the pair is assigned and m is claimed for the rest of the frame,
 *     otherwise assoc = -1 and iou = 0.  A detection with a non-finite coordinate, x2 <= x1 or y2 <= y1 gets -1 and claims nothing. */
typedef struct {
  double min_iou;        /* 0.3: a detection is assigned only when its best IoU is >= this (and > 0) */
  double occl_ratio;     /* 0.7: share of a prediction's clipped box one nearer prediction must cover to hide it */
  double min_box_px;     /* 10: the clipped predicted box must be at least this wide AND this high */
  int32_t match_labels;  /* 1: candidates need equal labels; 0: labels ignored */
  int32_t occlusion;     /* 1: hidden predictions take no detection; 0: step 2 skipped */
} esl_assoc_params;      /* 32 bytes */
void esl_assoc_params_default(esl_assoc_params* p);

/* One frame's predictions (steps 1 and 2), for inspection and tests.  boxes_out holds c for eligible objects and NaN otherwise,
 * depth_out z_m or NaN, flags_out bit 0 eligible, bit 1 occluded.  objs == NULL: the resident graph's current ellipsoid states (M must
 * equal its n_objs).  Errors as esl_associate_boxes. */
int esl_predict_boxes(esl_ctx* ctx, const double Tcw[7], const double* objs /* M x 10 world, NULL = resident ellipsoid states */,
                      int32_t M, const double K[4], int32_t rows, int32_t cols, const esl_assoc_params* p /* NULL = defaults */,
                      double* boxes_out /* M x 4 */, double* depth_out /* M */, int32_t* flags_out /* M: bit 0 eligible, bit 1 occluded */);

/* Many frames.  frame_stats_out holds per frame: eligible predictions, occluded ones, assigned detections, spilled (1 when the frame's
 * eligible predictions did not fit the on-chip tile of 1,024 and went through global scratch; the result is the same bits).
 * ESL_ERR_INVALID: null or negative arguments (labels are needed whenever their count is > 0), offsets that do not start at 0 or
 * decrease, non-finite or negative min_iou / occl_ratio / min_box_px, rows or cols < 1, F or M differing from the resident graph when
 * the NULL forms are used.  ESL_ERR_STATE: a NULL source without a resident graph and states.  F = 0, M = 0 and a frame without
 * detections are valid; with M = 0 every detection gets -1.  The calls leave the resident graph, its states and its solver blobs alone,
 * keep grow-only device buffers of their own (freed by esl_ctx_destroy), run on this context's GPU only and issue no collective.  With
 * esl_profile_enable(ctx, 2) the kernel launches of a call are bracketed as kernel class 4. */
int esl_associate_boxes(esl_ctx* ctx, const double* cams /* F x 7 Tcw, NULL = resident camera states (F must equal n_cams) */, int32_t F,
                        const double* objs /* M x 10, NULL = resident (M must equal n_objs) */, const int32_t* obj_labels /* M */, int32_t M,
                        const double K[4], int32_t rows, int32_t cols,
                        const int32_t* det_offsets /* F + 1, CSR, non-decreasing, [0] = 0 */, const double* det_boxes /* n_det x 4: x1 y1 x2 y2 */,
                        const int32_t* det_labels /* n_det */, const esl_assoc_params* p /* NULL = defaults */,
                        int32_t* assoc_out /* n_det: map index or -1 */, double* iou_out /* n_det or NULL */,
                        int32_t* frame_stats_out /* F x 4 or NULL: eligible, occluded, assigned, spilled */);

/* ---- map maintenance: find and fuse duplicate ellipsoids of a map (additive part of ABI 5: detect by the symbol) --------------------------
 * Every call above takes the association as given; a detection that matches no prediction becomes a new instance at the caller
 * (CreateInstance, DataAssociation.cpp:127-131), so an object seen again after a gap, from the other side, after a loop closure, or
 * split off as outliers by esl_init_quadrics_robust stands in the map twice.  esl_map_merge decides which ellipsoids of a map are the same
 * object, fuses them and rewrites an edge list onto the repaired map, with the obs_obj < 0 = skipped convention of esl_init_quadrics
 * and esl_associate_boxes.  Everything runs in FP64; every decision is an integer comparison or a total order, so the result does not
 * depend on the order in which threads meet the pairs, and runs are bit-reproducible.
 *  1. Valid ellipsoid: all ten numbers finite, the quaternion's norm finite and > 0 (it is normalised), the half-axes s = (|a|, |b|, |c|)
 *     all > 0.  An invalid ellipsoid is in no pair and forms a group of its own.
 *  2. Lattice.  With n = lattice: the integer triples k = (kx, ky, kz), each 2 p + 1 - n for p = 0 .. n - 1, with |k|^2 <= n^2 (an integer
 *     test; no triple lies on the sphere), N_ball(n) of them: 32, 280, 2176, 17256 for n = 4, 8, 16, 32.  Unit-ball point u = k / n;
 *     sample of ellipsoid i: x = c_i + R_i (s_i o u).
 *  3. Counts.  cnt_ij = the samples of i with |diag(1 / s_j) R_j^T (x - c_j)|^2 <= 1, cnt_ji likewise with the roles swapped.
 *     V = 4/3 pi s0 s1 s2; inter = (cnt_ij V_i + cnt_ji V_j) / (2 N_ball); iou = inter / (V_i + V_j - inter);
 *     contain = min(1, inter / min(V_i, V_j)).  The lattice, not a closed form: there is none for two oriented ellipsoids, and counts
 *     are integers, which every device reproduces.  The estimator's error at n = 16 is about 0.006 in IoU (tests/map_merge_scenes.py).
 *  4. Candidates: the pairs i < j of valid ellipsoids, of equal label if match_labels, with |c_i - c_j|^2 <= (r_i + r_j)^2 (1 + 1e-9),
 *     r = max(s) -- a pair that fails this has both counts 0, the gate only saves work.  All pairs are tried (M <= 65536).  The
 *     OVERLAPPING pairs are the candidates with cnt_ij + cnt_ji > 0, in (i, j) lexicographic order.  More than max_pairs candidates:
 *     status 3, nothing is merged.
 *  5. Links: an overlapping pair with iou >= min_iou or contain >= min_contain.  Groups are the connected components of the links, so
 *     chains merge transitively: A ~ B and B ~ C puts all three in one group even when A and C do not overlap.  A group's id is its
 *     smallest member index.
 *  6. Weights: int32 >= 0 with a total below 2^31; weights == NULL: the number of an object's list entries, or 1 for every object when
 *     no list is given.  The representative of a group is the member with the largest weight, ties to the lowest index.  Groups are
 *     numbered 0 .. n_groups - 1 in ascending order of group id, so unmerged objects keep their relative order.  Row g of the merged map
 *     is the representative's ten numbers bit for bit -- no averaging of poses: an ellipsoid's axes are defined only up to permutation
 *     and sign --, the merged label is the representative's, the merged weight the integer sum of the members' weights.
 *  7. Edge list (n_obs > 0): obs_obj_out[e] = new_index[obs_obj[e]], entries with obs_obj < 0 stay -1.  Of the entries that now share
 *     one (obs_cam, new object) -- both copies were boxed in one frame -- the one survives that comes first in the total order: larger
 *     weight of the ORIGINAL object, then lower original index, then lower list position.  The others become -1 and are counted in
 *     n_conflicts. */
typedef struct {
  int32_t lattice;      /* 16: n of step 2, 4 .. 32 */
  int32_t match_labels; /* 1: candidates need equal labels; 0: labels ignored */
  double min_iou;       /* 0.3: finite, in (0, 1] */
  double min_contain;   /* 0.7: finite, > 0; > 1 = containment never links */
  int32_t max_pairs;    /* 4194304: more candidates than this give status 3 */
  int32_t pad;
} esl_merge_params;     /* 32 bytes; design choices, not values tuned on real data */
void esl_merge_params_default(esl_merge_params* p);

/* Inspection and tests: the overlapping pairs of step 4 with their integers and measures.  n_pairs reports how many were found, only the
 * first cap of them are written; with more than max_pairs candidates n_candidates reports them, n_pairs is -1 and nothing is written.
 * Errors as esl_map_merge. */
int esl_map_overlaps(esl_ctx* ctx, const double* objs /* M x 10, NULL = resident ellipsoid states (M must equal n_objs) */,
                     const int32_t* labels /* M */, int32_t M, const esl_merge_params* p /* NULL = defaults */, int64_t cap,
                     int32_t* pairs_out /* cap x 2: i, j */, int32_t* counts_out /* cap x 2: cnt_ij, cnt_ji */, double* iou_out /* cap */,
                     double* contain_out /* cap */, int64_t* n_pairs, int64_t* n_candidates);

typedef struct {
  int32_t status;            /* 0 ok, 3 candidates > max_pairs */
  int32_t n_valid, n_groups;
  int32_t n_merged_groups;   /* groups of more than one member */
  int32_t largest_group, n_conflicts;
  int64_t n_candidates, n_pairs, n_links;
} esl_merge_result;          /* 48 bytes */

/* Steps 1 - 7.  Status 3 is a result, not an error: the return is ESL_OK, the last error text is left alone, every object is its own
 * group (new_index = 0 .. M - 1, the merged map is the input, the weights are each object's own) and obs_obj_out is obs_obj with the
 * negative entries as -1.
 * ESL_ERR_INVALID: null or negative arguments (labels and the five map outputs are needed whenever M > 0, obs_cam and obs_obj whenever
 * n_obs > 0), M > 65536, lattice outside 4 .. 32, min_iou not finite or outside (0, 1], min_contain not finite or <= 0, max_pairs < 0,
 * a negative weight or a weight total >= 2^31, n_obs >= 2^31, a non-skipped entry with obs_obj >= M or obs_cam < 0, M differing from
 * the resident graph's n_objs when objs == NULL.  ESL_ERR_STATE: objs == NULL without a resident graph and states.  M = 0 and n_obs = 0
 * are valid.  The calls leave the resident graph, its states and the solver blobs alone, keep grow-only device buffers of their own
 * (freed by esl_ctx_destroy; a warm call allocates nothing), run on this context's GPU only and issue no collective.  With
 * esl_profile_enable(ctx, 2) their launches are bracketed as kernel class 4. */
int esl_map_merge(esl_ctx* ctx, const double* objs /* M x 10, NULL = resident ellipsoid states */, const int32_t* labels /* M */,
                  const int32_t* weights /* M or NULL */, int32_t M,
                  const int32_t* obs_cam /* n_obs */, const int32_t* obs_obj /* n_obs: 0..M-1, < 0 = entry skipped */, int64_t n_obs /* may be 0 */,
                  const esl_merge_params* p /* NULL = defaults */,
                  int32_t* group_out /* M: group id */, int32_t* new_index_out /* M: row of the merged map */,
                  double* merged_objs_out /* M x 10, the first n_groups rows are written */, int32_t* merged_labels_out /* M */,
                  int32_t* merged_weights_out /* M */, int32_t* obs_obj_out /* n_obs or NULL */, esl_merge_result* out);

/* ---- rendering the map: per-pixel depth, instance and visibility (additive part of ABI 5: detect by the symbol) ---------------------------
 * Every call above sees an ellipsoid in an image through its bounding box only.  esl_render_map casts the ray of every pixel of every
 * frame against every ellipsoid of the map and keeps the nearest hit: which pixels show which object (the union of occluders that
 * esl_associate_boxes leaves out), and, against a measured depth image, whether the sensor agrees with the map, stops short of it (an
 * unmodelled occluder) or sees through it (a moved or removed object).  The reference only draws its map (FrameDrawer::
 * drawProjectionOnImage, Pangolin).  Everything runs in FP64; every choice is a strict comparison or a total order and the only atomics
 * are integer atomics, so runs are bit-reproducible.
 *  1. Valid object, as step 1 of esl_map_merge: all ten numbers finite, the quaternion's norm finite and > 0 (it is normalised), the
 *     half-axes s = (|a|, |b|, |c|) all > 0.  An invalid object hits no pixel (flag bit 1).
 *  2. Camera-frame body.  With Rco = Rcw Rwo and tco = Rcw two + tcw as the bbox edge forms them: A = Rco diag(1 / s^2) Rco^T, g = A tco,
 *     c0 = tco^T A tco - 1.  c0 <= 0: the camera centre is inside or on the body, which is not drawn in this frame (flag bit 2).
 *  3. Ray of pixel (col, row): d = ((col - cx) / fx, (row - cy) / fy, 1), the integer-pixel convention with which esl_fit_frame and the
 *     plane extraction back-project a depth sample.  alpha = d^T A d, beta = d^T g, Delta = beta^2 - alpha c0.  Hit iff beta > 0 and
 *     Delta > 0, both strict (a grazing ray is no hit); z = c0 / (beta + sqrt(Delta)), the near root of z^2 alpha - 2 z beta + c0 = 0 in the
 *     form without cancellation.
 *  4. Pixel: the hit with the smallest z wins, ties to the lowest m.  depth_out = z, inst_out = m; NaN / -1 without a hit.
 *  5. Counts per (frame, object): cover[0] = the pixels it hits, whatever else is there; cover[1] = the pixels it wins.  The caller's
 *     visibility is cover[1] / cover[0].
 *  6. Depth comparison over the pixels m wins, with r the raw sample and z_meas = r / depth_scale: r == 0 or z_meas outside
 *     [depth_min, depth_max] -> no data; |z_meas - z| <= depth_tol -> agree; z_meas < z - depth_tol -> nearer (something unmodelled stands
 *     in front); otherwise farther (the sensor sees through the object).  The four counts of an object sum to its cover[1].
 * flags_out per (frame, object): bit 0 drawn (valid, camera outside, not wholly behind the principal plane), bit 1 invalid, bit 2 camera
 * inside, bit 3 bounded by its conic box: the body lies wholly in front of the principal plane (the dual conic's C22 < 0, tco_z > 0, the
 * outline's box finite), so the kernel tests it only on the pixels of that box widened by one.  A body wholly behind has no flag; one
 * that meets the principal plane is tested on every pixel.  These bounds only cull: they never change a result. */
typedef struct {
  double depth_scale;  /* 5000: raw units per metre, intr[4] of esl_fit_frame */
  double depth_min;    /* 0.1 */
  double depth_max;    /* 6.0: a measured sample outside [depth_min, depth_max], or raw 0, is "no data" */
  double depth_tol;    /* 0.05 m: |z_meas - z| <= depth_tol agrees */
} esl_render_params;   /* 32 bytes; design choices, not tuned on real data */
void esl_render_params_default(esl_render_params* p);

/* ESL_ERR_INVALID: null ctx or K, negative F or M, rows or cols < 1 or > 16384, fx or fy not finite or <= 0, a non-finite or negative
 * parameter, depth_scale <= 0, depth_min > depth_max, cmp_out without depth_meas, F or M differing from the resident graph when the NULL
 * forms are used.  ESL_ERR_STATE: a NULL source without a resident graph and states.  F = 0, M = 0 and all outputs NULL are valid; with
 * M = 0 the images are NaN / -1.  An output that is not asked for is neither computed into nor allocated; depth_meas without cmp_out is
 * not read.  The call leaves the resident graph, its states and the solver blobs alone, keeps grow-only device buffers of its own (freed
 * by esl_ctx_destroy; a warm call of the same shape allocates nothing; at most F (96 M + 14 rows cols) bytes), runs on this context's GPU
 * only and issues no collective.  With esl_profile_enable(ctx, 2) its launches are bracketed as kernel class 4. */
int esl_render_map(esl_ctx* ctx,
                   const double* cams /* F x 7 Tcw, NULL = resident camera states (F must equal n_cams) */, int32_t F,
                   const double* objs /* M x 10 world, NULL = resident ellipsoid states (M must equal n_objs) */, int32_t M,
                   const double K[4], int32_t rows, int32_t cols,
                   const uint16_t* depth_meas /* F x rows x cols or NULL */, const esl_render_params* p /* NULL = defaults */,
                   double* depth_out /* F x rows x cols or NULL: z of the nearest hit, NaN where none */,
                   int32_t* inst_out /* F x rows x cols or NULL: its map index, -1 where none */,
                   int32_t* cover_out /* F x M x 2 or NULL: pixels the object hits alone; pixels where it is the nearest */,
                   int32_t* cmp_out /* F x M x 4 or NULL, needs depth_meas: agree, nearer, farther, no data (over the pixels it wins) */,
                   int32_t* flags_out /* F x M or NULL: bit 0 drawn, bit 1 invalid, bit 2 camera inside, bit 3 bounded by its conic box */);

/* ---- the dense map: voxel-fused points of many RGB-D frames (additive part of ABI 5: detect by the symbol) ---------------------------------
 * The reference's dense builder (src/dense_builder/builder.cpp, Tracking.cpp:232-249) back-projects every depth pixel of every frame,
 * moves it into the world with the frame's pose and voxel-filters the growing cloud at 1 cm, re-filtering already filtered centroids
 * every frame: its result depends on the frame order and on float summation.  Here the map is stated the way esl_fit_frame states its
 * voxel grid: every sample of every frame counts once, all sums are integers, the result is a function of the SET of samples alone.
 * Everything is FP64 and integers; every reduction is an integer sum or a total order, so the map after any sequence of
 * esl_dense_add_frames calls equals, bit for bit, the map after one call with all the frames, in any frame order, from run to run.
 * Frames may differ in size and intrinsics from call to call.
 *  1. Sample: pixel (col, row) of frame f with row and col multiples of stride (n_sampled).  r = the raw depth; r == 0 counts in n_zero.
 *     z = r / depth_scale; z < depth_min or z > depth_max counts in n_depth_out.  p_c = ((col - cx) z / fx, (row - cy) z / fy, z):
 *     multiply, then divide (builder.cpp:66-67), integer pixels as in esl_fit_frame and esl_render_map.
 *  2. World point.  Poses are Tcw = (t, q), the graph's convention.  The quaternion is divided by its norm sqrt(x^2 + y^2 + z^2 + w^2)
 *     (summed left to right), R is the rotation matrix by the library's formula (R00 = 1 - (2y y + 2z z), R01 = 2y x - 2z w, ...),
 *     d = p_c - t, p_w[a] = (R[0][a] d0 + R[1][a] d1) + R[2][a] d2: p_w = R^T (p_c - t).  No product is contracted with a sum.  A
 *     non-finite pose number, or a quaternion whose norm is 0 or not finite, gives ESL_ERR_INVALID before anything is added.
 *  3. Key: k_a = floor(p_w[a] / leaf).  |k_a| > 2^20 - 1 on any axis (or not finite) counts in n_key_out and the sample is dropped;
 *     the others count in n_used.  Packed key = (kx + 2^20) << 42 | (ky + 2^20) << 21 | (kz + 2^20): its unsigned order is the
 *     lexicographic order of (kx, ky, kz).
 *  4. Voxel: count; S_a = the sum of llrint(p_w[a] 2^30) as int64; with colour the sums of B, G and R.  n_samples may not reach 2^31:
 *     a call whose sampled pixels (before the depth test) could take it there returns ESL_ERR_INVALID and adds nothing.  S_a itself
 *     is exact while count * max |p_w[a]| of a voxel stays below 2^33 m (it wraps beyond).
 *  5. Votes (with_inst): per (voxel, id >= 0) the number of samples.  A voxel's label is the id with the most samples, ties to the
 *     lowest id; votes is that number; -1 / 0 without a labelled sample.
 *  6. Capacity: the voxel table has the smallest power of two >= 2 max_voxels slots, the pair table twice that.  More than max_voxels
 *     voxels, or more than 2 max_voxels pairs, sets the sticky status 3 -- a result, not an error: the return is ESL_OK.  From then on
 *     the map is invalid until the next esl_dense_begin: esl_dense_add_frames adds nothing more (its counts are 0), esl_dense_extract
 *     writes nothing and reports n_voxels = -1, esl_dense_info_get reports n_voxels = n_pairs = -1.  No probe loop is unbounded.
 *  7. Extract: the voxels in ascending packed-key order, the first cap of them written, n_voxels reporting all.  key_out = (kx, ky, kz);
 *     xyz_out[a] = (double)S_a / 2^30 / (double)count; bgr_out = (2 sum + count) / (2 count) in integers (0 on a map without colour);
 *     inst_out / votes_out as step 5 (-1 / 0 on a map without labels).  Extract does not change the map; adds and extracts may alternate.
 * The map follows the poses (esl_dense_remove_frames / _move_frames / _purge / _slots_get, below the calls above).  Every per-voxel
 * quantity is an integer sum, so subtracting a frame's samples is the exact inverse of adding them.  The contract: while the status
 * stays 0, any interleaving of add, remove, move and purge calls leaves the map that esl_dense_begin and ONE esl_dense_add_frames of
 * the multiset difference (the samples added and not removed) would leave -- the same bytes in every output of esl_dense_extract,
 * esl_dense_objects and esl_dense_planes and in esl_dense_info.  Only esl_dense_slots_get and the capacity status (step 11) may tell
 * the two apart.
 *  8. Remove.  The samples of the given frames are formed by steps 1 to 3 exactly as esl_dense_add_frames forms them (the same
 *     arithmetic, pose handling and validation; n_sampled, n_zero, n_depth_out, n_key_out and n_used mean the same).  Every used
 *     sample subtracts from its voxel what adding it would have added: 1 from count, llrint(p_w[a] 2^30) from S_a, its B, G and R
 *     from the colour sums and, with labels and id >= 0, one vote from its (voxel, id) pair.  Removal only looks up: it claims no
 *     voxel slot and no pair slot.  A used sample whose voxel is not in the table counts in n_missing and subtracts nothing; one whose
 *     voxel is there but whose (voxel, id) pair is not counts in n_missing too: its voxel is still decremented, no vote is subtracted.
 *     n_emptied = the number of voxels whose count this call took to 0.  n_samples drops by n_used.
 *  9. Live and dead; consistency.  A claimed voxel slot with count > 0 is live, with count == 0 dead; the same holds for a pair slot
 *     and its 32-bit count.  After every removing call an audit pass over both tables recounts the live and the dead slots and sets
 *     the sticky status 4 (inconsistent) when n_missing > 0, a voxel count is negative as int64, a dead voxel has a non-zero S_a or
 *     colour sum, a pair count has bit 31 set, or a live pair belongs to a dead voxel: something was removed that had not been added
 *     as given.  Status 4 is a result like status 3, with the same consequences: the return is ESL_OK; nothing more is added or removed
 *     until the next esl_dense_begin (the calls' counts are 0); esl_dense_extract, esl_dense_objects and esl_dense_planes report
 *     n_voxels = -1 and write nothing; esl_dense_info_get reports n_voxels = n_pairs = -1.  A map at status 3 stays at 3.
 * 10. What the rest sees: live slots only.  esl_dense_info's n_voxels and n_pairs count live slots; extract, objects and planes list
 *     live voxels, and a dead voxel is no neighbour of a component; a dead pair casts no vote.  A dead slot keeps its key until a
 *     purge, so no probe chain loses a link, and a later add of the same key revives it.
 * 11. Capacity counts CLAIMED slots, live plus dead: status 3 is raised when the claimed voxel slots exceed max_voxels or the claimed
 *     pair slots 2 max_voxels (on a map without removals: step 6).  esl_dense_purge rebuilds both tables from the live records and
 *     the live pairs alone: afterwards claimed = live and dead = 0, and nothing any other call reports has changed.
 *     esl_dense_slots_get reports the claimed and the dead slots of both tables (-1 four times on a map whose status is not 0).
 * Move (esl_dense_move_frames) = remove with cams_old (step 8), then add with cams_new (steps 1 to 5), in one call and with one upload
 * of the images, for the frames whose seven cams_old doubles differ from their cams_new doubles in any bit (n_frames_moved); the
 * others are skipped (n_frames_same).  Every check runs before anything changes: all poses of both sets, and n_samples + (sampled
 * pixels of a frame) n_frames_moved < 2^31 (conservative: the removal is not credited).  If the removal ends in status 4, nothing is
 * added. */
typedef struct {
  double  leaf;         /* 0.01 m  (Tracking.cpp:241 voxelFilter(0.01)); finite, > 0 */
  double  depth_scale;  /* 5000   raw units per metre; finite, > 0 */
  double  depth_min;    /* 0.5    (builder.cpp:63) */
  double  depth_max;    /* 6.0    (depth_thresh); finite, depth_min <= depth_max */
  int32_t stride;       /* 1: every stride-th row and column from 0; >= 1 */
  int32_t max_voxels;   /* 1048576: 1 .. 2^26 */
} esl_dense_params;     /* 40 bytes; design choices except where a reference line is named */
void esl_dense_params_default(esl_dense_params* p);

/* Start an empty map (forgetting any earlier one of this context).  ESL_ERR_INVALID: null ctx, a bad parameter, a negative flag.  The
 * tables take 72 bytes per slot, 24 more per slot with labels: 144 MiB / 192 MiB at the default max_voxels. */
int esl_dense_begin(esl_ctx* ctx, const esl_dense_params* p /* NULL = defaults */, int32_t with_color, int32_t with_inst);

typedef struct { int64_t n_sampled, n_zero, n_depth_out, n_key_out, n_used; int32_t status, pad; } esl_dense_add_result; /* 48 bytes */
/* ESL_ERR_STATE: no esl_dense_begin before; bgr or inst NULL when esl_dense_begin asked for them (passing them when it did not is
 * allowed: they are not read); cams == NULL without a resident graph and states.  ESL_ERR_INVALID: null ctx, K or depth, negative F,
 * rows or cols < 1 or > 16384, fx or fy not finite or <= 0, an invalid pose (step 2), n_samples reaching 2^31 (step 4), F differing
 * from the resident graph's n_cams when cams == NULL.  F = 0 is valid.  An error leaves the map as it was. */
int esl_dense_add_frames(esl_ctx* ctx, const double* cams /* F x 7 Tcw, NULL = resident camera states */, int32_t F,
                         const double K[4], int32_t rows, int32_t cols,
                         const uint16_t* depth /* F x rows x cols */, const uint8_t* bgr /* F x rows x cols x 3 or NULL */,
                         const int32_t* inst /* F x rows x cols or NULL: esl_render_map's inst_out or any labelling, < 0 = none */,
                         esl_dense_add_result* out /* this call's counts; may be NULL */);

typedef struct { int64_t n_samples; int32_t n_voxels, n_pairs, status, with_color, with_inst, pad; } esl_dense_info; /* 32 bytes */
int esl_dense_info_get(esl_ctx* ctx, esl_dense_info* out);

/* ESL_ERR_INVALID: null ctx or n_voxels, negative cap.  ESL_ERR_STATE: no esl_dense_begin before.  Any output may be NULL. */
int esl_dense_extract(esl_ctx* ctx, int64_t cap, int32_t* key_out /* cap x 3 */, double* xyz_out /* cap x 3 */, int32_t* count_out /* cap */,
                      uint8_t* bgr_out /* cap x 3 */, int32_t* inst_out /* cap */, int32_t* votes_out /* cap */, int64_t* n_voxels);
int esl_dense_end(esl_ctx* ctx);   /* forget the map; the buffers stay (grow-only), esl_ctx_destroy frees them */

/* Steps 8 to 11 (additive part of ABI 5: detect by the symbol). */
typedef struct { int64_t n_sampled, n_zero, n_depth_out, n_key_out, n_used, n_missing, n_emptied; int32_t status, pad; } esl_dense_remove_result; /* 64 bytes */
/* Errors as esl_dense_add_frames, case by case (the frames' sampled pixels reaching 2^31 in place of n_samples).  F = 0 is valid.  An
 * error leaves the map as it was. */
int esl_dense_remove_frames(esl_ctx* ctx, const double* cams /* F x 7 Tcw, the poses the frames were added with; NULL = resident */,
                            int32_t F, const double K[4], int32_t rows, int32_t cols,
                            const uint16_t* depth /* F x rows x cols */, const uint8_t* bgr /* F x rows x cols x 3 or NULL */,
                            const int32_t* inst /* F x rows x cols or NULL */, esl_dense_remove_result* out /* may be NULL */);

typedef struct { esl_dense_remove_result removed; esl_dense_add_result added; int32_t n_frames_moved, n_frames_same; } esl_dense_move_result; /* 120 bytes */
/* Errors as esl_dense_add_frames, case by case (cams_new in the place of cams); ESL_ERR_INVALID also for a null cams_old with F > 0
 * and an invalid pose in either set. */
int esl_dense_move_frames(esl_ctx* ctx, const double* cams_old /* F x 7, not NULL */,
                          const double* cams_new /* F x 7, NULL = resident camera states */, int32_t F, const double K[4], int32_t rows,
                          int32_t cols, const uint16_t* depth, const uint8_t* bgr, const int32_t* inst,
                          esl_dense_move_result* out /* may be NULL */);

typedef struct { int64_t voxel_slots, dead_voxels, pair_slots, dead_pairs; } esl_dense_slots; /* 32 bytes: claimed slots and the dead among them */
/* ESL_ERR_INVALID: null ctx (esl_dense_slots_get: or out).  ESL_ERR_STATE: no esl_dense_begin before.  On a map whose status is not 0
 * both return ESL_OK and esl_dense_purge does nothing.  before / after: the slots ahead of and behind the purge. */
int esl_dense_slots_get(esl_ctx* ctx, esl_dense_slots* out);
int esl_dense_purge(esl_ctx* ctx, esl_dense_slots* before /* or NULL */, esl_dense_slots* after /* or NULL */);
/* The calls leave the resident graph, its states and the solver blobs alone, keep grow-only device buffers of their own (a warm call
 * allocates nothing), run on this context's GPU only and issue no collective.  With esl_profile_enable(ctx, 2) their launches are
 * bracketed as kernel class 4.  esl_debug_dense_allocs: the device allocations these calls have made on this context and the bytes
 * their buffers hold (the owner has no value in esl_scratch_owner). */
int esl_debug_dense_allocs(esl_ctx* ctx, int64_t* allocs_out, int64_t* bytes_out);

/* ---- per-instance ellipsoids from the dense map (additive part of ABI 5: detect by the symbol) ------------------------------------------
 * The reference estimates an object's ellipsoid from the depth points of ONE view (EllipsoidExtractor.cpp; esl_fit_frame).  The dense
 * map holds the same object seen from every frame, deduplicated, exactly summed and labelled by vote.  esl_dense_objects answers, per
 * instance label of that map: which voxels hang together, and which gravity-aligned ellipsoid bounds the largest connected set.  It
 * is the map-side twin of esl_fit_frame: voxel centres instead of points, connected components instead of Euclidean clustering, the
 * same gravity-aligned PCA and extent rule.  Integers and total orders decide everything discrete; runs are bit-reproducible and do
 * not depend on the order the frames were added in.
 *  1. Kept voxel.  A voxel of the map (dense-map steps 3 to 5) has its integer key k, count, label and votes.  Three tests run in
 *     this order and a voxel is counted at the first one it fails: label in [0, N) (passing: n_in_range); votes >= min_votes and
 *     count >= min_count (passing: n_gated); height h >= plane_dist (passing: n_kept).  Centre x_a = ((double)k_a + 0.5) leaf.  The
 *     plane is normalised once on the host: n^ = n / |n|, d^ = d / |n|, |n| = sqrt(n0^2 + n1^2 + n2^2) summed left to right;
 *     h = (n^0 x0 + n^1 x1) + n^2 x2 + d^.  No product is contracted with a sum.
 *  2. Components.  Two kept voxels of equal label are linked iff max_a |k_a - k'_a| <= reach; components are the connected components
 *     of the links.  A component's key is the smallest packed key of its members, its size the number of members, its samples the
 *     integer sum of the members' counts.  n_components_all counts every component.
 *  3. Table: the components of size >= min_component, sorted by label ascending, then size descending, then key ascending;
 *     n_components rows.  More rows than max_components give out->status = 3 -- a result, the return is ESL_OK --: objs_out and
 *     stats_out are zero, the first min(comp_cap, n_components) rows of comp_out are zero, voxel_comp_out is -1, n_ok is 0; the
 *     counts of the result stand.  comp_out row: label, size, samples, kx, ky, kz of the key; the first comp_cap rows are written.
 *  4. Object o: its chosen component is the first table row of label o.  Status 1: no kept voxel of label o; 2: kept voxels but no
 *     table row; 6: the guard of step 5; 0 otherwise.  A non-zero status zeroes the object's ten numbers.
 *  5. Moments of the chosen component, all int64: kmin_a, kmax_a over the members; d = k - kmin, n = size, s_a = sum d_a,
 *     M_ab = sum d_a d_b.  Guard: with span = max_a (kmax_a - kmin_a + 1) the object takes status 6 when n span^2 >= 2^62 (tested in
 *     integers without overflowing): below it no sum can leave int64.  A connected component needs some 8e5 voxels in a line to reach it.
 *  6. Frame.  The gravity basis (u, v, n^) by the rule of esl_relocalize step 1: e_k = the axis with the smallest |n^_k| (lowest k on
 *     ties), u = normalise(e_k x n^), v = n^ x u.  m_a = s_a / n, C_ab = M_ab / n - m_a m_b (voxel units), C_uu = u^T C u, C_uv =
 *     u^T C v, C_vv = v^T C v, each a^T C b = (a0 r0 + a1 r1) + a2 r2 with r_i = (C_i0 b0 + C_i1 b1) + C_i2 b2.  theta = 0.5 atan2(2 C_uv,
 *     C_uu - C_vv), x = cos theta u + sin theta v, y = n^ x x, R = [x y n^] (columns).
 *  7. Extents over the members: the projections (x0 p0 + x1 p1) + x2 p2 of every member's centre p, the same with y and with n^;
 *     minimum and maximum of each.  Centre coordinate = (min + max) / 2, half-axis = (max - min) / 2 + leaf / 2: the box of the
 *     members' voxel centres grown by half a voxel, the reference's extent rule (esl_fit_frame's last step).
 *  8. Output row: t_a = (x_a c_x + y_a c_y) + n^_a c_z; q = the library's rotation-to-quaternion of R, negated when qw < 0; a, b, c =
 *     the half-axes along x, y, n^.  stats_out[6 o ..] = status, kept voxels of the label, table rows of the label, the chosen row
 *     or -1, size and samples of the chosen component.  out->n_ok counts the objects of status 0.
 *  9. voxel_comp_out[i] for the i-th voxel in ascending packed-key order (esl_dense_extract's order), the first voxel_cap written:
 *     the table row of the voxel's component; -2 kept, but in a component below min_component; -1 not kept.
 * Voxel CENTRES are used, not the voxels' centroids, and the reach is a Chebyshev distance on keys, not a Euclidean radius. */
typedef struct {
  int32_t reach;           /* 2: voxels link when max_a |k_a - k'_a| <= reach (integer keys); 1..3.  2 = the reference's 2 cm cluster tolerance at the 1 cm leaf */
  int32_t min_votes;       /* 1: a voxel takes part only with votes >= this */
  int32_t min_count;       /* 1: ... and count (samples) >= this */
  int32_t min_component;   /* 100: components with fewer voxels are not objects (MinClusterSize, TUM3.yaml:9) */
  int32_t max_components;  /* 65536: more table rows than this give status 3; 1 .. 2^20 */
  int32_t pad;
  double  plane_dist;      /* 0.05 m: voxels whose centre is lower than this above the ground are dropped (EllipsoidExtractor.cpp:570); finite */
} esl_dense_obj_params;    /* 32 bytes; design choices except where a reference line is named */
void esl_dense_obj_params_default(esl_dense_obj_params* p);

typedef struct { int32_t status, n_voxels, n_in_range, n_gated, n_kept, n_components_all, n_components, n_ok; } esl_dense_obj_result; /* 32 bytes */

/* ESL_ERR_INVALID: null ctx, ground_world or out; N < 0 or a negative cap; objs_out NULL with N > 0; a cap > 0 with its array NULL; a
 * non-finite plane number or |n| < 1e-12; reach outside 1..3; min_votes, min_count or min_component < 1; max_components outside
 * 1..2^20; plane_dist not finite.  ESL_ERR_STATE: no esl_dense_begin before; a map begun without labels.  A map over its capacity
 * (sticky status 3) is not an error: ESL_OK, out->status = 3, n_voxels = -1, nothing else is written.  N = 0 and an empty map are valid.
 * The call changes nothing in the map except the best words, which it rebuilds as esl_dense_extract does: adds, extracts and object
 * calls may alternate.  Its buffers are the dense map's own (grow-only; a warm call of a shape no larger than an earlier one allocates
 * nothing: esl_debug_dense_allocs); one GPU, no collective, launches bracketed as kernel class 4. */
int esl_dense_objects(esl_ctx* ctx, int32_t N /* labels 0 .. N-1 are objects */, const double ground_world[4],
                      const esl_dense_obj_params* p /* NULL = defaults */,
                      double* objs_out /* N x 10 world ellipsoids */, int32_t* stats_out /* N x 6 or NULL */,
                      int64_t comp_cap, int32_t* comp_out /* comp_cap x 6 or NULL */,
                      int64_t voxel_cap, int32_t* voxel_comp_out /* voxel_cap or NULL, in esl_dense_extract's order */,
                      esl_dense_obj_result* out);

/* ---- dominant planes and the ground from the dense map (additive part of ABI 5: detect by the symbol) -----------------------------------
 * esl_dense_objects and esl_relocalize take a world ground plane as an input; esl_extract_ground_plane finds one in ONE depth image.
 * The dense map holds the floor, the walls and the table tops as seen from every frame, deduplicated into voxels with exact integer
 * keys and counts.  esl_dense_planes reads them as planes: an exhaustive, totally ordered hypothesise-and-score search on the device
 * that peels one plane per round, in the manner of esl_relocalize and esl_init_quadrics_robust.  Integers and total orders decide
 * everything discrete, the few floating-point steps run in one stated order (planes are built on the host: one compiler decides every
 * bit), and the result is a function of the set of samples: any frame order, any split into esl_dense_add_frames calls and any run
 * give the same bytes.
 *  1. Eligible voxel.  A voxel of the map (dense-map steps 3 to 5) has its key k, count, label and votes.  It is eligible iff
 *     count >= min_count and, with skip_labelled != 0, it carries no label (votes == 0; on a map begun without labels no voxel carries
 *     one).  Centre x_a = ((double)k_a + 0.5) leaf.  n_eligible counts them; kmin_a, kmax_a over them give span = max_a (kmax_a -
 *     kmin_a + 1).
 *  2. Round r = 0, 1, ...: U_r = the eligible voxels not yet assigned, in ascending packed-key order, n_r its length.  n_r < 3 ends the
 *     search with stop_reason 1; such a round does not count as started.
 *  3. Hypothesis h = 0 .. n_hypotheses - 1 of round r: for k = 0, 1, 2, i_k = (mix >> 11) % n_r with mix = the splitmix64 finaliser
 *     (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31) of seed ^ (0x9E3779B97F4A7C15 *
 *     (uint64)(4 (r n_hypotheses + h) + k + 1)), everything mod 2^64.  With a, b, c the keys of the entries i_0, i_1, i_2 of U_r the
 *     hypothesis is INVALID iff two indices are equal; or one of the three pairwise Chebyshev key distances is < min_baseline; or,
 *     with N = (b - a) x (c - a) in int64 (exact) and N_a converted to double, norm = sqrt((N0 N0 + N1 N1) + N2 N2) is
 *     < 0.5 (min_baseline min_baseline) -- near-collinear triples.  Otherwise n^ = N / norm and d^ = -((n^0 x0 + n^1 x1) + n^2 x2), x
 *     the centre of a.
 *  4. Score over all of U_r: h(x) = (n^0 x0 + n^1 x1) + n^2 x2 + d^, no product contracted with a sum; inlier iff |h(x)| <= dist_tol;
 *     n_in = the inlier voxels, samples = the int64 sum of their counts.
 *  5. Winner: the valid hypothesis with the largest n_in, then the largest samples, then the smallest h.  None valid: stop_reason 2.
 *  6. Refinement (refine != 0).  Over the winner's inliers the int64 moments relative to kmin: n, s_a = sum d_a, M_ab = sum d_a d_b,
 *     d = k - kmin.  n span^2 >= 2^62 (tested in integers) skips the refit: refined = 3.  Otherwise m_a = s_a / n, C_ab = M_ab / n -
 *     m_a m_b; the eigenvector of C's smallest eigenvalue (ties to the lowest index) by a cyclic Jacobi -- 8 sweeps over the pivots
 *     (0,1), (0,2), (1,2); a zero pivot is skipped; theta = (C_qq - C_pp) / (2 C_pq), t = sign(theta) / (|theta| + sqrt(theta^2 +
 *     1)), c = 1 / sqrt(t^2 + 1), s = t c; columns, then rows of C, then the columns of V (p: c x_p - s x_q, q: s x_p + c x_q) --
 *     re-normalised by sqrt((v0 v0 + v1 v1) + v2 v2); xbar_a = ((double)kmin_a + m_a + 0.5) leaf, d^ = -((n^0 xbar0 + n^1 xbar1) +
 *     n^2 xbar2).  The refit is scored over U_r by step 4 and replaces the winner iff its (n_in, samples) is lexicographically not
 *     smaller: refined = 1; otherwise 2; 0 with refine == 0.
 *  7. The final plane's n_in < min_inliers ends the search with stop_reason 3: the plane is not reported, nothing is assigned.
 *     Otherwise its inliers are assigned plane index p = r and the next round starts; max_planes planes reported end the search with
 *     stop_reason 0.  rounds = the rounds started.
 *  8. planes_out row p: (n^, d^) negated when d^ < 0; with d^ == 0, when the first non-zero component of n^ is negative.  centroid_out:
 *     ((double)kmin_a + s_a / n + 0.5) leaf of the final inliers.  stats_out[8 p ..] = final inlier voxels, n_r of its round, valid
 *     hypotheses of its round, the winner h, the winner's inlier voxels before the refit, refined, 0, 0.  samples_out[p] = the inliers'
 *     sample sum.  voxel_plane_out[i] for the i-th voxel in esl_dense_extract's order, the first voxel_cap written: p assigned; -2
 *     eligible and unassigned; -1 not eligible.  hyp_out[(r n_hypotheses + h) 3 ..] = valid, n_in, samples of every hypothesis of
 *     every round started, the stopping round included (zero for an invalid hypothesis); the other rows are zero.
 *  9. Ground (up non-zero): up^ = up / sqrt((up0 up0 + up1 up1) + up2 up2).  Candidates: the reported planes (rows of planes_out) with
 *     |(n^0 up^0 + n^1 up^1) + n^2 up^2| >= up_min_cos.  ground_index = the candidate with the most inlier voxels, ties to the lowest
 *     p, or -1; ground_out = that plane negated when n^ . up^ < 0 -- the orientation the height gate of esl_dense_objects needs,
 *     whatever side of the floor the origin lies on -- or zero.  With up zero ground_index is -1. */
typedef struct {
  double   dist_tol;       /* 0.02 m: a voxel is an inlier of a plane when |height of its centre| <= dist_tol (PlaneRefinementComparator's 0.02) */
  double   up[3];          /* 0 0 0: no ground choice; otherwise the world's up direction, any length > 1e-12 */
  double   up_min_cos;     /* 0.7071067811865476: a ground candidate needs |n^ . up^| >= this (the reference's 45 degrees, PlaneExtractor.cpp:126-183) */
  int32_t  n_hypotheses;   /* 1024 per round; 1 .. 65536 */
  int32_t  max_planes;     /* 8; 1 .. 64 */
  int32_t  min_inliers;    /* 1000 voxels; >= 3 */
  int32_t  min_baseline;   /* 8: the three voxels of a hypothesis are pairwise at Chebyshev key distance >= this; >= 1 */
  int32_t  min_count;      /* 1: a voxel takes part only with count (samples) >= this */
  int32_t  skip_labelled;  /* 0; 1: voxels that carry an instance label (votes > 0) do not take part */
  int32_t  refine;         /* 1: least-squares re-fit over the winner's inliers, kept only when not worse */
  int32_t  pad;
  uint64_t seed;           /* 0 */
} esl_dense_plane_params;  /* 80 bytes; design choices, not values tuned on real data */
void esl_dense_plane_params_default(esl_dense_plane_params* p);

typedef struct { int32_t status, n_voxels, n_eligible, n_planes, n_assigned, ground_index, rounds, stop_reason; } esl_dense_plane_result; /* 32 bytes */

/* ESL_ERR_INVALID: null ctx, out or planes_out; a negative voxel_cap, or voxel_cap > 0 with voxel_plane_out NULL; a parameter outside
 * the ranges above; dist_tol not finite or <= 0; a non-finite up component, or an up that is neither zero nor longer than 1e-12;
 * up_min_cos outside [0, 1]; max_planes n_hypotheses >= 2^31.  ESL_ERR_STATE: no esl_dense_begin before.  A map over its capacity is
 * a result: ESL_OK, out->status = 3, n_voxels = -1, nothing else is written.  An empty map and a map without labels are valid.  The
 * call changes nothing in the map except the best words and the shared sorted list, which esl_dense_extract and esl_dense_objects
 * rebuild too: adds, extracts, object calls and plane calls may alternate.  Its buffers are slots of the dense map's own set
 * (grow-only, sized by the map and the parameters; a warm call of a shape no larger than an earlier one allocates nothing:
 * esl_debug_dense_allocs); one GPU, no collective, launches bracketed as kernel class 4. */
int esl_dense_planes(esl_ctx* ctx, const esl_dense_plane_params* p /* NULL = defaults */,
                     double* planes_out     /* max_planes x 4 world, unit normal, n_planes rows written, the others zero */,
                     double* centroid_out   /* max_planes x 3 or NULL */,
                     int32_t* stats_out     /* max_planes x 8 or NULL */,
                     int64_t* samples_out   /* max_planes or NULL */,
                     double ground_out[4]   /* or NULL */,
                     int64_t voxel_cap, int32_t* voxel_plane_out /* voxel_cap or NULL, in esl_dense_extract's order */,
                     int64_t* hyp_out       /* max_planes x n_hypotheses x 3 or NULL: valid, inlier voxels, inlier samples -- tests and tuning */,
                     esl_dense_plane_result* out);
/* the score kernel's layout: entries of U_r per LDS tile and hypotheses per workgroup (tests place list lengths around them) */
int esl_debug_dense_planes_layout(int32_t* tile_out, int32_t* group_out);

/* ---- viewing the dense map: per-pixel depth, colour, label and voxel from any pose, checked on depth (additive part of ABI 5: detect by the symbol) ---
 * The reference builds its dense map to show it (src/dense_builder, the Pangolin viewer).  esl_dense_render gives the dense map what
 * esl_render_map gives the ellipsoid map: every live voxel is splatted as a square of its leaf into every frame, the nearest voxel
 * wins each pixel, and against a measured depth image every won pixel is counted as agreeing, nearer or farther -- per frame (does the
 * map explain the images after a move?) and per voxel (which voxels do later frames see through?).  The call only counts: it does not
 * change the map.  Everything is FP64 and integers; every choice is a strict comparison or a total order and the only atomics are
 * integer atomics, so runs are bit-reproducible.
 *  1. Voxels.  The live voxels of the map in ascending packed-key order: the list, and the index i, that esl_dense_extract would give
 *     at this moment.  Each carries extract's xyz ((double)S_a / 2^30 / (double)count), count, bgr and inst (dense-map step 7).  A voxel
 *     with count < min_count is skipped in every frame; it counts in n_small, once per call.
 *  2. Camera point.  Poses are Tcw = (t, q); they are validated and turned into R on the host exactly as step 2 of the dense map does
 *     (an invalid pose gives ESL_ERR_INVALID before anything runs).  p_c[a] = ((R[a][0] p0 + R[a][1] p1) + R[a][2] p2) + t[a]; no product
 *     is contracted with a sum.  z = p_c[2].  The voxel is not drawn in this frame unless z >= depth_min && z <= depth_max (a NaN
 *     fails): such voxels count in the frame's n_depth_out.
 *  3. Footprint.  e = footprint leaf / 2, one double computed on the host.  With x = p_c[0]: u = (fx x) / z + cx, u0 = (fx (x - e)) / z +
 *     cx, u1 = (fx (x + e)) / z + cx; the same with fy, p_c[1], cy for v, v0, v1: multiply, then divide, then add.  If any of the six is
 *     not finite or exceeds 2^30 in magnitude the voxel counts in the frame's n_outside (the values are compared as doubles, never
 *     converted).  col = floor(u + 0.5), c0 = min(col, ceil(u0)), c1 = max(col, floor(u1)): the pixels whose centre lies inside the
 *     projected square, and always the pixel nearest the centroid.  Then c0 = max(c0, col - max_radius), c1 = min(c1, col +
 *     max_radius), then both are clipped to [0, cols - 1]; rows alike.  An empty range on either axis counts in n_outside; otherwise
 *     the voxel counts in n_drawn.
 *  4. Pixel.  zq = llrint(z 2^20) (depth_max <= 4095 keeps zq < 2^32).  Every pixel of the footprint receives the candidate
 *     zq << 32 | i and keeps the smallest: the nearest voxel, ties to the lowest index.  The stored depth is the winner's own z, not zq.
 *  5. Images.  depth_out = the winner's z, voxel_out = i, bgr_out / inst_out = the winner's colour and label as esl_dense_extract
 *     reports them (0 / -1 on a map without colour / labels).  A pixel without a winner gets NaN, -1, 0, -1.
 *  6. Depth comparison at every pixel with a winner: step 6 of esl_render_map word for word (no data, agree, nearer, farther, with this
 *     call's depth_scale, depth_min, depth_max and depth_tol).  frame_out[8 f ..] = n_drawn, n_depth_out, n_outside, covered (the pixels
 *     with a winner), agree, nearer, farther, no data; the last four sum to covered and are 0 without depth_meas.  vox_out[4 i ..] =
 *     won (the pixels voxel i wins), agree, nearer, farther, summed over the call's frames, for the first vox_cap voxels; the last
 *     three are 0 without depth_meas.
 *  7. Memory.  The candidates of a chunk of frames live in a buffer of at most zbuf_bytes: the frames are processed in chunks of
 *     max(1, floor(zbuf_bytes / (8 rows cols))), n_chunks = ceil(F / that).  No result depends on the chunking.
 *  8. Map status.  On a map whose status is not 0 the call returns ESL_OK, the result reports that status and n_voxels = -1, and
 *     nothing else is written -- as esl_dense_extract, esl_dense_objects and esl_dense_planes do. */
typedef struct {
  double  depth_scale;  /* 5000: raw units per metre of depth_meas; finite, > 0 */
  double  depth_min;    /* 0.1: the gate of a voxel's z (step 2) and of a measured sample (step 6); finite, >= 0 */
  double  depth_max;    /* 6.0: finite, >= depth_min, <= 4095 */
  double  depth_tol;    /* 0.05 m: |z_meas - z| <= depth_tol agrees; finite, >= 0 */
  double  footprint;    /* 1.0: the side of a voxel's square in leaves; 0 = the nearest pixel only; finite, >= 0 */
  int32_t max_radius;   /* 8: a footprint reaches at most this many pixels from its centre pixel; 0 .. 64 */
  int32_t min_count;    /* 1: voxels with fewer samples are not drawn; >= 1 */
  int64_t zbuf_bytes;   /* 268435456: the most the per-pixel candidates of one chunk of frames may take; >= 8 rows cols */
} esl_dense_render_params;   /* 56 bytes; design choices, not values tuned on real data */
void esl_dense_render_params_default(esl_dense_render_params* p);

typedef struct { int32_t status, n_voxels, n_small, n_chunks; } esl_dense_render_result; /* 16 bytes */

/* ESL_ERR_INVALID: null ctx, K or out; negative F or vox_cap, vox_cap > 0 with vox_out NULL; rows or cols < 1 or > 16384; fx or fy not
 * finite or <= 0; depth_scale not finite or <= 0; depth_min, depth_max or depth_tol not finite or negative; depth_min > depth_max;
 * depth_max > 4095; footprint not finite or < 0; max_radius < 0 or > 64; min_count < 1; zbuf_bytes < 8 rows cols; an invalid pose
 * (step 2); F differing from the resident graph's n_cams when cams == NULL.  The comparison counts of frame_out and vox_out are always
 * written (zero without depth_meas), so no output needs depth_meas.  ESL_ERR_STATE: no esl_dense_begin before; cams == NULL without a
 * resident graph and states.  F = 0, an empty map and all outputs NULL are valid.  An output that is not asked for is neither computed
 * nor allocated.  The call changes nothing in the map except the best words and the shared sorted list, which the extracting calls
 * rebuild too.  Its buffers are a set of its own beside the dense map's (grow-only; a warm call of the same shape allocates nothing:
 * esl_debug_dense_allocs counts them; at most zbuf_bytes + a chunk's images + 40 bytes per voxel); one GPU, no collective, launches
 * bracketed as kernel class 4. */
int esl_dense_render(esl_ctx* ctx,
                     const double* cams /* F x 7 Tcw, NULL = resident camera states (F must equal n_cams) */, int32_t F,
                     const double K[4], int32_t rows, int32_t cols,
                     const uint16_t* depth_meas /* F x rows x cols or NULL */, const esl_dense_render_params* p /* NULL = defaults */,
                     double* depth_out  /* F x rows x cols or NULL: z of the winning voxel, NaN where none */,
                     int32_t* voxel_out /* F x rows x cols or NULL: its index in esl_dense_extract's order, -1 where none */,
                     uint8_t* bgr_out   /* F x rows x cols x 3 or NULL: its colour, 0 where none */,
                     int32_t* inst_out  /* F x rows x cols or NULL: its label, -1 where none */,
                     int32_t* frame_out /* F x 8 or NULL: n_drawn, n_depth_out, n_outside, covered, agree, nearer, farther, no data */,
                     int64_t vox_cap, int32_t* vox_out /* vox_cap x 4 or NULL: won, agree, nearer, farther; the first min(vox_cap, n_voxels) rows written */,
                     esl_dense_render_result* out);

/* ---- normals of the dense map (additive part of ABI 5: detect by the symbol) -------------------------------------------------------------
 * Per live voxel, in esl_dense_extract's order: a unit normal, a curvature, a neighbour count and a valid flag, from the centroids of
 * the voxel's neighbourhood.  For shading, meshing and plane patches, and what esl_dense_align_frames matches against.  The call reads
 * the map and does not change it.  FP64 and integers; one voxel's sums are taken in one fixed order, so runs are bit-reproducible.
 *  N1. Eligibility.  A voxel is eligible when it is live (dense-map step 9) and count >= min_count.  A live voxel that is not eligible
 *      reports a zero normal, a NaN curvature, 0 neighbours and valid = 0.
 *  N2. Neighbours.  The neighbours of an eligible voxel i are the eligible voxels among the (2 radius + 1)^3 keys around its key whose
 *      components lie within +-(2^20 - 1), itself included; they are visited in ascending packed-key order.  A dead slot is no
 *      neighbour (dense-map step 10).
 *  N3. Moments.  c = the centroid of step 7 ((double)S_a / 2^30 / (double)count).  d_j = c_j - c_i; m = the number of neighbours;
 *      s = the sum of d_j; M = the sum of d_j d_j^T as six entries xx, xy, xz, yy, yz, zz: all summed in visit order from 0, one product
 *      and one add at a time.  u = s / m; C_ab = M_ab / m - u_a u_b; trace C = (C_xx + C_yy) + C_zz.
 *  N4. Normal.  n = the eigenvector of the smallest eigenvalue of C by the cyclic Jacobi of esl_dense_planes' step 6 (8 sweeps over the
 *      pivots (0,1), (0,2), (1,2); ties to the lowest index; re-normalised), turned so that its first non-zero component is positive.
 *      lambda = n . (C n), each row of C n and the final product summed left to right; curvature = lambda / trace C.
 *  N5. Validity.  valid = m >= min_neighbors and trace C > 0 and curvature <= max_curvature (the Jacobi runs only when the first two
 *      hold).  An invalid voxel reports a zero normal, a NaN curvature and its m. */
typedef struct {
  double  max_curvature;  /* 0.05: lambda / trace above this (an edge, a corner, noise) is no surface; finite, >= 0 */
  int32_t radius;         /* 1: the neighbourhood reaches this many keys on every axis; 1 or 2 */
  int32_t min_count;      /* 1: voxels with fewer samples are neither given a normal nor counted as neighbours; >= 1 */
  int32_t min_neighbors;  /* 5: fewer neighbours (the voxel included) give no normal; >= 1 */
} esl_dense_normal_params;   /* 24 bytes; design choices, not values tuned on real data */
void esl_dense_normal_params_default(esl_dense_normal_params* p);

typedef struct { int32_t status, n_voxels, n_eligible, n_valid; } esl_dense_normal_result; /* 16 bytes */

/* ESL_ERR_INVALID: null ctx or out; negative cap; max_curvature not finite or negative; radius outside 1 .. 2; min_count < 1;
 * min_neighbors < 1.  ESL_ERR_STATE: no esl_dense_begin before.  The first min(cap, n_voxels) rows of every non-NULL output are written;
 * n_voxels reports all.  On a map whose status is not 0 the call returns ESL_OK, the result reports that status and n_voxels = -1, and
 * nothing else is written.  The buffers are a set of its own beside the dense map's, shared with esl_dense_align_frames (grow-only; a
 * warm call allocates nothing: esl_debug_dense_allocs counts them; 61 bytes per voxel and 4 per table slot); one GPU, no collective,
 * launches bracketed as kernel class 4. */
int esl_dense_normals(esl_ctx* ctx, const esl_dense_normal_params* p /* NULL = defaults */, int64_t cap,
                      double* normal_out /* cap x 3 or NULL */, double* curvature_out /* cap or NULL */,
                      int32_t* neighbors_out /* cap or NULL */, uint8_t* valid_out /* cap or NULL */, esl_dense_normal_result* out);

/* ---- aligning frames to the dense map: frame-to-model pose refinement (additive part of ABI 5: detect by the symbol) -------------------
 * Given depth frames and pose guesses, find the poses at which the frames lie on the map: point-to-plane Gauss-Newton against the
 * voxel centroids and their normals (steps N1 to N5, recomputed at the start of every call).  The step between esl_dense_render (does
 * the map explain the image?) and esl_dense_move_frames (apply a new pose).  H of the last pass is the information matrix of the pose
 * up to the residual's variance: a caller can put it into the graph as a prior.  The call reads the map and does not change it.  FP64
 * and integers; every reduction over samples is an integer sum, so the call is bit-reproducible and a frame's result does not depend
 * on the other frames of the call or on their order.  Per frame and per pass it = 0 .. iters (the last pass only evaluates):
 *  a. Samples are formed by dense-map steps 1 to 3, exactly as esl_dense_add_frames forms them, with the map's own esl_dense_params but
 *     this call's stride.  n_sampled, n_zero, n_depth_out, n_key_out and n_used mean what they mean there.
 *  b. Match.  Candidates are the valid voxels (step N5) among the (2 reach + 1)^3 keys around the sample's key whose components lie
 *     within +-(2^20 - 1).  d2 = ((p_w - c)_x^2 + (p_w - c)_y^2) + (p_w - c)_z^2.  The match is the candidate with the smallest d2, ties
 *     to the smallest packed key.  No candidate counts in n_nomatch; d2 > max_dist^2 counts in n_far (max_dist = 0 means (reach + 1)
 *     leaf; the square is one double computed on the host); the rest count in n_inlier.
 *  c. Terms of an inlier.  o = R^T (0 - t), the camera centre (step 2 of the dense map at p_c = 0); q = p_w - o; r = p_w - c;
 *     e = (n_x r_x + n_y r_y) + n_z r_z; J = (n, q x n) with (q x n)_x = q_y n_z - q_z n_y and so on.  The increment delta = (v, omega)
 *     moves the centre by v and turns the frame about its centre by omega, in world axes: e changes by J . delta.  The 21 products
 *     J_a J_b (a <= b, row after row), the 6 products J_a e and e^2 are each added as llrint(x 2^30) into an int64, the inlier count
 *     beside them.  These 29 integers and the eight counts of steps a and b are the pass's row of 37 words.  Before anything runs:
 *     Q = max(1, max_dist, depth_max sqrt(1 + X^2 + Y^2)) (1 + 2^-20), X = max(|cx|, |cols - 1 - cx|) / fx, Y alike, bounds |q|, |J_a| and
 *     |e|; a call with (sampled pixels of a frame) (Q^2 2^30 + 1) >= 2^62 returns ESL_ERR_INVALID.
 *  d. Step (host).  H_ab and g_a are the sums as doubles divided by 2^30.  If n_inlier < min_inliers the frame stops as too few.
 *     A = H with A_aa = H_aa + damping H_aa; A = L L^T by Cholesky, every sum taken term after term; a pivot that is not > 0 or is below
 *     min_pivot_ratio times the largest A_aa stops the frame as degenerate (a camera that sees one wall slides along it).  A stopped
 *     frame keeps the pose this pass started from, and this pass is its evaluation.  Otherwise L L^T delta = -g; the quaternion is
 *     divided by its norm as step 2 divides it; dq = (omega / 2, 1) divided by its norm; q_new = q (x) conj(dq) (Hamilton product);
 *     o_new = o + v; t_new = -(R_new o_new) with R_new by step 2's formula.  No sine or cosine anywhere.  |v| <= tol_t and
 *     |omega| <= tol_r stops the frame as converged: one more pass evaluates it at its new pose.  A frame that has stopped is skipped
 *     by the later passes.
 *  e. Outputs.  cams_out = the final poses.  frames_out: status (0 all iters taken, 1 converged, 2 too few, 3 degenerate), the steps
 *     taken, the eight counts, sum_e2 = (the e^2 sum) / 2^30 and H of the frame's last pass, which is at its final pose, and |v|, |omega| of
 *     its last step.  iter_out: per frame and pass the row of 37 words (zero for a pass the frame skipped).  On a map whose status is
 *     not 0 the call returns ESL_OK, the result reports that status and n_voxels = -1, and nothing else is written. */
typedef struct {
  double  max_dist;         /* 0 = (reach + 1) leaf: a match farther than this is no inlier; finite, >= 0 */
  double  damping;          /* 0: Levenberg's lambda on diag H; finite, >= 0 */
  double  min_pivot_ratio;  /* 1e-6: a Cholesky pivot below this times the largest diagonal entry = degenerate; finite, >= 0 */
  double  tol_t;            /* 1e-5 m; finite, >= 0 */
  double  tol_r;            /* 1e-5 rad; finite, >= 0 */
  int32_t iters;            /* 4: Gauss-Newton steps at most; 0 .. 64 (0 only evaluates) */
  int32_t stride;           /* 2: every stride-th row and column from 0; >= 1 */
  int32_t reach;            /* 1: the match is sought this many keys around the sample's; 0 .. 2 */
  int32_t min_inliers;      /* 100; >= 1 */
  esl_dense_normal_params normals;   /* steps N1 to N5 */
} esl_dense_align_params;   /* 80 bytes; design choices, not values tuned on real data */
void esl_dense_align_params_default(esl_dense_align_params* p);

typedef struct {
  int32_t status, iters;
  int64_t n_sampled, n_zero, n_depth_out, n_key_out, n_used, n_nomatch, n_far, n_inlier;
  double  sum_e2, H[36], step_t, step_r;
} esl_dense_align_frame;    /* 384 bytes */
typedef struct { int32_t status, n_voxels, n_valid, n_passes; } esl_dense_align_result; /* 16 bytes */

/* Errors follow esl_dense_add_frames, case by case: ESL_ERR_STATE: no esl_dense_begin before; cams == NULL without a resident graph
 * and states.  ESL_ERR_INVALID: null ctx, K, depth (with F > 0) or out; negative F; rows or cols < 1 or > 16384; fx or fy not finite or
 * <= 0; an invalid pose (step 2); F differing from the resident graph's n_cams when cams == NULL; (sampled pixels of a frame) F reaching
 * 2^31; a parameter outside the range its comment names; the bound of step c.  bgr and inst are not asked for.  F = 0 is valid.  The
 * buffers are esl_dense_normals' set (a warm call of the same shape allocates nothing; 2 bytes per pixel, 296 per frame and pass
 * beside the normals'); per pass the host uploads 12 doubles and a flag per frame and reads back 37 words per frame; one GPU, no
 * collective, launches bracketed as kernel class 4. */
int esl_dense_align_frames(esl_ctx* ctx, const double* cams /* F x 7 Tcw, the start poses; NULL = resident camera states */, int32_t F,
                           const double K[4], int32_t rows, int32_t cols, const uint16_t* depth /* F x rows x cols */,
                           const esl_dense_align_params* p /* NULL = defaults */, double* cams_out /* F x 7 or NULL */,
                           esl_dense_align_frame* frames_out /* F or NULL */,
                           int64_t* iter_out /* F x (iters + 1) x 37 or NULL */, esl_dense_align_result* out);

/* ---- carving the dense map: drop the voxels that later frames see through (additive part of ABI 5: detect by the symbol) -----------------
 * An object that stood in some frames and was moved stays in the dense map as a ghost: esl_dense_objects fits it, esl_dense_align_frames
 * matches against it, esl_dense_render draws it.  esl_dense_carve_frames is the classical space-carving test per (voxel, frame): project
 * the voxel into an observer frame, read the measured depth around that pixel, ask whether the camera saw past the voxel.  The map stays
 * a function of the multiset of its samples (dense-map step 8 and what follows it): the call never clears a record.  It decides which
 * voxels are seen through, finds the pixels of the OWNER frames whose samples lie in those voxels, hands back the owners' depth images
 * without them and, when asked, removes exactly those samples by dense-map step 8.  Everything is FP64 and integers; every choice is a
 * comparison and every sum an integer sum, so runs are bit-reproducible in any frame order and any split of the observers over calls.
 *  C1. Voxels.  The live voxels of the map in ascending packed-key order: the list, the index i and the xyz that esl_dense_extract
 *      would give at the moment of the call.
 *  C2. Observation of voxel i in observer frame f.  Poses are validated and turned into R, t on the host as dense-map step 2 does.
 *      p_c as step 2 of esl_dense_render; z = p_c[2] must pass z >= depth_min && z <= depth_max (a NaN fails), else the pair counts in
 *      the frame's depth out.  u = (fx p_c[0]) / z + cx, v = (fy p_c[1]) / z + cy: multiply, then divide, then add.  If u or v is not
 *      finite or exceeds 2^30 in magnitude the pair counts in the frame's outside.  col = floor(u + 0.5), row = floor(v + 0.5), compared
 *      as doubles; the centre pixel must lie in the image (0 <= col <= cols - 1, 0 <= row <= rows - 1), else outside.  Otherwise the
 *      pair is in view.  The window is [col - window, col + window] x [row - window, row + window] clipped to the image.  Every pixel of
 *      the window is classed against z by step 6 of esl_render_map word for word (agree, nearer, farther, no data) with this call's
 *      depth_scale, depth_min, depth_max and depth_tol.  The observation's class: agree if any pixel agrees; else nearer if any is
 *      nearer (something stands in front: the voxel is occluded); else through if any is farther; else no data.  Exactly one class per
 *      pair in view.
 *  C3. Counts.  vox_out[4 i ..] = agree, nearer, through, no data of voxel i, summed over the observers.  obs_out[8 f ..] = in view,
 *      depth out, outside, agree, nearer, through, no data, 0 of frame f, summed over the voxels.  All integer sums.
 *  C4. Verdict.  Voxel i is carved iff through >= min_through and through >= through_per_agree agree (the product as a 64-bit
 *      integer).  n_tested = the voxels with agree + nearer + through > 0.  A voxel's verdict depends on that voxel and the observers
 *      alone, never on another voxel.
 *  C5. Owners' samples.  Every owner frame's samples are formed by dense-map steps 1 to 3 exactly as esl_dense_add_frames forms them:
 *      the map's own esl_dense_params and stride, cams_own and depth_own.  A used sample whose key has a live voxel counts in the
 *      frame's found, one without in its not found; own_out[4 f ..] = used, found, carved, not found.  A found sample whose voxel is
 *      carved is carved: mask_out = 1 and depth_kept_out = 0 at its pixel.  Every other pixel keeps its raw value and mask 0: unsampled
 *      pixels, zero, out of range, not found, not carved.
 *  C6. Apply.  With apply = 1 the call then performs dense-map step 8 on the owner frames with depth images that hold the raw value at
 *      the carved pixels and 0 elsewhere, and bgr_own / inst_own as given; its result goes to `removed`.  The map is then the map of
 *      esl_dense_begin plus one add of the owners with depth_kept_out, plus whatever other frames it held: the same bytes in extract,
 *      objects, planes and info; only esl_dense_slots_get differs (the carved voxels' slots are dead until a purge).  A later
 *      esl_dense_remove_frames / _move_frames of an owner takes its kept image.  vox_out / carved_out refer to the list before the
 *      removal.  With apply = 0 the map is untouched but for the best words and the shared sorted list, as with every extracting call,
 *      and `removed` is zero.
 *  C7. Map status.  On a map whose status is not 0 the call returns ESL_OK, the result reports that status and n_voxels = -1, and
 *      nothing else is written.
 * Limits: window <= 4; rows, cols <= 16384; every count is an int32; F_obs <= 65535 (a voxel's four counts are accumulated as four
 * 16-bit fields of one 64-bit word).  Not part of this call: carving by rendered visibility, a TSDF, a purge after the removal
 * (esl_dense_purge), images kept on the device between calls, more than one GPU. */
typedef struct {
  double  depth_scale;        /* 5000: raw units per metre of depth_obs; finite, > 0 */
  double  depth_min;          /* 0.1: the gate of a voxel's z and of a measured sample (step C2); finite, >= 0 */
  double  depth_max;          /* 6.0: finite, >= depth_min, <= 4095 */
  double  depth_tol;          /* 0.05 m: |z_meas - z| <= depth_tol agrees; finite, >= 0 */
  int32_t window;             /* 1: the pixels read around the centre pixel reach this far; 0 .. 4 */
  int32_t min_through;        /* 2: a carved voxel was seen through at least this often; >= 1 */
  int32_t through_per_agree;  /* 1: and at least this many times per agreeing observation; >= 0 */
  int32_t apply;              /* 0: 1 = remove the carved samples from the map (step C6); 0 or 1 */
} esl_dense_carve_params;   /* 48 bytes; design choices, not values tuned on real data */
void esl_dense_carve_params_default(esl_dense_carve_params* p);

typedef struct {
  int32_t status, n_voxels, n_tested, n_carved;
  int64_t samples_found, samples_carved;   /* summed over the owner frames */
  esl_dense_remove_result removed;          /* step C6; zeros when apply = 0 */
} esl_dense_carve_result;   /* 96 bytes */

/* Errors follow esl_dense_render and esl_dense_remove_frames, case by case and in this order.  ESL_ERR_INVALID: null ctx or out;
 * negative F_obs or F_own; null K; rows or cols < 1 or > 16384; fx or fy not finite or <= 0; negative vox_cap; depth_scale not finite or
 * <= 0; depth_min, depth_max or depth_tol not finite or negative; depth_min > depth_max; depth_max > 4095; window outside 0 .. 4;
 * min_through < 1; through_per_agree < 0; apply not 0 or 1; F_obs > 65535; null depth_obs with F_obs > 0; null cams_own or depth_own
 * with F_own > 0.  ESL_ERR_STATE: no esl_dense_begin before; with apply = 1 and F_own > 0, bgr_own or inst_own NULL when esl_dense_begin
 * asked for them; cams_obs == NULL without a resident graph and states.  ESL_ERR_INVALID again: F_obs differing from the resident
 * graph's n_cams when cams_obs == NULL; an invalid pose among the observers, then among the owners; the owners' sampled pixels reaching
 * 2^31.  A refused call changes nothing.  F_obs = 0, F_own = 0 and an empty map are valid; any output may be NULL (vox_out and
 * carved_out receive the first min(vox_cap, n_voxels) rows).  Its buffers are a set of its own beside the dense map's (grow-only; a warm
 * call of the same shape allocates nothing: esl_debug_dense_allocs counts them; 2 bytes per observer pixel, 2 per owner pixel, 1 more with
 * mask_out and 2 more with apply = 1, 49 per voxel, 1 per table slot); with apply = 1 the carved-depth images travel to the host and back through
 * esl_dense_remove_frames' own upload.  One GPU, no collective, launches bracketed as kernel class 4. */
int esl_dense_carve_frames(esl_ctx* ctx,
                           const double* cams_obs /* F_obs x 7 Tcw, the frames that vote; NULL = resident camera states */, int32_t F_obs,
                           const uint16_t* depth_obs /* F_obs x rows x cols */,
                           const double* cams_own /* F_own x 7: frames that are in the map, with the poses they were added with */, int32_t F_own,
                           const uint16_t* depth_own /* F_own x rows x cols, as added */,
                           const uint8_t* bgr_own /* F_own x rows x cols x 3 or NULL */, const int32_t* inst_own /* F_own x rows x cols or NULL */,
                           const double K[4], int32_t rows, int32_t cols, const esl_dense_carve_params* p /* NULL = defaults */,
                           int64_t vox_cap, int32_t* vox_out /* vox_cap x 4 or NULL: agree, nearer, through, no data */,
                           uint8_t* carved_out /* vox_cap or NULL */,
                           int32_t* obs_out /* F_obs x 8 or NULL: in view, depth out, outside, agree, nearer, through, no data, 0 */,
                           uint16_t* depth_kept_out /* F_own x rows x cols or NULL */,
                           uint8_t* mask_out /* F_own x rows x cols or NULL: 1 = carved sample */,
                           int32_t* own_out /* F_own x 4 or NULL: used, found, carved, not found */,
                           esl_dense_carve_result* out);

/* ---- covisibility of the dense map: which frames see the same voxels, which frames are redundant (additive part of ABI 5: detect by
 * the symbol) -----------------------------------------------------------------------------------------------------------------------------
 * Frames a and b are covisible in the voxels of the map that both of them see, and "sees" is the class agree of step C2 of the carving.
 * esl_dense_covis_frames gives, for F frames with their measured depth: per voxel the number of frames that see it, per pair of frames
 * the number of voxels both see (the covisibility graph's weights: candidates for loop-closure edges, observers and owners of a
 * carving), and the keyframe-culling rule of feature-based SLAM on the map's voxels: a frame is redundant when a given fraction of
 * what it sees is seen by at least min_others other frames; redundant frames leave one by one, the counts following.  The call reads the
 * map as esl_dense_carve_frames with apply = 0 does.  Everything is integers after step V2; every choice is a comparison and every sum
 * an integer sum, so runs are bit-reproducible and a permutation of the frames permutes the outputs.
 *  V1. Voxels.  As step C1: the live voxels in ascending packed-key order, index i, xyz as esl_dense_extract gives them.
 *  V2. Sees.  Frame f sees voxel i iff step C2 of the carving gives the class agree, with this call's depth_scale, depth_min, depth_max,
 *      depth_tol and window.  Poses are validated and turned into R, t on the host as dense-map step 2 does.
 *  V3. Counts.  vox_out[i] = k_i, the number of frames that see voxel i.  frame_out[8 f ..] = in view, depth out, outside, seen,
 *      covered, unique, cull round, 0 of frame f: seen_f = the voxels f sees, unique_f = those of them with k_i = 1, the first three
 *      as in obs_out of the carving.
 *  V4. Pairs.  pair_out[a F + b] = the number of voxels that a and b both see, as int32: symmetric, its diagonal is seen_a.
 *  V5. Covered and redundant.  A voxel that f sees is covered without f iff k_i - 1 >= min_others; covered_f counts such voxels among
 *      the voxels f sees.  f is redundant iff seen_f >= 1 and covered_f cover_den >= cover_num seen_f, both products as 64-bit integers.
 *  V6. Cull rounds r = 0 .. max_cull - 1; the alive frames start as all frames.  k_i^r counts alive frames only and covered_f^r
 *      follows from k_i^r as in V5.  The candidates are the alive frames with keep_in[f] == 0 that are redundant under k^r (a protected
 *      frame still counts as an observer).  The candidate with the smallest seen_f - covered_f^r, ties to the lowest f, leaves the alive
 *      set: its cull round is r.  The rounds stop when there is no candidate; a frame never culled has round -1.  frame_out's covered
 *      column and vox_out are the values of round 0; pair_out always covers all F frames.  n_culled = the rounds done; with
 *      max_cull = 0 nothing is culled.
 *  V7. Map status.  As C7: on a map whose status is not 0 the call returns ESL_OK, sets that status and n_voxels = -1 and writes
 *      nothing else.
 * Limits: F <= 4096 (pair_out is at most 64 MiB); window <= 4; rows, cols <= 16384; every count is an int32.  Not part of this call:
 * emitting graph edges, aligning or removing frames on the result, weights other than voxel counts, bits kept on the device between
 * calls, more than one GPU. */
typedef struct {
  double  depth_scale;        /* 5000: raw units per metre of depth; finite, > 0 */
  double  depth_min;          /* 0.1: the gate of a voxel's z and of a measured sample (step C2); finite, >= 0 */
  double  depth_max;          /* 6.0: finite, >= depth_min, <= 4095 */
  double  depth_tol;          /* 0.05 m: |z_meas - z| <= depth_tol agrees; finite, >= 0 */
  int32_t window;             /* 1: the pixels read around the centre pixel reach this far; 0 .. 4 */
  int32_t min_others;         /* 3: a voxel is covered without f when this many other frames see it; >= 1 */
  int32_t cover_num;          /* 9: f is redundant when covered_f / seen_f >= cover_num / cover_den; 0 .. cover_den */
  int32_t cover_den;          /* 10: 1 .. 2^20 */
  int32_t max_cull;           /* 0: the cull rounds of step V6 at most; >= 0 */
  int32_t reserved;           /* 0 */
} esl_dense_covis_params;   /* 56 bytes; design choices, not values tuned on real data */
void esl_dense_covis_params_default(esl_dense_covis_params* p);

typedef struct {
  int32_t status, n_voxels, n_seen, n_culled;   /* n_seen: the voxels with k_i >= 1 */
  int64_t sum_seen;                             /* the sum of seen_f over the frames = the sum of k_i over the voxels */
  int64_t sum_pairs;                            /* the sum of pair[a][b] over a < b = the sum of k_i (k_i - 1) / 2 over the voxels,
                                                 * which is how it is formed: it is there without pair_out too */
} esl_dense_covis_result;   /* 32 bytes */

/* Errors follow esl_dense_carve_frames, case by case and in this order.  ESL_ERR_INVALID: null ctx or out; negative F; null K; rows or
 * cols < 1 or > 16384; fx or fy not finite or <= 0; negative vox_cap; depth_scale not finite or <= 0; depth_min, depth_max or depth_tol
 * not finite or negative; depth_min > depth_max; depth_max > 4095; window outside 0 .. 4; min_others < 1; cover_den outside 1 .. 2^20;
 * cover_num outside 0 .. cover_den; negative max_cull; reserved not 0; F > 4096; null depth with F > 0.  ESL_ERR_STATE: no
 * esl_dense_begin before; cams == NULL without a resident graph and states.  ESL_ERR_INVALID again: F differing from the resident
 * graph's n_cams when cams == NULL; an invalid pose.  A refused call changes nothing.  F = 0 and an empty map are valid; any output but
 * `out` may be NULL (vox_out receives the first min(vox_cap, n_voxels) values; without pair_out the pair counts are not formed).  Its
 * buffers are a set of its own beside the dense map's (grow-only; a warm call of the same shape allocates nothing:
 * esl_debug_dense_allocs counts them; 2 bytes per pixel, 8 F ceil(n / 64) for the bits, 28 per voxel and a quarter more for two
 * masks, 4 F F with pair_out, 136 per frame).  Per cull round the host reads back F int32 and launches two kernels.  One GPU, no
 * collective, launches bracketed as kernel class 4. */
int esl_dense_covis_frames(esl_ctx* ctx, const double* cams /* F x 7 Tcw; NULL = resident camera states */, int32_t F,
                           const uint16_t* depth /* F x rows x cols */, const uint8_t* keep_in /* F or NULL: != 0 protects a frame */,
                           const double K[4], int32_t rows, int32_t cols, const esl_dense_covis_params* p /* NULL = defaults */,
                           int64_t vox_cap, int32_t* vox_out /* vox_cap or NULL: k_i */,
                           int32_t* frame_out /* F x 8 or NULL: in view, depth out, outside, seen, covered, unique, cull round, 0 */,
                           int32_t* pair_out /* F x F or NULL */, esl_dense_covis_result* out);

/* ---- diagnostics ---------------------------------------------------------------------------------*/
/* Dense FP64-MFMA Cholesky factor + solve (the reduced-camera solver of SLAM mode) on a procedurally generated,
 * strictly diagonally dominant n x n system; returns the time of factor + solve (HIP events) and |A x - b| / |b|.
 * A known-answer test of the solver and the micro-benchmark behind the "mfma" roofline numbers. */
int esl_selftest_cholesky(esl_ctx* ctx, int32_t n, double* ms_out, double* rel_residual_out);
/* test / debug (additive part of ABI 5: detect by the symbol): how many device allocations the map-side calls of one owner have made
 * on this context so far and how many bytes the owner's grow-only buffers hold -- a warm call of a shape no larger than an earlier
 * one changes neither.  Zeros for an owner that has not run yet; ESL_ERR_INVALID for an unknown owner or a null pointer.  Host code only. */
typedef enum {
  ESL_SCRATCH_RELOC = 0,        /* esl_reloc_set_map, esl_relocalize */
  ESL_SCRATCH_ASSOC = 1,        /* esl_predict_boxes, esl_associate_boxes */
  ESL_SCRATCH_MERGE = 2,        /* esl_map_overlaps, esl_map_merge */
  ESL_SCRATCH_RENDER = 3,       /* esl_render_map */
  ESL_SCRATCH_INIT_BATCH = 4,   /* esl_init_quadrics (the robust call's refit included) */
  ESL_SCRATCH_INIT_ROBUST = 5   /* esl_init_quadrics_robust's own buffers */
} esl_scratch_owner;
int esl_debug_scratch_allocs(esl_ctx* ctx, int32_t owner, int64_t* allocs_out, int64_t* bytes_out);
/* = esl_debug_scratch_allocs(ctx, ESL_SCRATCH_RENDER, ...) */
int esl_debug_render_allocs(esl_ctx* ctx, int64_t* allocs_out, int64_t* bytes_out);
/* test / debug: the static task list of the persistent dense factorisation for an order-n system (outer panels of W 128-panels,
 * `filler` far-update tasks between the chain-dependent groups): 4 int32 per task {type, a, b, c} -- 0: S(panel a, strip b),
 * 1: u(panel a, row tile b, column tile c), 2: U(outer panel a, row tile b, column tile c), 3: one 128 x 64 QUARTER of a rank-128 update
 * u (c = column tile | quarter << 16: the diagonal tiles' updates run as quarters) --, ns[np][nR] = strips of row tile R that
 * panel k solves, meta = {np, n_outer, nR, n_tasks, W}.  Host code only (no device needed), but the list depends on the environment:
 * ESL_CHOL_FUSE=0 puts strips 0, 1 of every panel and the diagonal halves of the quarter tasks back on the list (the chain does
 * them itself by default).  Call with null buffers for the sizes. */
int esl_debug_chol_plan(int32_t n, int32_t W, int32_t filler, int32_t* tasks_out, int64_t cap_tasks, int32_t* ns_out, int64_t cap_ns, int32_t meta_out[5]);
/* test / debug: would the rank-K update of rows [base, rows) x columns [base, col_limit) of a matrix with leading dimension lda
 * (ext != 0: the operand is external, leading dimension ldp) run on the 128 x 128 tile kernel -- the one whose assign form lets the
 * camera-first trial run the segments' products beside the update?  Host code only; ESL_UPD_V=0 answers no everywhere. */
int esl_debug_update_v_applies(int64_t lda, int64_t rows, int64_t base, int64_t col_limit, int32_t ext, int64_t ldp, int32_t* applies_out);
/* test / debug: the camera segment length (16, 32 or 48) the camera-first trial's layout chooses for its one-sided assembly of T when
 * ESL_CF_STRIDE is unset, from a graph's counts with segments of one, two and three chunks of 16 cameras: flops the separators' rank-K
 * update executes, entry-products of the assembly, elements of the segments' slabs.  n_o = order of the reduced system (16 below
 * 8,192).  ms_out (may be null): the cost model's milliseconds per trial for the three.  Host code only: the rule, like every other
 * decision of that layout, is in csrc/esl_cf_plan.hpp (cf_stride_choose, cf_plan_build), which tests/cf_plan_main.cpp prints on the CPU. */
int esl_debug_cf_stride_choose(int64_t n_o, const double upd_flops[3], const double pairs[3], const double slab[3], int32_t* stride_out, double ms_out[3]);

#ifdef __cplusplus
}
#endif
#endif /* ESL_H_ */
