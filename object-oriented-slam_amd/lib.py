"""ctypes binding of csrc/libesl_hip.so (the C-ABI of include/esl.h).

The library is the product: if it is missing or no HIP device is usable, everything here raises —
there is no CPU fallback (the CPU restatement under oracle/ is test infrastructure and is never
imported from this package).
"""
import ctypes as C
import os
import subprocess
import time

import numpy as np

from . import abi

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# ESL_HIP_LIB: load another build of the SAME library (kernel tuning variants side by side); never a fallback
LIB_PATH = os.environ.get("ESL_HIP_LIB") or os.path.join(_CSRC, "libesl_hip.so")
_lib = None

EXPORTS = [
    "esl_abi_version", "esl_last_error", "esl_device_count", "esl_ctx_create", "esl_ctx_destroy",
    "esl_ctx_synchronize", "esl_ctx_trim", "esl_lm_params_default", "esl_optimize", "esl_optimize_fixed", "esl_graph_upload", "esl_graph_upload_fixed", "esl_graph_obj_fixed", "esl_graph_append", "esl_graph_sizes", "esl_states_upload",
    "esl_states_download", "esl_optimize_resident", "esl_states_snapshot", "esl_states_restore", "esl_profile_enable", "esl_profile_get", "esl_lm_begin", "esl_lm_linearize", "esl_lm_reduced_system", "esl_lm_reduced_residual",
    "esl_lm_try_step", "esl_lm_commit", "esl_lm_solver_used", "esl_lm_solver_stats", "esl_lm_os_counts", "esl_lm_download", "esl_lm_set_robust", "esl_edge_chi2", "esl_pcg_params_default", "esl_lm_set_pcg", "esl_lm_pcg_stats", "esl_comm_unique_id", "esl_comm_init", "esl_comm_init_host", "esl_comm_set_replicated", "esl_comm_destroy", "esl_partition_objects", "esl_fit_params_default", "esl_fit_frame", "esl_fit_frame_debug", "esl_fit_frame_ex", "esl_selftest_cholesky", "esl_debug_chol_plan", "esl_debug_update_v_applies", "esl_debug_cf_stride_choose",
    "esl_init_quadric", "esl_init_from_qstar", "esl_init_plane_error", "esl_init_quadrics", "esl_plane_params_default", "esl_extract_ground_plane", "esl_extract_planes",
    "esl_reloc_params_default", "esl_reloc_set_map", "esl_relocalize",
    "esl_assoc_params_default", "esl_predict_boxes", "esl_associate_boxes",
    "esl_init_robust_params_default", "esl_init_quadrics_robust",
    "esl_merge_params_default", "esl_map_overlaps", "esl_map_merge",
    "esl_render_params_default", "esl_render_map", "esl_debug_render_allocs", "esl_debug_scratch_allocs",
    "esl_dense_params_default", "esl_dense_begin", "esl_dense_add_frames", "esl_dense_info_get", "esl_dense_extract", "esl_dense_end",
    "esl_debug_dense_allocs", "esl_dense_obj_params_default", "esl_dense_objects",
    "esl_dense_plane_params_default", "esl_dense_planes", "esl_debug_dense_planes_layout",
    "esl_dense_remove_frames", "esl_dense_move_frames", "esl_dense_slots_get", "esl_dense_purge",
    "esl_dense_render_params_default", "esl_dense_render",
    "esl_dense_normal_params_default", "esl_dense_normals", "esl_dense_align_params_default", "esl_dense_align_frames",
    "esl_dense_carve_params_default", "esl_dense_carve_frames",
    "esl_dense_covis_params_default", "esl_dense_covis_frames",
]


class EslError(RuntimeError):
    pass


def build(force=False):
    """Compile every HIP translation unit for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", _CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", _CSRC])
    return LIB_PATH


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EslError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        L.esl_last_error.restype = C.c_char_p
        for name in EXPORTS:
            if not hasattr(L, name):
                raise EslError(f"libesl_hip.so does not export {name}")
        abi.render_argtypes(L)
        abi.dense_argtypes(L)
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        msg = load().esl_last_error().decode(errors="replace")
        raise EslError(f"{what} failed with esl_status {rc}: {msg}")


def device_count():
    return int(load().esl_device_count())


_dp = C.POINTER(C.c_double)


def _fixed_flags(obj_fixed, n_objs):
    """obj_fixed (None or n_objs flags) as a contiguous uint8 array, or None"""
    if obj_fixed is None:
        return None
    f = np.ascontiguousarray(np.asarray(obj_fixed) != 0, dtype=np.uint8).reshape(-1)
    if f.size != n_objs:
        raise ValueError(f"obj_fixed has {f.size} entries, the graph {n_objs} ellipsoids")
    return f


def _edge_counts(graph):
    return [len(graph.bbox_cam), len(graph.e3d_cam), len(graph.grav_obj), len(graph.odom_i)]


class Context:
    """One HIP device + stream + device-resident graph/states (esl_ctx)."""

    def __init__(self, device=0):
        L = load()
        self._h = C.c_void_p()
        self.device = int(device)
        _check(L.esl_ctx_create(C.c_int(device), C.byref(self._h)), "esl_ctx_create")
        self._graph = None
        self._edge_counts = [0, 0, 0, 0]   # bbox, 3-D, gravity, odometry edges of the resident graph (esl_edge_chi2)

    def close(self):
        if self._h:
            load().esl_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- one shot -----------------------------------------------------------------------------
    def optimize(self, graph, cams, objs, params=None, obj_fixed=None):
        """esl_optimize; obj_fixed (n_objs flags): esl_optimize_fixed -- those ellipsoids stay exactly as given (all of them fixed and
        free cameras: pose-only optimisation against the map)."""
        p = params if params is not None else abi.default_lm_params()
        g = graph.c_struct()
        cams = np.array(cams, dtype=np.float64, order="C").reshape(-1, 7).copy()
        objs = np.array(objs, dtype=np.float64, order="C").reshape(-1, 10).copy()
        rep = abi.EslLmReport()
        self._edge_counts = _edge_counts(graph)
        fx = _fixed_flags(obj_fixed, graph.n_objs)
        if fx is not None:
            _check(load().esl_optimize_fixed(self._h, C.byref(g), fx.ctypes.data_as(C.POINTER(C.c_uint8)), cams.ctypes.data_as(_dp),
                                             objs.ctypes.data_as(_dp), C.byref(p), C.byref(rep)), "esl_optimize_fixed")
            return cams, objs, rep.as_dict()
        _check(load().esl_optimize(self._h, C.byref(g), cams.ctypes.data_as(_dp), objs.ctypes.data_as(_dp),
                                   C.byref(p), C.byref(rep)), "esl_optimize")
        return cams, objs, rep.as_dict()

    # ---- resident / step API --------------------------------------------------------------------
    def upload_graph(self, graph, obj_fixed=None):
        """esl_graph_upload; obj_fixed (n_objs flags): esl_graph_upload_fixed."""
        g = graph.c_struct()
        fx = _fixed_flags(obj_fixed, graph.n_objs)
        if fx is not None:
            _check(load().esl_graph_upload_fixed(self._h, C.byref(g), fx.ctypes.data_as(C.POINTER(C.c_uint8))), "esl_graph_upload_fixed")
        else:
            _check(load().esl_graph_upload(self._h, C.byref(g)), "esl_graph_upload")
        self._graph = graph
        self._edge_counts = _edge_counts(graph)

    def graph_obj_fixed(self):
        """esl_graph_obj_fixed: the fixed flags of the resident graph's ellipsoids (all zero after a plain upload)."""
        n = self.graph_sizes()["n_objs"]
        f = np.zeros(max(n, 1), dtype=np.uint8)
        _check(load().esl_graph_obj_fixed(self._h, f.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int32(n)), "esl_graph_obj_fixed")
        return f[:n]

    def append_graph(self, new_cams=(), new_objs=(), bbox=None, e3d=None, grav_obj=(), new_cam_fixed=None, odom=None):
        """esl_graph_append: bbox = (cam, obj, meas (n,4), weight), e3d = (cam, obj, meas (n,10), weight); indices in the extended
        numbering (new cameras / ellipsoids follow the existing ones).  SLAM mode: new_cam_fixed = flags of the new cameras (None:
        fixed), odom = (i, j, meas (n,7)[, info (n,6)])."""
        keep = []

        def arr(a, dt, tail=None):
            a = np.ascontiguousarray(a, dtype=dt)
            if tail is not None and a.size:
                a = a.reshape((-1,) + tail)
            keep.append(a)
            return a
        d = abi.EslGraphDelta()
        nc, no = arr(new_cams, np.float64, (7,)), arr(new_objs, np.float64, (10,))
        d.n_new_cams, d.n_new_objs = (len(nc) if nc.size else 0), (len(no) if no.size else 0)
        d.new_cams = nc.ctypes.data_as(_dp) if nc.size else _dp(); d.new_objs = no.ctypes.data_as(_dp) if no.size else _dp()
        ip = C.POINTER(C.c_int32)
        if bbox is not None and len(bbox[0]):
            bc, bo, bm, bw = arr(bbox[0], np.int32), arr(bbox[1], np.int32), arr(bbox[2], np.float64, (4,)), arr(bbox[3], np.float64)
            d.n_bbox = len(bc); d.bbox_cam = bc.ctypes.data_as(ip); d.bbox_obj = bo.ctypes.data_as(ip)
            d.bbox_meas = bm.ctypes.data_as(_dp); d.bbox_weight = bw.ctypes.data_as(_dp)
        if e3d is not None and len(e3d[0]):
            ec, eo, em, ew = arr(e3d[0], np.int32), arr(e3d[1], np.int32), arr(e3d[2], np.float64, (10,)), arr(e3d[3], np.float64)
            d.n_e3d = len(ec); d.e3d_cam = ec.ctypes.data_as(ip); d.e3d_obj = eo.ctypes.data_as(ip)
            d.e3d_meas = em.ctypes.data_as(_dp); d.e3d_weight = ew.ctypes.data_as(_dp)
        go = arr(grav_obj, np.int32)
        if go.size:
            d.n_grav = len(go); d.grav_obj = go.ctypes.data_as(ip)
        if new_cam_fixed is not None and d.n_new_cams:
            fx = arr(new_cam_fixed, np.uint8)
            assert fx.size == d.n_new_cams
            d.new_cam_fixed = fx.ctypes.data_as(C.POINTER(C.c_uint8))
        if odom is not None and len(odom[0]):
            oi, oj, om = arr(odom[0], np.int32), arr(odom[1], np.int32), arr(odom[2], np.float64, (7,))
            d.n_odom = len(oi); d.odom_i = oi.ctypes.data_as(ip); d.odom_j = oj.ctypes.data_as(ip); d.odom_meas = om.ctypes.data_as(_dp)
            if len(odom) > 3 and odom[3] is not None:
                d.odom_info = arr(odom[3], np.float64, (6,)).ctypes.data_as(_dp)
        _check(load().esl_graph_append(self._h, C.byref(d)), "esl_graph_append")
        self._edge_counts = [a + b for a, b in zip(self._edge_counts, (d.n_bbox, d.n_e3d, d.n_grav, d.n_odom))]
        if self._graph is not None:
            self._graph = _Sizes(self._graph.n_cams + d.n_new_cams, self._graph.n_objs + d.n_new_objs)

    def graph_sizes(self):
        v = [C.c_int32(0) for _ in range(5)]
        _check(load().esl_graph_sizes(self._h, *[C.byref(x) for x in v]), "esl_graph_sizes")
        return dict(zip(("n_cams", "n_objs", "n_bbox", "n_e3d", "relayouts"), [x.value for x in v]))

    def upload_states(self, cams, objs):
        cams = np.ascontiguousarray(cams, dtype=np.float64)
        objs = np.ascontiguousarray(objs, dtype=np.float64)
        _check(load().esl_states_upload(self._h, cams.ctypes.data_as(_dp), objs.ctypes.data_as(_dp)), "esl_states_upload")

    def download_states(self):
        cams = np.zeros((self._graph.n_cams, 7))
        objs = np.zeros((self._graph.n_objs, 10))
        _check(load().esl_states_download(self._h, cams.ctypes.data_as(_dp), objs.ctypes.data_as(_dp)), "esl_states_download")
        return cams, objs

    def optimize_resident(self, params=None):
        p = params if params is not None else abi.default_lm_params()
        rep = abi.EslLmReport()
        _check(load().esl_optimize_resident(self._h, C.byref(p), C.byref(rep)), "esl_optimize_resident")
        return rep.as_dict()

    def lm_begin(self, params=None):
        p = params if params is not None else abi.default_lm_params()
        nv, nd = C.c_int32(0), C.c_int32(0)
        _check(load().esl_lm_begin(self._h, C.byref(p), C.byref(nv), C.byref(nd)), "esl_lm_begin")
        return nv.value, nd.value

    def lm_linearize(self):
        out = abi.EslLmPartials()
        _check(load().esl_lm_linearize(self._h, C.byref(out)), "esl_lm_linearize")
        return out

    def lm_try_step(self, lam):
        out = abi.EslLmPartials()
        _check(load().esl_lm_try_step(self._h, C.c_double(lam), C.byref(out)), "esl_lm_try_step")
        return out

    def lm_commit(self, accept):
        _check(load().esl_lm_commit(self._h, C.c_int(1 if accept else 0)), "esl_lm_commit")

    def lm_solver_used(self):
        """esl_linear_solver of the last SLAM-mode trial step: 1 reduced camera system, 2 reduced ellipsoid system (cameras first), 3 the camera chain
        alone (no free camera sees a free ellipsoid), 4 matrix-free PCG on the reduced camera system."""
        v = C.c_int32(0)
        _check(load().esl_lm_solver_used(self._h, C.byref(v)), "esl_lm_solver_used")
        return v.value

    def lm_solver_stats(self):
        """Shape of the camera-first elimination as the last trial ran it (esl_lm_solver_stats)."""
        st = (C.c_double * 10)()   # ESL_SOLVER_STATS
        _check(load().esl_lm_solver_stats(self._h, st), "esl_lm_solver_stats")
        names = ["x_form", "stride", "separators", "segments", "product_flops", "product_bytes", "slab_bytes", "dense_update_rows",
                 "dense_update_flops_executed", "t_ordered_by_first_camera"]
        return {n: float(st[i]) for i, n in enumerate(names)}

    def lm_os_counts(self):
        """The one-sided assembly's pair list as the last trial ran it (esl_lm_os_counts)."""
        n = (C.c_double * abi.ESL_OS_COUNTS)()
        _check(load().esl_lm_os_counts(self._h, n), "esl_lm_os_counts")
        names = ["row_side_pairs", "merged_pairs", "merged_shorter_side_pairs", "list_pairs", "list_flops", "list_bytes"]
        return {k: float(n[i]) for i, k in enumerate(names)}

    def lm_reduced_system(self, lam):
        ptr, n, lda = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        _check(load().esl_lm_reduced_system(self._h, C.c_double(lam), C.byref(ptr), C.byref(n), C.byref(lda)),
               "esl_lm_reduced_system")
        return ptr.value, n.value, lda.value

    def lm_reduced_residual(self):
        """|S x_c - b_s| / |b_s| of the last SLAM-mode trial step (the reduced system is re-built for it)."""
        r = C.c_double(0)
        _check(load().esl_lm_reduced_residual(self._h, C.byref(r)), "esl_lm_reduced_residual")
        return r.value

    def set_robust(self, bbox=None, e3d=None, grav=None, odom=None):
        """esl_lm_set_robust: each argument None (no kernel) or (kind name, delta), e.g. bbox=("huber", 1.0); kinds: none, huber,
        pseudo_huber, cauchy, tukey.  The setting stays with the context and applies from the next run on."""
        p = abi.default_robust_params(bbox=bbox, e3d=e3d, grav=grav, odom=odom)
        _check(load().esl_lm_set_robust(self._h, C.byref(p)), "esl_lm_set_robust")

    def set_pcg(self, max_iters=None, check_every=None, rel_tol=None):
        """esl_lm_set_pcg: the settings of ESL_SOLVER_PCG (None: the default -- 1000 iterations, a host look every 8, rel_tol 1e-10).  The
        setting stays with the context and applies from the next run on."""
        p = abi.default_pcg_params()
        if max_iters is not None:
            p.max_iters = int(max_iters)
        if check_every is not None:
            p.check_every = int(check_every)
        if rel_tol is not None:
            p.rel_tol = float(rel_tol)
        _check(load().esl_lm_set_pcg(self._h, C.byref(p)), "esl_lm_set_pcg")

    def lm_pcg_stats(self):
        """esl_lm_pcg_stats: the last PCG solve and the sums over this run's solves (all zeros before any PCG trial)."""
        st = (C.c_double * 8)()   # ESL_PCG_STATS
        _check(load().esl_lm_pcg_stats(self._h, st), "esl_lm_pcg_stats")
        names = ["iterations", "rel_residual", "converged", "solves", "iterations_total", "max_iters", "rel_tol", "reserved"]
        return {n: float(st[i]) for i, n in enumerate(names)}

    def edge_chi2(self, edge_class):
        """esl_edge_chi2: (raw chi2, robust weight rho1) of every edge of one class ("bbox", "e3d", "grav", "odom" or its number) at the
        resident states, in caller order (upload order, then append order)."""
        cls = abi.EDGE_CLASSES[edge_class] if isinstance(edge_class, str) else int(edge_class)
        n = self._edge_counts[cls]
        chi, w = np.zeros(n), np.zeros(n)
        _check(load().esl_edge_chi2(self._h, C.c_int32(cls), chi.ctypes.data_as(_dp), w.ctypes.data_as(_dp), C.c_int64(n)),
               "esl_edge_chi2")
        return chi, w

    def lm_download(self, which, count):
        out = np.zeros(int(count))
        _check(load().esl_lm_download(self._h, C.c_int32(which), out.ctypes.data_as(_dp), C.c_int64(int(count))),
               "esl_lm_download")
        return out

    def snapshot_states(self):
        _check(load().esl_states_snapshot(self._h), "esl_states_snapshot")

    def restore_states(self):
        _check(load().esl_states_restore(self._h), "esl_states_restore")

    def profile_enable(self, level=2):
        """0/False off; 1 only the linearise kernels (cheap, for timed regions); 2/True every kernel class."""
        lv = 2 if level is True else int(level)
        _check(load().esl_profile_enable(self._h, C.c_int(lv)), "esl_profile_enable")

    def profile_get(self):
        cnt = (C.c_int64 * 10)()   # ESL_PROF_KINDS
        ms = (C.c_double * 10)()
        _check(load().esl_profile_get(self._h, cnt, ms), "esl_profile_get")
        names = ["linearize", "lm_trial", "schur_build", "cholesky_solve", "reduce", "k5", "shard_allreduce", "rank_k_update", "sparse_block_products",
                 "dense_factorisation"]
        return {n: dict(count=int(cnt[i]), total_ms=float(ms[i])) for i, n in enumerate(names) if cnt[i]}

    def init_quadric(self, poses_Twc, bboxes, K, rows=480, cols=640, faithful=1):
        """Initializer::initializeQuadric: returns (ellipsoid 10-vector, Q* 4x4, ok)."""
        poses = np.ascontiguousarray(poses_Twc, dtype=np.float64).reshape(-1, 7)
        boxes = np.ascontiguousarray(bboxes, dtype=np.float64).reshape(-1, 4)
        Kd = np.ascontiguousarray(K, dtype=np.float64)
        e = np.zeros(10); Q = np.zeros(16); ok = C.c_int32(0)
        _check(load().esl_init_quadric(self._h, poses.ctypes.data_as(_dp), boxes.ctypes.data_as(_dp), C.c_int32(len(poses)),
                                       Kd.ctypes.data_as(_dp), C.c_int32(rows), C.c_int32(cols), C.c_int32(faithful),
                                       e.ctypes.data_as(_dp), Q.ctypes.data_as(_dp), C.byref(ok)), "esl_init_quadric")
        return e, Q.reshape(4, 4), bool(ok.value)

    def init_from_qstar(self, qstar, faithful=1):
        """Initializer::getEllipsoidFromQStar: (ellipsoid 10-vector, ok)."""
        Q = np.ascontiguousarray(qstar, dtype=np.float64).reshape(16)
        e = np.zeros(10); ok = C.c_int32(0)
        _check(load().esl_init_from_qstar(self._h, Q.ctypes.data_as(_dp), C.c_int32(faithful), e.ctypes.data_as(_dp), C.byref(ok)),
               "esl_init_from_qstar")
        return e, bool(ok.value)

    def init_plane_error(self, poses_Twc, bboxes, K, ellipsoid, rows=480, cols=640):
        """Initializer::quadricErrorWithPlanes."""
        poses = np.ascontiguousarray(poses_Twc, dtype=np.float64).reshape(-1, 7)
        boxes = np.ascontiguousarray(bboxes, dtype=np.float64).reshape(-1, 4)
        Kd = np.ascontiguousarray(K, dtype=np.float64); e = np.ascontiguousarray(ellipsoid, dtype=np.float64)
        err = C.c_double(0)
        _check(load().esl_init_plane_error(self._h, poses.ctypes.data_as(_dp), boxes.ctypes.data_as(_dp), C.c_int32(len(poses)),
                                           Kd.ctypes.data_as(_dp), C.c_int32(rows), C.c_int32(cols), e.ctypes.data_as(_dp),
                                           C.byref(err)), "esl_init_plane_error")
        return err.value

    def init_quadrics(self, cams, N, obs_cam, obs_obj, obs_boxes, K, rows=480, cols=640, faithful=1, min_observations=0):
        """esl_init_quadrics: Initializer::initializeQuadric for N objects in one call.  cams (F, 7) Tcw, or None for the resident
        graph's current camera states; the observations as an edge list obs_cam (n_obs,), obs_obj (n_obs,; < 0 = skipped),
        obs_boxes (n_obs, 4).  Returns (ellipsoids (N, 10), qstar (N, 4, 4), plane_error (N,), stats (N, 4): status, observations,
        planes, spilled)."""
        _ip = C.POINTER(C.c_int32)

        def ptr(a, t):
            return a.ctypes.data_as(t) if a.size else t()
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        oc = np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
        oo = np.ascontiguousarray(obs_obj, dtype=np.int32).reshape(-1)
        ob = np.ascontiguousarray(obs_boxes, dtype=np.float64).reshape(-1, 4)
        if not len(oc) == len(oo) == len(ob):
            raise ValueError(f"{len(oc)} frame indices, {len(oo)} object indices, {len(ob)} boxes")
        if cams is None:
            F, cp = (self._graph.n_cams if self._graph is not None else 0), _dp()
        else:
            cams = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, 7)
            F, cp = len(cams), ptr(cams, _dp)
        N = int(N)
        n = max(N, 1)
        e = np.zeros((n, 10)); Q = np.zeros((n, 16)); err = np.zeros(n); stats = np.zeros((n, 4), dtype=np.int32)
        t0 = time.perf_counter()
        rc = load().esl_init_quadrics(self._h, cp, C.c_int32(F), C.c_int32(N), ptr(oc, _ip), ptr(oo, _ip), ptr(ob, _dp),
                                      C.c_int64(len(oc)), Kc.ctypes.data_as(_dp), C.c_int32(rows), C.c_int32(cols), C.c_int32(faithful),
                                      C.c_int32(min_observations), e.ctypes.data_as(_dp), Q.ctypes.data_as(_dp), err.ctypes.data_as(_dp),
                                      stats.ctypes.data_as(_ip))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_init_quadrics")
        return e[:max(N, 0)], Q[:max(N, 0)].reshape(-1, 4, 4), err[:max(N, 0)], stats[:max(N, 0)]

    def init_quadrics_robust(self, cams, N, obs_cam, obs_obj, obs_boxes, K, rows=480, cols=640, faithful=1, min_observations=0,
                             params=None, want_hyp=False):
        """esl_init_quadrics_robust: esl_init_quadrics by consensus over small view subsets, which rejects outlier boxes.  Arguments as
        init_quadrics; params an abi.EslInitRobustParams (None: the defaults).  Returns dict(ellipsoids (N, 10), qstar (N, 4, 4),
        plane_error (N,), stats (N, 8): status, observations, planes, spilled, final inliers, valid hypotheses, winner, refined;
        inliers (n_obs,) 0 / 1, residuals (n_obs,) px or NaN, hyp (N, n_hypotheses, 4): valid, planes, inliers, cost -- or None)."""
        _ip = C.POINTER(C.c_int32)

        def ptr(a, t):
            return a.ctypes.data_as(t) if a.size else t()
        p = params if params is not None else abi.default_init_robust_params()
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        oc = np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
        oo = np.ascontiguousarray(obs_obj, dtype=np.int32).reshape(-1)
        ob = np.ascontiguousarray(obs_boxes, dtype=np.float64).reshape(-1, 4)
        if not len(oc) == len(oo) == len(ob):
            raise ValueError(f"{len(oc)} frame indices, {len(oo)} object indices, {len(ob)} boxes")
        if cams is None:
            F, cp = (self._graph.n_cams if self._graph is not None else 0), _dp()
        else:
            cams = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, 7)
            F, cp = len(cams), ptr(cams, _dp)
        N = int(N)
        n, no, H = max(N, 1), max(len(oc), 1), max(int(p.n_hypotheses), 1)
        e = np.zeros((n, 10)); Q = np.zeros((n, 16)); err = np.zeros(n); stats = np.zeros((n, 8), dtype=np.int32)
        inl = np.zeros(no, dtype=np.int32); res = np.full(no, np.nan)
        hyp = np.zeros((n, H, 4)) if want_hyp else None
        t0 = time.perf_counter()
        rc = load().esl_init_quadrics_robust(self._h, cp, C.c_int32(F), C.c_int32(N), ptr(oc, _ip), ptr(oo, _ip), ptr(ob, _dp),
                                             C.c_int64(len(oc)), Kc.ctypes.data_as(_dp), C.c_int32(rows), C.c_int32(cols),
                                             C.c_int32(faithful), C.c_int32(min_observations), C.byref(p), e.ctypes.data_as(_dp),
                                             Q.ctypes.data_as(_dp), err.ctypes.data_as(_dp), stats.ctypes.data_as(_ip),
                                             inl.ctypes.data_as(_ip), res.ctypes.data_as(_dp), hyp.ctypes.data_as(_dp) if want_hyp else _dp())
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_init_quadrics_robust")
        N = max(N, 0)
        return dict(ellipsoids=e[:N], qstar=Q[:N].reshape(-1, 4, 4), plane_error=err[:N], stats=stats[:N], inliers=inl[:len(oc)],
                    residuals=res[:len(oc)], hyp=hyp[:N] if want_hyp else None)

    def fit_frame(self, depth, bboxes, labels, Twc, intr, ground, params=None):
        """EllipsoidExtractor::EstimateLocalEllipsoid for every box of one frame.
        Returns (ellipsoids (B,10) in the camera frame, prob (B,), status (B,), debug (B,16))."""
        p = params if params is not None else default_fit_params()
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        h, w = depth.shape
        boxes = np.ascontiguousarray(bboxes, dtype=np.float64).reshape(-1, 4)
        B = len(boxes)
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        Twc = np.ascontiguousarray(Twc, dtype=np.float64); intr = np.ascontiguousarray(intr, dtype=np.float64)
        ground = np.ascontiguousarray(ground, dtype=np.float64)
        ell = np.zeros((B, 10)); prob = np.zeros(B); st = np.zeros(B, dtype=np.int32); dbg = np.zeros((B, 16))
        fn = load().esl_fit_frame_debug
        cargs = (self._h, depth.ctypes.data_as(C.POINTER(C.c_uint16)), C.c_int32(w), C.c_int32(h),
                 boxes.ctypes.data_as(_dp), lab.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(B),
                 Twc.ctypes.data_as(_dp), intr.ctypes.data_as(_dp), ground.ctypes.data_as(_dp),
                 C.byref(p), ell.ctypes.data_as(_dp), prob.ctypes.data_as(_dp),
                 st.ctypes.data_as(C.POINTER(C.c_int32)), dbg.ctypes.data_as(_dp))
        t0 = time.perf_counter()
        rc = fn(*cargs)
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone (bench.py reports it next to the Python-inclusive time)
        _check(rc, "esl_fit_frame")
        return ell, prob, st, dbg

    def fit_frame_ex(self, depth, bboxes, labels, Twc, intr, ground, params=None):
        """fit_frame + SymmetryOutputData per box (EllipsoidExtractor::GetSymmetryOutputData): returns
        (ellipsoids, prob, status, debug, sym) with sym a dict of arrays result (B,), symmetry_type (B,), plane (B,4),
        plane2 (B,4), prob (B,), center (B,3)."""
        p = params if params is not None else default_fit_params()
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        h, w = depth.shape
        boxes = np.ascontiguousarray(bboxes, dtype=np.float64).reshape(-1, 4)
        B = len(boxes)
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        Twc = np.ascontiguousarray(Twc, dtype=np.float64); intr = np.ascontiguousarray(intr, dtype=np.float64)
        ground = np.ascontiguousarray(ground, dtype=np.float64)
        ell = np.zeros((B, 10)); prob = np.zeros(B); st = np.zeros(B, dtype=np.int32); dbg = np.zeros((B, 16))
        sym = (abi.EslFitSymmetry * max(B, 1))()
        _check(load().esl_fit_frame_ex(self._h, depth.ctypes.data_as(C.POINTER(C.c_uint16)), C.c_int32(w), C.c_int32(h),
                                       boxes.ctypes.data_as(_dp), lab.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(B),
                                       Twc.ctypes.data_as(_dp), intr.ctypes.data_as(_dp), ground.ctypes.data_as(_dp),
                                       C.byref(p), ell.ctypes.data_as(_dp), prob.ctypes.data_as(_dp),
                                       st.ctypes.data_as(C.POINTER(C.c_int32)), sym, dbg.ctypes.data_as(_dp)), "esl_fit_frame_ex")
        out = dict(result=np.array([sym[b].result for b in range(B)], dtype=np.int32),
                   symmetry_type=np.array([sym[b].symmetry_type for b in range(B)], dtype=np.int32),
                   plane=np.array([list(sym[b].plane) for b in range(B)]).reshape(B, 4),
                   plane2=np.array([list(sym[b].plane2) for b in range(B)]).reshape(B, 4),
                   prob=np.array([sym[b].prob for b in range(B)]),
                   center=np.array([list(sym[b].center) for b in range(B)]).reshape(B, 3))
        return ell, prob, st, dbg, out

    def extract_ground_plane(self, depth, intr, params=None):
        """PlaneExtractor::extractGroundPlane: dict(ok, plane (camera frame, 4), n_planes, n_pixels)."""
        p = params if params is not None else abi.default_plane_params()
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        h, w = depth.shape
        intr = np.ascontiguousarray(intr, dtype=np.float64)
        plane = np.zeros(4); ok = C.c_int32(0); npl = C.c_int32(0); npx = C.c_int32(0)
        _check(load().esl_extract_ground_plane(self._h, depth.ctypes.data_as(C.POINTER(C.c_uint16)), C.c_int32(w), C.c_int32(h),
                                               intr.ctypes.data_as(_dp), C.byref(p), plane.ctypes.data_as(_dp), C.byref(ok),
                                               C.byref(npl), C.byref(npx)), "esl_extract_ground_plane")
        return dict(ok=bool(ok.value), plane=plane, n_planes=npl.value, n_pixels=npx.value)

    def extract_planes(self, depth, intr, params=None, max_planes=64):
        """PlaneExtractor::extractPlanes: dict(n_planes, planes (n, 4), sizes (n,), labels (h, w) plane index or -1)."""
        p = params if params is not None else abi.default_plane_params()
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        h, w = depth.shape
        intr = np.ascontiguousarray(intr, dtype=np.float64)
        planes = np.zeros((max(max_planes, 1), 4)); sizes = np.zeros(max(max_planes, 1), dtype=np.int32); n = C.c_int32(0)
        labels = np.zeros((h, w), dtype=np.int32)
        _check(load().esl_extract_planes(self._h, depth.ctypes.data_as(C.POINTER(C.c_uint16)), C.c_int32(w), C.c_int32(h),
                                         intr.ctypes.data_as(_dp), C.byref(p), C.c_int32(max_planes), planes.ctypes.data_as(_dp),
                                         sizes.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n),
                                         labels.ctypes.data_as(C.POINTER(C.c_int32))), "esl_extract_planes")
        k = min(n.value, max_planes)
        return dict(n_planes=n.value, planes=planes[:k], sizes=sizes[:k], labels=labels)

    def reloc_set_map(self, objs, labels, ground_world):
        """esl_reloc_set_map: the fixed map esl_relocalize searches -- objs (M, 10) world ellipsoids, or None to take the resident
        graph's current ellipsoid states on the device; labels (M,); the world ground plane (4,)."""
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        gw = np.ascontiguousarray(ground_world, dtype=np.float64).reshape(4)
        if objs is None:
            op = _dp()
        else:
            objs = np.ascontiguousarray(objs, dtype=np.float64).reshape(-1, 10)
            if len(objs) != len(lab):
                raise ValueError(f"{len(objs)} ellipsoids, {len(lab)} labels")
            op = objs.ctypes.data_as(_dp)
        _check(load().esl_reloc_set_map(self._h, op, lab.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(len(lab)),
                                        gw.ctypes.data_as(_dp)), "esl_reloc_set_map")

    def relocalize(self, det_objs, det_labels, ground_cam, params=None):
        """esl_relocalize: camera pose and detection -> map association of one frame against the map of reloc_set_map, with no
        pose prior.  det_objs (D, 10) single-frame ellipsoids in the camera frame (fit_frame's output), det_labels (D,), ground_cam
        the ground plane in the camera frame.  Returns (dict of esl_reloc_result, assoc (D,) map index or -1); status 1 - 3 are
        results, not errors."""
        p = params if params is not None else abi.default_reloc_params()
        det = np.ascontiguousarray(det_objs, dtype=np.float64).reshape(-1, 10)
        lab = np.ascontiguousarray(det_labels, dtype=np.int32).reshape(-1)
        if len(det) != len(lab):
            raise ValueError(f"{len(det)} detections, {len(lab)} labels")
        gc = np.ascontiguousarray(ground_cam, dtype=np.float64).reshape(4)
        D = len(det)
        assoc = np.full(max(D, 1), -1, dtype=np.int32)
        res = abi.EslRelocResult()
        t0 = time.perf_counter()
        rc = load().esl_relocalize(self._h, det.ctypes.data_as(_dp) if D else _dp(),
                                   lab.ctypes.data_as(C.POINTER(C.c_int32)) if D else C.POINTER(C.c_int32)(), C.c_int32(D),
                                   gc.ctypes.data_as(_dp), C.byref(p), C.byref(res), assoc.ctypes.data_as(C.POINTER(C.c_int32)))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_relocalize")
        return res.as_dict(), assoc[:D]

    def predict_boxes(self, Tcw, objs, K, rows, cols, params=None):
        """esl_predict_boxes: the map's predicted boxes in one frame.  Tcw (7,), objs (M, 10) world ellipsoids or None for the resident
        graph's current ellipsoid states.  Returns (boxes (M, 4) clipped, NaN where not eligible; depth (M,); flags (M,) bit 0 eligible,
        bit 1 occluded)."""
        p = params if params is not None else abi.default_assoc_params()
        _ip = C.POINTER(C.c_int32)
        Tcw = np.ascontiguousarray(Tcw, dtype=np.float64).reshape(7)
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        if objs is None:
            M, op = self.graph_sizes()["n_objs"], _dp()
        else:
            objs = np.ascontiguousarray(objs, dtype=np.float64).reshape(-1, 10)
            M, op = len(objs), (objs.ctypes.data_as(_dp) if len(objs) else _dp())
        boxes = np.full((max(M, 1), 4), np.nan); depth = np.full(max(M, 1), np.nan); flags = np.zeros(max(M, 1), dtype=np.int32)
        _check(load().esl_predict_boxes(self._h, Tcw.ctypes.data_as(_dp), op, C.c_int32(M), Kc.ctypes.data_as(_dp), C.c_int32(rows),
                                        C.c_int32(cols), C.byref(p), boxes.ctypes.data_as(_dp), depth.ctypes.data_as(_dp),
                                        flags.ctypes.data_as(_ip)), "esl_predict_boxes")
        return boxes[:M], depth[:M], flags[:M]

    def associate_boxes(self, cams, objs, obj_labels, K, rows, cols, det_offsets, det_boxes, det_labels, params=None):
        """esl_associate_boxes: detection boxes -> map objects in many frames, given the poses.  cams (F, 7) Tcw and objs (M, 10), or
        None for the resident graph's current states; obj_labels (M,); det_offsets (F + 1,) CSR; det_boxes (n_det, 4) x1 y1 x2 y2;
        det_labels (n_det,).  Returns (assoc (n_det,) map index or -1, iou (n_det,), frame_stats (F, 4): eligible, occluded, assigned,
        spilled)."""
        p = params if params is not None else abi.default_assoc_params()
        _ip = C.POINTER(C.c_int32)

        def ptr(a, t):
            return a.ctypes.data_as(t) if a.size else t()
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        off = np.ascontiguousarray(det_offsets, dtype=np.int32).reshape(-1)
        db = np.ascontiguousarray(det_boxes, dtype=np.float64).reshape(-1, 4)
        dl = np.ascontiguousarray(det_labels, dtype=np.int32).reshape(-1)
        ol = np.ascontiguousarray(obj_labels, dtype=np.int32).reshape(-1)
        if len(db) != len(dl):
            raise ValueError(f"{len(db)} detection boxes, {len(dl)} labels")
        if len(off) and off[-1] != len(db):
            raise ValueError(f"det_offsets end at {off[-1]}, there are {len(db)} detection boxes")
        if cams is None:
            F, cp = len(off) - 1, _dp()
        else:
            cams = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, 7)
            F, cp = len(cams), ptr(cams, _dp)
            if len(off) != F + 1:
                raise ValueError(f"{F} frames need {F + 1} offsets, got {len(off)}")
        if objs is None:
            M, op = len(ol), _dp()
        else:
            objs = np.ascontiguousarray(objs, dtype=np.float64).reshape(-1, 10)
            M, op = len(objs), ptr(objs, _dp)
            if len(ol) != M:
                raise ValueError(f"{M} ellipsoids, {len(ol)} labels")
        n = len(db)
        assoc = np.full(max(n, 1), -1, dtype=np.int32); iou = np.zeros(max(n, 1)); stats = np.zeros((max(F, 1), 4), dtype=np.int32)
        t0 = time.perf_counter()
        rc = load().esl_associate_boxes(self._h, cp, C.c_int32(F), op, ptr(ol, _ip), C.c_int32(M), Kc.ctypes.data_as(_dp),
                                        C.c_int32(rows), C.c_int32(cols), ptr(off, _ip), ptr(db, _dp), ptr(dl, _ip), C.byref(p),
                                        assoc.ctypes.data_as(_ip), iou.ctypes.data_as(_dp), stats.ctypes.data_as(_ip))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_associate_boxes")
        return assoc[:n], iou[:n], stats[:F]

    def _merge_map(self, objs, labels):
        """(M, objs pointer, labels array, the array behind the pointer) of map_overlaps / map_merge; objs None: the resident states"""
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if objs is None:
            return len(lab), _dp(), lab, None
        objs = np.ascontiguousarray(objs, dtype=np.float64).reshape(-1, 10)
        if len(objs) != len(lab):
            raise ValueError(f"{len(objs)} ellipsoids, {len(lab)} labels")
        return len(objs), (objs.ctypes.data_as(_dp) if len(objs) else _dp()), lab, objs

    def map_overlaps(self, objs, labels, params=None, cap=None):
        """esl_map_overlaps: the overlapping pairs of a map with their lattice counts and measures.  objs (M, 10) world ellipsoids, or
        None for the resident graph's current ellipsoid states; labels (M,); cap: how many pairs to fetch at most (None: all).  Returns
        dict(pairs (k, 2), counts (k, 2): cnt_ij, cnt_ji, iou (k,), contain (k,), n_pairs, n_candidates), k = min(cap, n_pairs);
        n_pairs is -1 when there are more candidates than max_pairs."""
        p = params if params is not None else abi.default_merge_params()
        _ip, _lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        M, op, lab, _keep = self._merge_map(objs, labels)
        n_pairs, n_cand = C.c_int64(0), C.c_int64(0)

        def call(cap):
            k = max(int(cap), 1)
            pairs = np.zeros((k, 2), dtype=np.int32); cnt = np.zeros((k, 2), dtype=np.int32); iou = np.zeros(k); con = np.zeros(k)
            t0 = time.perf_counter()
            rc = load().esl_map_overlaps(self._h, op, lab.ctypes.data_as(_ip) if M else _ip(), C.c_int32(M), C.byref(p), C.c_int64(cap),
                                         pairs.ctypes.data_as(_ip), cnt.ctypes.data_as(_ip), iou.ctypes.data_as(_dp), con.ctypes.data_as(_dp),
                                         C.byref(n_pairs), C.byref(n_cand))
            self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
            _check(rc, "esl_map_overlaps")
            return pairs, cnt, iou, con
        if cap is None:              # ask for the count, then for everything
            call(0)
            cap = max(n_pairs.value, 0)
        pairs, cnt, iou, con = call(cap)
        k = max(min(int(cap), n_pairs.value), 0)
        return dict(pairs=pairs[:k], counts=cnt[:k], iou=iou[:k], contain=con[:k], n_pairs=n_pairs.value, n_candidates=n_cand.value)

    def map_merge(self, objs, labels, weights=None, obs_cam=None, obs_obj=None, params=None):
        """esl_map_merge: find the duplicate ellipsoids of a map, fuse them, rewrite an edge list.  objs (M, 10) or None for the resident
        ellipsoid states; labels (M,); weights (M,) int or None (the objects' list entries, or 1 without a list); obs_cam / obs_obj
        (n_obs,) the edge list or None.  Returns dict(result: dict of esl_merge_result, group (M,), new_index (M,), objs (n_groups, 10),
        labels (n_groups,), weights (n_groups,), obs_obj (n_obs,) or None)."""
        p = params if params is not None else abi.default_merge_params()
        _ip = C.POINTER(C.c_int32)

        def ptr(a, t):
            return a.ctypes.data_as(t) if a is not None and a.size else t()
        M, op, lab, _keep = self._merge_map(objs, labels)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32).reshape(-1)
        if w is not None and len(w) != M:
            raise ValueError(f"{M} ellipsoids, {len(w)} weights")
        oc = None if obs_cam is None else np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
        oo = None if obs_obj is None else np.ascontiguousarray(obs_obj, dtype=np.int32).reshape(-1)
        if (oc is None) != (oo is None) or (oc is not None and len(oc) != len(oo)):
            raise ValueError("obs_cam and obs_obj go together and have equal lengths")
        n_obs = 0 if oo is None else len(oo)
        m = max(M, 1)
        group = np.zeros(m, dtype=np.int32); new = np.zeros(m, dtype=np.int32); mo = np.zeros((m, 10)); ml = np.zeros(m, dtype=np.int32)
        mw = np.zeros(m, dtype=np.int32); out = np.full(max(n_obs, 1), -1, dtype=np.int32)
        res = abi.EslMergeResult()
        t0 = time.perf_counter()
        rc = load().esl_map_merge(self._h, op, ptr(lab, _ip), ptr(w, _ip), C.c_int32(M), ptr(oc, _ip), ptr(oo, _ip), C.c_int64(n_obs),
                                  C.byref(p), group.ctypes.data_as(_ip), new.ctypes.data_as(_ip), mo.ctypes.data_as(_dp),
                                  ml.ctypes.data_as(_ip), mw.ctypes.data_as(_ip), out.ctypes.data_as(_ip) if n_obs else _ip(),
                                  C.byref(res))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_map_merge")
        G = res.n_groups
        return dict(result=res.as_dict(), group=group[:M], new_index=new[:M], objs=mo[:G], labels=ml[:G], weights=mw[:G],
                    obs_obj=out[:n_obs] if oo is not None else None)

    def render_map(self, cams, objs, K, rows, cols, depth_meas=None, params=None, want=("depth", "inst", "cover", "flags")):
        """esl_render_map: the ray cast of every pixel against every ellipsoid, nearest hit kept.  cams (F, 7) Tcw and objs (M, 10) world,
        or None for the resident graph's current states; depth_meas (F, rows, cols) uint16 or None.  want names the outputs to compute;
        "cmp" is added when a depth is given.  Returns a dict of numpy arrays: depth (F, rows, cols) NaN where nothing is hit, inst
        (F, rows, cols) map index or -1, cover (F, M, 2) pixels hit / pixels won, cmp (F, M, 4) agree / nearer / farther / no data,
        flags (F, M) bit 0 drawn, bit 1 invalid, bit 2 camera inside, bit 3 bounded by its conic box."""
        p = params if params is not None else abi.default_render_params()
        want = set(want)
        if depth_meas is not None:
            want.add("cmp")
        unknown = want - {"depth", "inst", "cover", "cmp", "flags"}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        _ip, _up = C.POINTER(C.c_int32), C.POINTER(C.c_uint16)
        sizes = self.graph_sizes() if cams is None or objs is None else None
        if cams is None:
            F, cp = sizes["n_cams"], None
        else:
            cams = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, 7)
            F, cp = len(cams), (cams.ctypes.data_as(_dp) if len(cams) else None)
        if objs is None:
            M, op = sizes["n_objs"], None
        else:
            objs = np.ascontiguousarray(objs, dtype=np.float64).reshape(-1, 10)
            M, op = len(objs), (objs.ctypes.data_as(_dp) if len(objs) else None)
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        rows, cols = int(rows), int(cols)
        mp = None
        if depth_meas is not None:
            depth_meas = np.ascontiguousarray(depth_meas, dtype=np.uint16)
            if depth_meas.shape != (F, rows, cols):
                raise ValueError(f"depth_meas has shape {depth_meas.shape}, expected {(F, rows, cols)}")
            mp = depth_meas.ctypes.data_as(_up)          # an empty array has a valid address too
        r, c = (rows, cols) if rows > 0 and cols > 0 else (0, 0)          # the library refuses such a shape before it writes
        out = {}
        if "depth" in want:
            out["depth"] = np.full((F, r, c), np.nan)
        if "inst" in want:
            out["inst"] = np.full((F, r, c), -1, dtype=np.int32)
        if "cover" in want:
            out["cover"] = np.zeros((F, M, 2), dtype=np.int32)
        if "cmp" in want:
            out["cmp"] = np.zeros((F, M, 4), dtype=np.int32)
        if "flags" in want:
            out["flags"] = np.zeros((F, M), dtype=np.int32)

        def optr(k, t):
            return out[k].ctypes.data_as(t) if k in out else None
        t0 = time.perf_counter()
        rc = load().esl_render_map(self._h, cp, F, op, M, Kc.ctypes.data_as(_dp), rows, cols, mp, C.byref(p), optr("depth", _dp),
                                   optr("inst", _ip), optr("cover", _ip), optr("cmp", _ip), optr("flags", _ip))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_render_map")
        return out

    SCRATCH_OWNERS = ("reloc", "assoc", "merge", "render", "init_batch", "init_robust")   # esl_scratch_owner

    def scratch_allocs(self, owner):
        """esl_debug_scratch_allocs: (device allocations the owner's calls have made on this context, bytes its buffers hold);
        owner: a name of SCRATCH_OWNERS or the enum's value"""
        n, b = C.c_int64(0), C.c_int64(0)
        k = self.SCRATCH_OWNERS.index(owner) if isinstance(owner, str) else int(owner)
        _check(load().esl_debug_scratch_allocs(self._h, k, C.byref(n), C.byref(b)), "esl_debug_scratch_allocs")
        return n.value, b.value

    def render_allocs(self):
        """esl_debug_render_allocs: (device allocations render_map has made on this context, bytes its buffers hold)"""
        n, b = C.c_int64(0), C.c_int64(0)
        _check(load().esl_debug_render_allocs(self._h, C.byref(n), C.byref(b)), "esl_debug_render_allocs")
        return n.value, b.value

    # ---- the dense map ---------------------------------------------------------------------------
    DENSE_OUTPUTS = ("key", "xyz", "count", "bgr", "inst", "votes")

    def dense_begin(self, params=None, with_color=True, with_inst=True):
        """esl_dense_begin: start an empty voxel-fused map on this context (params: abi.default_dense_params(...))"""
        p = params if params is not None else abi.default_dense_params()
        _check(load().esl_dense_begin(self._h, C.byref(p), int(bool(with_color)), int(bool(with_inst))), "esl_dense_begin")

    def dense_add_frames(self, cams, K, rows, cols, depth, bgr=None, inst=None):
        """esl_dense_add_frames: add F frames.  cams (F, 7) Tcw or None for the resident camera states; depth (F, rows, cols) uint16,
        bgr (F, rows, cols, 3) uint8, inst (F, rows, cols) int32 (< 0 = unlabelled).  Returns the call's counts as a dict."""
        return self._dense_frames("esl_dense_add_frames", abi.EslDenseAddResult(), (cams,), K, rows, cols, depth, bgr, inst)

    def _dense_frames(self, name, res, cam_sets, K, rows, cols, depth, bgr, inst):
        """the frame calls of the dense map: cam_sets = the call's pose arrays, the last of which may be None (the resident states)"""
        rows, cols = int(rows), int(cols)
        sets = [None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 7) for a in cam_sets]
        F = self.graph_sizes()["n_cams"] if sets[-1] is None else len(sets[-1])
        if any(a is not None and len(a) != F for a in sets):
            raise ValueError("the pose sets differ in length")
        cps = [a.ctypes.data_as(_dp) if a is not None and len(a) else None for a in sets]

        def img(a, dt, t, tail=()):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape != (F, rows, cols) + tail:
                raise ValueError(f"an image array has shape {a.shape}, expected {(F, rows, cols) + tail}")
            return a, a.ctypes.data_as(t)
        depth, dptr = img(depth, np.uint16, C.POINTER(C.c_uint16))
        bgr, bptr = img(bgr, np.uint8, C.POINTER(C.c_uint8), (3,))
        inst, iptr = img(inst, np.int32, C.POINTER(C.c_int32))
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        t0 = time.perf_counter()
        rc = getattr(load(), name)(self._h, *cps, F, Kc.ctypes.data_as(_dp), rows, cols, dptr, bptr, iptr, C.byref(res))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, name)
        return res.as_dict()

    def dense_remove_frames(self, cams, K, rows, cols, depth, bgr=None, inst=None):
        """esl_dense_remove_frames: subtract F frames, given exactly as they were added (cams None = the resident camera states).
        Returns the call's counts as a dict, n_missing and n_emptied among them; status 4 = the map is inconsistent."""
        return self._dense_frames("esl_dense_remove_frames", abi.EslDenseRemoveResult(), (cams,), K, rows, cols, depth, bgr, inst)

    def dense_move_frames(self, cams_old, cams_new, K, rows, cols, depth, bgr=None, inst=None):
        """esl_dense_move_frames: remove the frames with cams_old and add them with cams_new (None = the resident camera states) in one
        call; frames whose pose did not change in any bit are skipped.  Returns dict(removed, added, n_frames_moved, n_frames_same)."""
        if cams_old is None:
            raise ValueError("cams_old may not be None")
        return self._dense_frames("esl_dense_move_frames", abi.EslDenseMoveResult(), (cams_old, cams_new), K, rows, cols, depth, bgr, inst)

    def dense_slots(self):
        """esl_dense_slots_get as a dict: voxel_slots, dead_voxels, pair_slots, dead_pairs (claimed slots and the dead among them)"""
        out = abi.EslDenseSlots()
        _check(load().esl_dense_slots_get(self._h, C.byref(out)), "esl_dense_slots_get")
        return out.as_dict()

    def dense_purge(self):
        """esl_dense_purge: rebuild the tables from the live voxels and pairs.  Returns (slots before, slots after) as dicts."""
        b, a = abi.EslDenseSlots(), abi.EslDenseSlots()
        t0 = time.perf_counter()
        rc = load().esl_dense_purge(self._h, C.byref(b), C.byref(a))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_dense_purge")
        return b.as_dict(), a.as_dict()

    def dense_info(self):
        """esl_dense_info_get as a dict: n_samples, n_voxels, n_pairs, status, with_color, with_inst"""
        info = abi.EslDenseInfo()
        _check(load().esl_dense_info_get(self._h, C.byref(info)), "esl_dense_info_get")
        return info.as_dict()

    def dense_extract(self, cap=None, want=DENSE_OUTPUTS):
        """esl_dense_extract: the voxels in ascending packed-key order.  cap None = all of them.  Returns a dict: n_voxels (all of the
        map's, -1 when the map went over its capacity) and, per name of `want`, the first min(cap, n_voxels) rows: key (n, 3) int32,
        xyz (n, 3) float64, count (n,) int32, bgr (n, 3) uint8, inst (n,) int32, votes (n,) int32."""
        unknown = set(want) - set(self.DENSE_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        if cap is None:
            cap = max(self.dense_info()["n_voxels"], 0)
        cap = int(cap)
        shapes = dict(key=((cap, 3), np.int32), xyz=((cap, 3), np.float64), count=((cap,), np.int32), bgr=((cap, 3), np.uint8),
                      inst=((cap,), np.int32), votes=((cap,), np.int32))
        types = dict(key=C.c_int32, xyz=C.c_double, count=C.c_int32, bgr=C.c_uint8, inst=C.c_int32, votes=C.c_int32)
        out = {k: np.zeros(*shapes[k]) for k in self.DENSE_OUTPUTS if k in want}

        def optr(k):
            return out[k].ctypes.data_as(C.POINTER(types[k])) if k in out else None
        n = C.c_int64(0)
        t0 = time.perf_counter()
        rc = load().esl_dense_extract(self._h, cap, optr("key"), optr("xyz"), optr("count"), optr("bgr"), optr("inst"), optr("votes"),
                                      C.byref(n))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_dense_extract")
        m = min(cap, max(n.value, 0))
        res = {k: v[:m] for k, v in out.items()}
        res["n_voxels"] = int(n.value)
        return res

    def dense_objects(self, N, ground_world, params=None, comp_cap=None, voxel_cap=None):
        """esl_dense_objects: per label 0 .. N-1 of the dense map, the gravity-aligned ellipsoid that bounds the label's largest connected
        set of kept voxels.  comp_cap / voxel_cap None = room for the whole table / every voxel.  Returns a dict: result (the totals),
        objs (N, 10), stats (N, 6) int32, comp (min(comp_cap, n_components), 6) int32, voxel_comp (min(voxel_cap, n_voxels),) int32; on
        a map over its capacity (result n_voxels = -1) the arrays are empty."""
        N = int(N)
        g = np.ascontiguousarray(ground_world, dtype=np.float64).reshape(4)
        p = params if params is not None else abi.default_dense_obj_params()
        nv = max(self.dense_info()["n_voxels"], 0)
        comp_cap = nv if comp_cap is None else int(comp_cap)          # a table never has more rows than the map has voxels
        voxel_cap = nv if voxel_cap is None else int(voxel_cap)
        objs = np.zeros((max(N, 0), 10)); stats = np.zeros((max(N, 0), 6), np.int32)
        comp = np.zeros((max(comp_cap, 0), 6), np.int32); vox = np.zeros(max(voxel_cap, 0), np.int32)
        ip = C.POINTER(C.c_int32)
        res = abi.EslDenseObjResult()
        t0 = time.perf_counter()
        rc = load().esl_dense_objects(self._h, N, g.ctypes.data_as(_dp), C.byref(p), objs.ctypes.data_as(_dp) if objs.size else None,
                                      stats.ctypes.data_as(ip) if stats.size else None, comp_cap, comp.ctypes.data_as(ip) if comp.size else None,
                                      voxel_cap, vox.ctypes.data_as(ip) if vox.size else None, C.byref(res))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_dense_objects")
        r = res.as_dict()
        if r["n_voxels"] < 0:
            return dict(result=r, objs=objs[:0], stats=stats[:0], comp=comp[:0], voxel_comp=vox[:0])
        return dict(result=r, objs=objs, stats=stats, comp=comp[:min(comp_cap, r["n_components"])], voxel_comp=vox[:min(voxel_cap, r["n_voxels"])])

    def dense_planes(self, params=None, voxel_cap=None, hyp=False):
        """esl_dense_planes: the dominant planes of the dense map, one per round of a hypothesise-and-score search, and the ground among
        them when params.up is not zero.  voxel_cap None = room for every voxel; hyp: also return every hypothesis's row.  Returns a
        dict: result (the totals), planes (n_planes, 4), centroid (n_planes, 3), stats (n_planes, 8) int32, samples (n_planes,) int64,
        ground (4,), voxel_plane (min(voxel_cap, n_voxels),) int32, hyp (rounds, n_hypotheses, 3) int64 or None; on a map over its
        capacity (result n_voxels = -1) the arrays are empty."""
        p = params if params is not None else abi.default_dense_plane_params()
        P, Hn = max(int(p.max_planes), 0), max(int(p.n_hypotheses), 0)
        nv = max(self.dense_info()["n_voxels"], 0)
        voxel_cap = nv if voxel_cap is None else int(voxel_cap)
        planes = np.zeros((max(P, 1), 4)); cen = np.zeros((max(P, 1), 3)); stats = np.zeros((max(P, 1), 8), np.int32)
        smp = np.zeros(max(P, 1), np.int64); ground = np.zeros(4); vox = np.zeros(max(voxel_cap, 0), np.int32)
        hy = np.zeros((max(P, 1), max(Hn, 1), 3), np.int64) if hyp and 0 < P <= 64 and 0 < Hn <= 65536 else None
        ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        res = abi.EslDensePlaneResult()
        t0 = time.perf_counter()
        rc = load().esl_dense_planes(self._h, C.byref(p), planes.ctypes.data_as(_dp), cen.ctypes.data_as(_dp), stats.ctypes.data_as(ip),
                                     smp.ctypes.data_as(lp), ground.ctypes.data_as(_dp), voxel_cap, vox.ctypes.data_as(ip) if vox.size else None,
                                     hy.ctypes.data_as(lp) if hy is not None else None, C.byref(res))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_dense_planes")
        r = res.as_dict()
        if r["n_voxels"] < 0:
            return dict(result=r, planes=planes[:0], centroid=cen[:0], stats=stats[:0], samples=smp[:0], ground=ground, voxel_plane=vox[:0],
                        hyp=None if hy is None else hy[:0])
        m = r["n_planes"]
        return dict(result=r, planes=planes[:m], centroid=cen[:m], stats=stats[:m], samples=smp[:m], ground=ground,
                    voxel_plane=vox[:min(voxel_cap, r["n_voxels"])], hyp=None if hy is None else hy[:r["rounds"]])

    @staticmethod
    def dense_planes_layout():
        """esl_debug_dense_planes_layout: (entries of U_r per LDS tile, hypotheses per workgroup) of the score kernel"""
        t, g = C.c_int32(0), C.c_int32(0)
        _check(load().esl_debug_dense_planes_layout(C.byref(t), C.byref(g)), "esl_debug_dense_planes_layout")
        return t.value, g.value

    DENSE_RENDER_OUTPUTS = ("depth", "voxel", "bgr", "inst", "frame", "vox")

    def dense_render(self, cams, K, rows, cols, depth_meas=None, params=None, want=DENSE_RENDER_OUTPUTS, vox_cap=None):
        """esl_dense_render: the dense map's live voxels splatted into F frames, the nearest voxel kept per pixel, and the winners compared
        with a measured depth.  cams (F, 7) Tcw or None for the resident camera states; depth_meas (F, rows, cols) uint16 or None; want
        names the outputs to compute; vox_cap None = room for every voxel.  Returns a dict: result (status, n_voxels, n_small,
        n_chunks) and, per name of want, depth (F, rows, cols) NaN where no voxel is drawn, voxel (F, rows, cols) index in
        dense_extract's order or -1, bgr (F, rows, cols, 3) uint8, inst (F, rows, cols) label or -1, frame (F, 8) int32 n_drawn /
        n_depth_out / n_outside / covered / agree / nearer / farther / no data, vox (min(vox_cap, n_voxels), 4) int32 won / agree /
        nearer / farther; on an invalid map (result n_voxels = -1) the arrays are as they were allocated and vox is empty."""
        p = params if params is not None else abi.default_dense_render_params()
        want = set(want)
        unknown = want - set(self.DENSE_RENDER_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        _ip, _up, _bp = C.POINTER(C.c_int32), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)
        if cams is None:
            F, cp = self.graph_sizes()["n_cams"], None
        else:
            cams = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, 7)
            F, cp = len(cams), (cams.ctypes.data_as(_dp) if len(cams) else None)
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        rows, cols = int(rows), int(cols)
        mp = None
        if depth_meas is not None:
            depth_meas = np.ascontiguousarray(depth_meas, dtype=np.uint16)
            if depth_meas.shape != (F, rows, cols):
                raise ValueError(f"depth_meas has shape {depth_meas.shape}, expected {(F, rows, cols)}")
            mp = depth_meas.ctypes.data_as(_up)          # an empty array has a valid address too
        r, c = (rows, cols) if rows > 0 and cols > 0 else (0, 0)          # the library refuses such a shape before it writes
        out = {}
        if "depth" in want:
            out["depth"] = np.full((F, r, c), np.nan)
        if "voxel" in want:
            out["voxel"] = np.full((F, r, c), -1, dtype=np.int32)
        if "bgr" in want:
            out["bgr"] = np.zeros((F, r, c, 3), dtype=np.uint8)
        if "inst" in want:
            out["inst"] = np.full((F, r, c), -1, dtype=np.int32)
        if "frame" in want:
            out["frame"] = np.zeros((F, 8), dtype=np.int32)
        if "vox" in want:
            if vox_cap is None:
                vox_cap = max(self.dense_info()["n_voxels"], 0) if self._dense_begun() else 0
            vox_cap = int(vox_cap)
            out["vox"] = np.zeros((max(vox_cap, 0), 4), dtype=np.int32)
        else:
            vox_cap = 0

        def optr(k, t):
            return out[k].ctypes.data_as(t) if k in out and out[k].size else None
        res = abi.EslDenseRenderResult()
        t0 = time.perf_counter()
        rc = load().esl_dense_render(self._h, cp, F, Kc.ctypes.data_as(_dp), rows, cols, mp, C.byref(p), optr("depth", _dp),
                                     optr("voxel", _ip), optr("bgr", _bp), optr("inst", _ip), optr("frame", _ip), vox_cap,
                                     optr("vox", _ip), C.byref(res))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_dense_render")
        out["result"] = res.as_dict()
        if "vox" in out:
            out["vox"] = out["vox"][:min(vox_cap, max(res.n_voxels, 0))]
        return out

    def dense_normals(self, params=None, cap=None):
        """esl_dense_normals: per live voxel, in dense_extract's order, the unit normal of its neighbourhood's centroids.  cap None = room
        for every voxel.  Returns a dict: result (status, n_voxels, n_eligible, n_valid) and the first min(cap, n_voxels) rows of normal
        (n, 3) (zero where invalid), curvature (n,) (NaN where invalid), neighbors (n,) int32 and valid (n,) uint8; on an invalid map
        (result n_voxels = -1) the arrays are empty."""
        p = params if params is not None else abi.default_dense_normal_params()
        if cap is None:
            cap = max(self.dense_info()["n_voxels"], 0) if self._dense_begun() else 0
        cap = int(cap)
        m = max(cap, 0)
        nrm = np.zeros((m, 3)); curv = np.full(m, np.nan); nb = np.zeros(m, np.int32); val = np.zeros(m, np.uint8)
        res = abi.EslDenseNormalResult()
        t0 = time.perf_counter()
        rc = load().esl_dense_normals(self._h, C.byref(p), cap, nrm.ctypes.data_as(_dp) if m else None, curv.ctypes.data_as(_dp) if m else None,
                                      nb.ctypes.data_as(C.POINTER(C.c_int32)) if m else None,
                                      val.ctypes.data_as(C.POINTER(C.c_uint8)) if m else None, C.byref(res))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_dense_normals")
        n = min(m, max(res.n_voxels, 0))
        return dict(result=res.as_dict(), normal=nrm[:n], curvature=curv[:n], neighbors=nb[:n], valid=val[:n])

    def dense_align_frames(self, cams, K, rows, cols, depth, params=None, iters_out=True):
        """esl_dense_align_frames: refine the poses of F depth frames against the dense map (point-to-plane Gauss-Newton on the voxels'
        centroids and normals).  cams (F, 7) Tcw, the start poses, or None for the resident camera states; depth (F, rows, cols) uint16.
        Returns a dict: result (status, n_voxels, n_valid, n_passes), cams (F, 7) the final poses, status / iters (F,) int32 (status 0 all
        steps taken, 1 converged, 2 too few inliers, 3 degenerate), counts (F, 8) int64 in abi.DENSE_ALIGN_COUNTS' order, sum_e2 (F,),
        H (F, 6, 6), step (F, 2) = |v|, |omega| of the last step, and with iters_out sums (F, iters + 1, 37) int64, a frame's words per
        pass; on an invalid map (result n_voxels = -1) nothing was written and the arrays are as they were allocated."""
        p = params if params is not None else abi.default_dense_align_params()
        if cams is None:
            F, cp = self.graph_sizes()["n_cams"], None
        else:
            cams = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, 7)
            F, cp = len(cams), (cams.ctypes.data_as(_dp) if len(cams) else None)
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        rows, cols = int(rows), int(cols)
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        if depth.shape != (F, rows, cols):
            raise ValueError(f"depth has shape {depth.shape}, expected {(F, rows, cols)}")
        cams_out = np.zeros((F, 7))
        fr = (abi.EslDenseAlignFrame * max(F, 1))()
        sums = np.zeros((F, max(int(p.iters), 0) + 1, abi.DENSE_ALIGN_ROW), np.int64) if iters_out else None
        res = abi.EslDenseAlignResult()
        t0 = time.perf_counter()
        rc = load().esl_dense_align_frames(self._h, cp, F, Kc.ctypes.data_as(_dp), rows, cols,
                                           depth.ctypes.data_as(C.POINTER(C.c_uint16)) if F else None, C.byref(p),
                                           cams_out.ctypes.data_as(_dp) if F else None, fr if F else None,
                                           sums.ctypes.data_as(C.POINTER(C.c_int64)) if sums is not None and sums.size else None, C.byref(res))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_dense_align_frames")
        out = dict(result=res.as_dict(), cams=cams_out,
                   status=np.array([fr[f].status for f in range(F)], np.int32), iters=np.array([fr[f].iters for f in range(F)], np.int32),
                   counts=np.array([[getattr(fr[f], k) for k in abi.DENSE_ALIGN_COUNTS] for f in range(F)], np.int64).reshape(F, 8),
                   sum_e2=np.array([fr[f].sum_e2 for f in range(F)], np.float64),
                   H=np.array([list(fr[f].H) for f in range(F)], np.float64).reshape(F, 6, 6),
                   step=np.array([[fr[f].step_t, fr[f].step_r] for f in range(F)], np.float64).reshape(F, 2))
        if sums is not None:
            out["sums"] = sums
        return out

    DENSE_CARVE_OUTPUTS = ("vox", "carved", "obs", "depth_kept", "mask", "own")

    def dense_carve_frames(self, cams_obs, depth_obs, cams_own, depth_own, K, rows, cols, bgr_own=None, inst_own=None, params=None,
                           want=DENSE_CARVE_OUTPUTS, vox_cap=None):
        """esl_dense_carve_frames: which live voxels of the dense map do the observer frames see through, which samples of the owner
        frames lie in them, and (params.apply = 1) their removal.  cams_obs (F_obs, 7) Tcw or None for the resident camera states,
        depth_obs (F_obs, rows, cols) uint16; cams_own (F_own, 7), depth_own / bgr_own / inst_own as the owners were added; want names
        the outputs to compute; vox_cap None = room for every voxel.  Returns a dict: result (status, n_voxels, n_tested, n_carved,
        samples_found, samples_carved, removed) and, per name of want, vox (min(vox_cap, n_voxels), 4) int32 agree / nearer / through /
        no data, carved (min(vox_cap, n_voxels),) uint8, obs (F_obs, 8) int32 in view / depth out / outside / agree / nearer / through /
        no data / 0, depth_kept (F_own, rows, cols) uint16, mask (F_own, rows, cols) uint8, own (F_own, 4) int32 used / found / carved /
        not found; on an invalid map (result n_voxels = -1) the arrays are as they were allocated and vox, carved are empty."""
        p = params if params is not None else abi.default_dense_carve_params()
        want = set(want)
        unknown = want - set(self.DENSE_CARVE_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        _ip, _up, _bp = C.POINTER(C.c_int32), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)
        rows, cols = int(rows), int(cols)
        if cams_obs is None:
            Fo, cop = self.graph_sizes()["n_cams"], None
        else:
            cams_obs = np.ascontiguousarray(cams_obs, dtype=np.float64).reshape(-1, 7)
            Fo, cop = len(cams_obs), (cams_obs.ctypes.data_as(_dp) if len(cams_obs) else None)
        cams_own = np.ascontiguousarray(np.zeros((0, 7)) if cams_own is None else cams_own, dtype=np.float64).reshape(-1, 7)
        Fw = len(cams_own)

        def img(a, F, dt, t, what, tail=()):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape != (F, rows, cols) + tail:
                raise ValueError(f"{what} has shape {a.shape}, expected {(F, rows, cols) + tail}")
            return a, a.ctypes.data_as(t)          # an empty array has a valid address too
        depth_obs, dop = img(depth_obs, Fo, np.uint16, _up, "depth_obs")
        depth_own, dwp = img(depth_own, Fw, np.uint16, _up, "depth_own")
        bgr_own, bwp = img(bgr_own, Fw, np.uint8, _bp, "bgr_own", (3,))
        inst_own, iwp = img(inst_own, Fw, np.int32, _ip, "inst_own")
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        r, c = (rows, cols) if rows > 0 and cols > 0 else (0, 0)          # the library refuses such a shape before it writes
        if "vox" in want or "carved" in want:
            if vox_cap is None:
                vox_cap = max(self.dense_info()["n_voxels"], 0) if self._dense_begun() else 0
            vox_cap = int(vox_cap)
        else:
            vox_cap = 0
        out = {}
        if "vox" in want:
            out["vox"] = np.zeros((max(vox_cap, 0), 4), dtype=np.int32)
        if "carved" in want:
            out["carved"] = np.zeros(max(vox_cap, 0), dtype=np.uint8)
        if "obs" in want:
            out["obs"] = np.zeros((Fo, 8), dtype=np.int32)
        if "depth_kept" in want:
            out["depth_kept"] = np.zeros((Fw, r, c), dtype=np.uint16)
        if "mask" in want:
            out["mask"] = np.zeros((Fw, r, c), dtype=np.uint8)
        if "own" in want:
            out["own"] = np.zeros((Fw, 4), dtype=np.int32)

        def optr(k, t):
            return out[k].ctypes.data_as(t) if k in out and out[k].size else None
        res = abi.EslDenseCarveResult()
        t0 = time.perf_counter()
        rc = load().esl_dense_carve_frames(self._h, cop, Fo, dop, cams_own.ctypes.data_as(_dp) if Fw else None, Fw, dwp, bwp, iwp,
                                           Kc.ctypes.data_as(_dp), rows, cols, C.byref(p), vox_cap, optr("vox", _ip), optr("carved", _bp),
                                           optr("obs", _ip), optr("depth_kept", _up), optr("mask", _bp), optr("own", _ip), C.byref(res))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_dense_carve_frames")
        out["result"] = res.as_dict()
        m = min(vox_cap, max(res.n_voxels, 0))
        for k in ("vox", "carved"):
            if k in out:
                out[k] = out[k][:m]
        return out

    DENSE_COVIS_OUTPUTS = ("vox", "frame", "pair")

    def dense_covis_frames(self, cams, depth, K, rows, cols, keep=None, params=None, want=DENSE_COVIS_OUTPUTS, vox_cap=None):
        """esl_dense_covis_frames: which voxels of the dense map does each frame see, how many do two frames share, which frames are
        redundant.  cams (F, 7) Tcw or None for the resident camera states, depth (F, rows, cols) uint16, keep (F,) non-zero = never
        culled, or None; want names the outputs to compute; vox_cap None = room for every voxel.  Returns a dict: result (status,
        n_voxels, n_seen, n_culled, sum_seen, sum_pairs) and, per name of want, vox (min(vox_cap, n_voxels),) int32 k_i, frame (F, 8)
        int32 in view / depth out / outside / seen / covered / unique / cull round / 0, pair (F, F) int32; on an invalid map (result
        n_voxels = -1) the arrays are as they were allocated and vox is empty."""
        p = params if params is not None else abi.default_dense_covis_params()
        want = set(want)
        unknown = want - set(self.DENSE_COVIS_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        _ip, _up, _bp = C.POINTER(C.c_int32), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)
        rows, cols = int(rows), int(cols)
        if cams is None:
            F, cp = self.graph_sizes()["n_cams"], None
        else:
            cams = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, 7)
            F, cp = len(cams), (cams.ctypes.data_as(_dp) if len(cams) else None)
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        if depth.shape != (F, rows, cols):
            raise ValueError(f"depth has shape {depth.shape}, expected {(F, rows, cols)}")
        kp = None
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.uint8).reshape(-1)
            if len(keep) != F:
                raise ValueError(f"keep has {len(keep)} entries, expected {F}")
            kp = keep.ctypes.data_as(_bp)
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        if "vox" in want:
            if vox_cap is None:
                vox_cap = max(self.dense_info()["n_voxels"], 0) if self._dense_begun() else 0
            vox_cap = int(vox_cap)
        else:
            vox_cap = 0
        out = {}
        if "vox" in want:
            out["vox"] = np.zeros(max(vox_cap, 0), dtype=np.int32)
        if "frame" in want:
            out["frame"] = np.zeros((F, 8), dtype=np.int32)
        if "pair" in want:
            out["pair"] = np.zeros((F, F), dtype=np.int32)

        def optr(k):
            return out[k].ctypes.data_as(_ip) if k in out and out[k].size else None
        res = abi.EslDenseCovisResult()
        t0 = time.perf_counter()
        rc = load().esl_dense_covis_frames(self._h, cp, F, depth.ctypes.data_as(_up), kp, Kc.ctypes.data_as(_dp), rows, cols, C.byref(p), vox_cap,
                                           optr("vox"), optr("frame"), optr("pair"), C.byref(res))
        self.last_call_s = time.perf_counter() - t0      # the C-ABI call alone
        _check(rc, "esl_dense_covis_frames")
        out["result"] = res.as_dict()
        if "vox" in out:
            out["vox"] = out["vox"][:min(vox_cap, max(res.n_voxels, 0))]
        return out

    def _dense_begun(self):
        """whether esl_dense_info_get answers, i.e. a map was begun on this context"""
        return load().esl_dense_info_get(self._h, C.byref(abi.EslDenseInfo())) == 0

    def dense_end(self):
        """esl_dense_end: forget the map (the buffers stay with the context)"""
        _check(load().esl_dense_end(self._h), "esl_dense_end")

    def dense_allocs(self):
        """esl_debug_dense_allocs: (device allocations the dense calls have made on this context, bytes their buffers hold)"""
        n, b = C.c_int64(0), C.c_int64(0)
        _check(load().esl_debug_dense_allocs(self._h, C.byref(n), C.byref(b)), "esl_debug_dense_allocs")
        return n.value, b.value

    def selftest_cholesky(self, n):
        """(ms, relative residual) of the dense FP64-MFMA Cholesky factor + solve on a generated SPD system."""
        ms, res = C.c_double(0), C.c_double(0)
        _check(load().esl_selftest_cholesky(self._h, C.c_int32(n), C.byref(ms), C.byref(res)), "esl_selftest_cholesky")
        return ms.value, res.value

    def comm_init(self, n_ranks, rank, unique_id):
        """Join the RCCL communicator; afterwards optimize_resident() is collective over all ranks."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _check(load().esl_comm_init(self._h, C.c_int32(n_ranks), C.c_int32(rank), buf), "esl_comm_init")

    def comm_init_host(self, n_ranks, rank, allreduce):
        """Collective mode over a host-supplied transport: allreduce(np.ndarray float64) sums in place over ranks."""
        def _cb(_user, buf, count):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(count,)))
                return 0
            except Exception:   # an exception must not unwind through the C frames
                import traceback; traceback.print_exc()
                return 1
        self._host_cb = HOST_ALLREDUCE_FN(_cb)   # keep alive as long as the context uses it
        _check(load().esl_comm_init_host(self._h, C.c_int32(n_ranks), C.c_int32(rank), self._host_cb, None), "esl_comm_init_host")

    def comm_set_replicated(self, on=True):
        """Every rank holds the whole graph; the ranks divide the dense solve of SLAM mode (esl_comm_set_replicated)."""
        _check(load().esl_comm_set_replicated(self._h, C.c_int(1 if on else 0)), "esl_comm_set_replicated")

    def comm_destroy(self):
        _check(load().esl_comm_destroy(self._h), "esl_comm_destroy")

    def synchronize(self):
        _check(load().esl_ctx_synchronize(self._h), "esl_ctx_synchronize")

    def trim(self):
        """Release the grow-only solver blobs of SLAM mode (esl_ctx_trim); they are rebuilt on demand."""
        _check(load().esl_ctx_trim(self._h), "esl_ctx_trim")


class _Sizes:
    """vertex counts of a resident graph that has been extended by append_graph (download_states needs them)"""

    def __init__(self, n_cams, n_objs):
        self.n_cams, self.n_objs = n_cams, n_objs


HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)


def comm_unique_id():
    buf = C.create_string_buffer(128)
    _check(load().esl_comm_unique_id(buf), "esl_comm_unique_id")
    return bytes(buf.raw)


def default_fit_params(**kw):
    """Reference settings (Example/param/TUM3.yaml, PointCloudFilter.cpp:31-38, EllipsoidExtractor.cpp:98,570)."""
    p = abi.EslFitParams()
    load().esl_fit_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def chol_plan(n, W, filler=128):
    """The persistent dense factorisation's static task list for an order-n system (esl_debug_chol_plan; host only):
    dict(np, n_outer, nR, W, tasks (n_tasks, 4) int32 {type, a, b, c}, ns (np, nR) int32)."""
    meta = (C.c_int32 * 5)()
    ip = C.POINTER(C.c_int32)
    _check(load().esl_debug_chol_plan(C.c_int32(n), C.c_int32(W), C.c_int32(filler), ip(), C.c_int64(0), ip(), C.c_int64(0), meta), "esl_debug_chol_plan")
    np_, n_outer, nR, n_tasks, W_ = [int(v) for v in meta]
    tasks = np.zeros((max(n_tasks, 1), 4), dtype=np.int32); ns = np.zeros((np_, nR), dtype=np.int32)
    _check(load().esl_debug_chol_plan(C.c_int32(n), C.c_int32(W), C.c_int32(filler), tasks.ctypes.data_as(ip), C.c_int64(n_tasks),
                                      ns.ctypes.data_as(ip), C.c_int64(ns.size), meta), "esl_debug_chol_plan")
    return dict(np=np_, n_outer=n_outer, nR=nR, W=W_, tasks=tasks[:n_tasks], ns=ns)


def update_v_applies(lda, rows, base, col_limit, ext=True, ldp=None):
    """Would the rank-K update of rows [base, rows) x columns [base, col_limit) run on k_chol_update_v (esl_debug_update_v_applies;
    host only)?"""
    out = C.c_int32(0)
    _check(load().esl_debug_update_v_applies(C.c_int64(lda), C.c_int64(rows), C.c_int64(base), C.c_int64(col_limit), C.c_int32(1 if ext else 0),
                                             C.c_int64(lda if ldp is None else ldp), C.byref(out)), "esl_debug_update_v_applies")
    return bool(out.value)


def cf_stride_choose(n_o, upd_flops, pairs, slab):
    """The camera segment length (16, 32 or 48) the camera-first layout chooses for its one-sided assembly of T from a graph's counts
    at the three lengths, and the cost model's ms per trial for each (esl_debug_cf_stride_choose; host only)."""
    arr = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    out, ms = C.c_int32(0), (C.c_double * 3)()
    _check(load().esl_debug_cf_stride_choose(C.c_int64(n_o), arr(upd_flops), arr(pairs), arr(slab), C.byref(out), ms), "esl_debug_cf_stride_choose")
    return int(out.value), [float(x) for x in ms]


def partition_objects(graph, n_parts):
    """Host-only balanced partition of ellipsoids over shards (works without a GPU)."""
    g = graph.c_struct()
    out = np.zeros(graph.n_objs, dtype=np.int32)
    _check(load().esl_partition_objects(C.byref(g), C.c_int32(n_parts), out.ctypes.data_as(C.POINTER(C.c_int32))),
           "esl_partition_objects")
    return out
