"""ctypes mirror of include/esl.h (the C-ABI of the MI355X backend).

Only plain-old-data layouts live here.  The product binding (lib.py) builds its argument structs
from these classes; the test-only CPU checker reuses the same layouts so that both sides of a
parity test are always called with byte-identical inputs.
"""
import ctypes as C

import numpy as np

ESL_MAX_TRACE = 32
ESL_OS_COUNTS = 6   # esl_lm_os_counts

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)


class EslGraph(C.Structure):
    _fields_ = [
        ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
        ("n_cams", C.c_int32), ("n_objs", C.c_int32),
        ("cam_fixed", c_uint8_p),
        ("n_bbox", C.c_int32), ("bbox_cam", c_int32_p), ("bbox_obj", c_int32_p),
        ("bbox_meas", c_double_p), ("bbox_weight", c_double_p),
        ("n_e3d", C.c_int32), ("e3d_cam", c_int32_p), ("e3d_obj", c_int32_p),
        ("e3d_meas", c_double_p), ("e3d_weight", c_double_p),
        ("n_grav", C.c_int32), ("grav_obj", c_int32_p),
        ("grav_normal", C.c_double * 4), ("grav_weight", C.c_double),
        ("n_odom", C.c_int32), ("odom_i", c_int32_p), ("odom_j", c_int32_p),
        ("odom_meas", c_double_p), ("odom_info", c_double_p),
        ("check_visibility", C.c_int32), ("image_rows", C.c_int32), ("image_cols", C.c_int32),
    ]


class EslGraphDelta(C.Structure):
    """esl_graph_delta: what one new frame adds to the resident graph (esl_graph_append)."""
    _fields_ = [
        ("n_new_cams", C.c_int32), ("new_cams", c_double_p), ("n_new_objs", C.c_int32), ("new_objs", c_double_p),
        ("n_bbox", C.c_int32), ("bbox_cam", c_int32_p), ("bbox_obj", c_int32_p), ("bbox_meas", c_double_p), ("bbox_weight", c_double_p),
        ("n_e3d", C.c_int32), ("e3d_cam", c_int32_p), ("e3d_obj", c_int32_p), ("e3d_meas", c_double_p), ("e3d_weight", c_double_p),
        ("n_grav", C.c_int32), ("grav_obj", c_int32_p),
        ("new_cam_fixed", C.POINTER(C.c_uint8)), ("n_odom", C.c_int32), ("odom_i", c_int32_p), ("odom_j", c_int32_p),
        ("odom_meas", c_double_p), ("odom_info", c_double_p),
    ]


class EslLmParams(C.Structure):
    _fields_ = [
        ("max_iters", C.c_int32), ("max_trials", C.c_int32), ("tau", C.c_double),
        ("jacobian_mode", C.c_int32), ("numeric_delta", C.c_double),
        ("linear_solver", C.c_int32), ("drop_nan_bbox", C.c_int32), ("bbox_residual", C.c_int32), ("e3d_half_turn", C.c_int32),
    ]


class EslLmReport(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32), ("total_trials", C.c_int32),
        ("n_bbox_valid", C.c_int32), ("n_bbox_dropped", C.c_int32), ("stop_reason", C.c_int32),
        ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double),
        ("trace_len", C.c_int32),
        ("trace_chi2", C.c_double * ESL_MAX_TRACE), ("trace_lambda", C.c_double * ESL_MAX_TRACE),
        ("trace_trials", C.c_int32 * ESL_MAX_TRACE),
    ]

    def as_dict(self):
        n = self.trace_len
        return dict(iterations=self.iterations, total_trials=self.total_trials,
                    n_bbox_valid=self.n_bbox_valid, n_bbox_dropped=self.n_bbox_dropped,
                    stop_reason=self.stop_reason, chi2_initial=self.chi2_initial,
                    chi2_final=self.chi2_final, lambda_final=self.lambda_final,
                    trace_chi2=list(self.trace_chi2[:n]), trace_lambda=list(self.trace_lambda[:n]),
                    trace_trials=list(self.trace_trials[:n]))


class EslLmPartials(C.Structure):
    _fields_ = [("chi2", C.c_double), ("max_diag", C.c_double), ("scale", C.c_double),
                ("solve_ok", C.c_int32), ("pad", C.c_int32)]


class EslFitParams(C.Structure):
    _fields_ = [
        ("stride", C.c_int32), ("depth_scale", C.c_double), ("depth_min", C.c_double),
        ("depth_max", C.c_double), ("voxel_leaf", C.c_double), ("plane_dist", C.c_double),
        ("cluster_tolerance", C.c_double), ("min_cluster_size", C.c_int32), ("center_dis", C.c_double),
        ("symmetry_open", C.c_int32), ("symmetry_grid", C.c_double), ("symmetry_sigma", C.c_double),
        ("symmetry_lm_iters", C.c_int32),
    ]


class EslFitSymmetry(C.Structure):
    """SymmetryOutputData (reference src/symmetry/Symmetry.h:16-32) as esl_fit_frame_ex returns it."""
    _fields_ = [("result", C.c_int32), ("symmetry_type", C.c_int32), ("plane", C.c_double * 4),
                ("plane2", C.c_double * 4), ("prob", C.c_double), ("center", C.c_double * 3)]


class EslPlaneParams(C.Structure):
    """esl_plane_params (PlaneExtractorParam + the PCL constants of PlaneExtractor.cpp:57-58, 74)."""
    _fields_ = [("min_size", C.c_int32), ("angle_threshold_deg", C.c_double), ("distance_threshold", C.c_double),
                ("normal_smoothing", C.c_int32), ("max_depth_change_factor", C.c_double), ("min_inliers", C.c_int32),
                ("refine", C.c_int32), ("refine_distance", C.c_double), ("max_curvature", C.c_double)]


def default_plane_params(**kw):
    """Example/param/TUM3.yaml:36-38 + PlaneExtractor.cpp:57-58, 74."""
    p = EslPlaneParams(min_size=200, angle_threshold_deg=5.0, distance_threshold=0.1, normal_smoothing=10,
                       max_depth_change_factor=0.05, min_inliers=100, refine=1, refine_distance=0.02, max_curvature=0.001)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


SOLVER_AUTO, SOLVER_REDUCED_CAMERA, SOLVER_REDUCED_ELLIPSOID, SOLVER_CAMERA_CHAIN, SOLVER_PCG = 0, 1, 2, 3, 4   # esl_linear_solver (include/esl.h)


class EslPcgParams(C.Structure):
    """esl_pcg_params: settings of ESL_SOLVER_PCG (esl_lm_set_pcg)."""
    _fields_ = [("max_iters", C.c_int32), ("check_every", C.c_int32), ("rel_tol", C.c_double)]


def default_pcg_params():
    """esl_pcg_params_default: 1000 iterations, a host look at the done flag every 8, rel_tol 1e-10."""
    return EslPcgParams(max_iters=1000, check_every=8, rel_tol=1e-10)


class EslRelocParams(C.Structure):
    """esl_reloc_params: gates and switches of esl_relocalize."""
    _fields_ = [("center_tol", C.c_double), ("height_tol", C.c_double), ("size_ratio", C.c_double), ("min_baseline", C.c_double),
                ("min_inliers", C.c_int32), ("max_candidates", C.c_int32), ("match_labels", C.c_int32), ("refine", C.c_int32)]


class EslRelocResult(C.Structure):
    """esl_reloc_result: what esl_relocalize found (status 0) or why it found nothing (1 - 3)."""
    _fields_ = [("status", C.c_int32), ("n_candidates", C.c_int32), ("n_hypotheses", C.c_int64), ("best_key", C.c_int64),
                ("n_inliers", C.c_int32), ("refined", C.c_int32), ("cost", C.c_double), ("yaw", C.c_double), ("tx", C.c_double),
                ("ty", C.c_double), ("Twc", C.c_double * 7)]

    def as_dict(self):
        return dict(status=self.status, n_candidates=self.n_candidates, n_hypotheses=self.n_hypotheses, best_key=self.best_key,
                    n_inliers=self.n_inliers, refined=self.refined, cost=self.cost, yaw=self.yaw, tx=self.tx, ty=self.ty,
                    Twc=np.array(list(self.Twc)))


def default_reloc_params(**kw):
    """esl_reloc_params_default: design choices, not values tuned on real data (include/esl.h)."""
    p = EslRelocParams(center_tol=0.25, height_tol=0.25, size_ratio=1.5, min_baseline=0.5, min_inliers=3, max_candidates=4096,
                       match_labels=1, refine=1)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class EslAssocParams(C.Structure):
    """esl_assoc_params: gates and switches of esl_predict_boxes / esl_associate_boxes."""
    _fields_ = [("min_iou", C.c_double), ("occl_ratio", C.c_double), ("min_box_px", C.c_double), ("match_labels", C.c_int32),
                ("occlusion", C.c_int32)]


def default_assoc_params(**kw):
    """esl_assoc_params_default (include/esl.h)."""
    p = EslAssocParams(min_iou=0.3, occl_ratio=0.7, min_box_px=10.0, match_labels=1, occlusion=1)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class EslInitRobustParams(C.Structure):
    """esl_init_robust_params: the hypothesise-and-score search of esl_init_quadrics_robust."""
    _fields_ = [("sample_size", C.c_int32), ("n_hypotheses", C.c_int32), ("inlier_px", C.c_double), ("min_inliers", C.c_int32),
                ("refine", C.c_int32), ("seed", C.c_uint64)]


def default_init_robust_params(**kw):
    """esl_init_robust_params_default: design choices, not values tuned on real data (include/esl.h)."""
    p = EslInitRobustParams(sample_size=5, n_hypotheses=64, inlier_px=10.0, min_inliers=8, refine=1, seed=0)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class EslMergeParams(C.Structure):
    """esl_merge_params: the lattice and the thresholds of esl_map_overlaps / esl_map_merge."""
    _fields_ = [("lattice", C.c_int32), ("match_labels", C.c_int32), ("min_iou", C.c_double), ("min_contain", C.c_double),
                ("max_pairs", C.c_int32), ("pad", C.c_int32)]


class EslMergeResult(C.Structure):
    """esl_merge_result: what esl_map_merge did (status 0), or that it did nothing (3: more candidates than max_pairs)."""
    _fields_ = [("status", C.c_int32), ("n_valid", C.c_int32), ("n_groups", C.c_int32), ("n_merged_groups", C.c_int32),
                ("largest_group", C.c_int32), ("n_conflicts", C.c_int32), ("n_candidates", C.c_int64), ("n_pairs", C.c_int64),
                ("n_links", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def default_merge_params(**kw):
    """esl_merge_params_default: design choices, not values tuned on real data (include/esl.h)."""
    p = EslMergeParams(lattice=16, match_labels=1, min_iou=0.3, min_contain=0.7, max_pairs=4194304, pad=0)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class EslRenderParams(C.Structure):
    """esl_render_params: how esl_render_map reads a measured depth image."""
    _fields_ = [("depth_scale", C.c_double), ("depth_min", C.c_double), ("depth_max", C.c_double), ("depth_tol", C.c_double)]


def default_render_params(**kw):
    """esl_render_params_default: design choices, not values tuned on real data (include/esl.h)."""
    p = EslRenderParams(depth_scale=5000.0, depth_min=0.1, depth_max=6.0, depth_tol=0.05)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def render_argtypes(L):
    """esl_render_map takes fifteen arguments, most of them nullable pointers: declared, so that None passes as NULL and a wrong type
    raises instead of reaching the library"""
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.esl_render_params_default.argtypes = [C.POINTER(EslRenderParams)]
    L.esl_render_params_default.restype = None
    L.esl_render_map.argtypes = [C.c_void_p, dp, C.c_int32, dp, C.c_int32, dp, C.c_int32, C.c_int32, C.POINTER(C.c_uint16),
                                 C.POINTER(EslRenderParams), dp, ip, ip, ip, ip]
    L.esl_render_map.restype = C.c_int


class EslDenseParams(C.Structure):
    """esl_dense_params: the voxel grid and the depth gate of the dense map (esl_dense_begin)."""
    _fields_ = [("leaf", C.c_double), ("depth_scale", C.c_double), ("depth_min", C.c_double), ("depth_max", C.c_double),
                ("stride", C.c_int32), ("max_voxels", C.c_int32)]


class EslDenseAddResult(C.Structure):
    """esl_dense_add_result: one esl_dense_add_frames call's counts; status 3 = the map went over its capacity."""
    _fields_ = [("n_sampled", C.c_int64), ("n_zero", C.c_int64), ("n_depth_out", C.c_int64), ("n_key_out", C.c_int64),
                ("n_used", C.c_int64), ("status", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


class EslDenseInfo(C.Structure):
    """esl_dense_info: the dense map so far."""
    _fields_ = [("n_samples", C.c_int64), ("n_voxels", C.c_int32), ("n_pairs", C.c_int32), ("status", C.c_int32),
                ("with_color", C.c_int32), ("with_inst", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


class EslDenseRemoveResult(C.Structure):
    """esl_dense_remove_result: one esl_dense_remove_frames call's counts; status 4 = the map is inconsistent."""
    _fields_ = [("n_sampled", C.c_int64), ("n_zero", C.c_int64), ("n_depth_out", C.c_int64), ("n_key_out", C.c_int64),
                ("n_used", C.c_int64), ("n_missing", C.c_int64), ("n_emptied", C.c_int64), ("status", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


class EslDenseMoveResult(C.Structure):
    """esl_dense_move_result: the removal's and the add's counts of one esl_dense_move_frames call, and the frames moved / skipped."""
    _fields_ = [("removed", EslDenseRemoveResult), ("added", EslDenseAddResult), ("n_frames_moved", C.c_int32), ("n_frames_same", C.c_int32)]

    def as_dict(self):
        return dict(removed=self.removed.as_dict(), added=self.added.as_dict(), n_frames_moved=int(self.n_frames_moved),
                    n_frames_same=int(self.n_frames_same))


class EslDenseSlots(C.Structure):
    """esl_dense_slots: the claimed slots of the voxel and the pair table and the dead among them."""
    _fields_ = [("voxel_slots", C.c_int64), ("dead_voxels", C.c_int64), ("pair_slots", C.c_int64), ("dead_pairs", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(EslDenseRemoveResult) == 64 and C.sizeof(EslDenseMoveResult) == 120 and C.sizeof(EslDenseSlots) == 32


def default_dense_params(**kw):
    """esl_dense_params_default: the reference's 1 cm leaf and depth gate; stride and max_voxels are design choices (include/esl.h)."""
    p = EslDenseParams(leaf=0.01, depth_scale=5000.0, depth_min=0.5, depth_max=6.0, stride=1, max_voxels=1048576)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class EslDenseObjParams(C.Structure):
    """esl_dense_obj_params: the gates, the reach and the table limits of esl_dense_objects."""
    _fields_ = [("reach", C.c_int32), ("min_votes", C.c_int32), ("min_count", C.c_int32), ("min_component", C.c_int32),
                ("max_components", C.c_int32), ("pad", C.c_int32), ("plane_dist", C.c_double)]


class EslDenseObjResult(C.Structure):
    """esl_dense_obj_result: the totals of one esl_dense_objects call; status 3 = more table rows than max_components, or a map over
    its capacity (n_voxels = -1)."""
    _fields_ = [("status", C.c_int32), ("n_voxels", C.c_int32), ("n_in_range", C.c_int32), ("n_gated", C.c_int32), ("n_kept", C.c_int32),
                ("n_components_all", C.c_int32), ("n_components", C.c_int32), ("n_ok", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def default_dense_obj_params(**kw):
    """esl_dense_obj_params_default (include/esl.h)"""
    p = EslDenseObjParams(reach=2, min_votes=1, min_count=1, min_component=100, max_components=65536, pad=0, plane_dist=0.05)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class EslDensePlaneParams(C.Structure):
    """esl_dense_plane_params: the inlier tolerance, the up direction, the search's sizes and the gates of esl_dense_planes."""
    _fields_ = [("dist_tol", C.c_double), ("up", C.c_double * 3), ("up_min_cos", C.c_double), ("n_hypotheses", C.c_int32),
                ("max_planes", C.c_int32), ("min_inliers", C.c_int32), ("min_baseline", C.c_int32), ("min_count", C.c_int32),
                ("skip_labelled", C.c_int32), ("refine", C.c_int32), ("pad", C.c_int32), ("seed", C.c_uint64)]


class EslDensePlaneResult(C.Structure):
    """esl_dense_plane_result: the totals of one esl_dense_planes call; status 3 = a map over its capacity (n_voxels = -1);
    stop_reason 0 max_planes reported, 1 fewer than three voxels left, 2 no valid hypothesis, 3 the best plane below min_inliers."""
    _fields_ = [("status", C.c_int32), ("n_voxels", C.c_int32), ("n_eligible", C.c_int32), ("n_planes", C.c_int32), ("n_assigned", C.c_int32),
                ("ground_index", C.c_int32), ("rounds", C.c_int32), ("stop_reason", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(EslDensePlaneParams) == 80 and C.sizeof(EslDensePlaneResult) == 32


def default_dense_plane_params(**kw):
    """esl_dense_plane_params_default (include/esl.h); up = a sequence of three numbers"""
    p = EslDensePlaneParams(dist_tol=0.02, up=(C.c_double * 3)(0.0, 0.0, 0.0), up_min_cos=0.7071067811865476, n_hypotheses=1024, max_planes=8,
                            min_inliers=1000, min_baseline=8, min_count=1, skip_labelled=0, refine=1, pad=0, seed=0)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, (C.c_double * 3)(*[float(x) for x in v]) if k == "up" else v)
    return p


class EslDenseRenderParams(C.Structure):
    """esl_dense_render_params: the depth gates, the footprint and the z-buffer's size of esl_dense_render."""
    _fields_ = [("depth_scale", C.c_double), ("depth_min", C.c_double), ("depth_max", C.c_double), ("depth_tol", C.c_double),
                ("footprint", C.c_double), ("max_radius", C.c_int32), ("min_count", C.c_int32), ("zbuf_bytes", C.c_int64)]


class EslDenseRenderResult(C.Structure):
    """esl_dense_render_result: status 3 / 4 = an invalid map (n_voxels = -1); n_small = voxels below min_count; n_chunks = chunks of frames."""
    _fields_ = [("status", C.c_int32), ("n_voxels", C.c_int32), ("n_small", C.c_int32), ("n_chunks", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(EslDenseRenderParams) == 56 and C.sizeof(EslDenseRenderResult) == 16


def default_dense_render_params(**kw):
    """esl_dense_render_params_default: design choices, not values tuned on real data (include/esl.h)"""
    p = EslDenseRenderParams(depth_scale=5000.0, depth_min=0.1, depth_max=6.0, depth_tol=0.05, footprint=1.0, max_radius=8, min_count=1,
                             zbuf_bytes=268435456)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class EslDenseNormalParams(C.Structure):
    """esl_dense_normal_params: the curvature gate, the neighbourhood and the counts of esl_dense_normals (steps N1 to N5)."""
    _fields_ = [("max_curvature", C.c_double), ("radius", C.c_int32), ("min_count", C.c_int32), ("min_neighbors", C.c_int32), ("pad", C.c_int32)]


class EslDenseNormalResult(C.Structure):
    """esl_dense_normal_result: status 3 / 4 = an invalid map (n_voxels = -1); the eligible voxels and those with a valid normal."""
    _fields_ = [("status", C.c_int32), ("n_voxels", C.c_int32), ("n_eligible", C.c_int32), ("n_valid", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class EslDenseAlignParams(C.Structure):
    """esl_dense_align_params: the match gate, the step's guards, the stopping rule, the sampling and the normals of esl_dense_align_frames."""
    _fields_ = [("max_dist", C.c_double), ("damping", C.c_double), ("min_pivot_ratio", C.c_double), ("tol_t", C.c_double), ("tol_r", C.c_double),
                ("iters", C.c_int32), ("stride", C.c_int32), ("reach", C.c_int32), ("min_inliers", C.c_int32), ("normals", EslDenseNormalParams)]


DENSE_ALIGN_COUNTS = ("n_sampled", "n_zero", "n_depth_out", "n_key_out", "n_used", "n_nomatch", "n_far", "n_inlier")
DENSE_ALIGN_STATUS = {0: "max_iters", 1: "converged", 2: "too_few", 3: "degenerate"}
DENSE_ALIGN_ROW = 37          # a frame's words per pass: 21 J J, 6 J e, e^2, the inlier count, the eight counts


class EslDenseAlignFrame(C.Structure):
    """esl_dense_align_frame: a frame's status, steps taken, the counts, sum e^2 and H of its last pass and the size of its last step."""
    _fields_ = [("status", C.c_int32), ("iters", C.c_int32)] + [(k, C.c_int64) for k in DENSE_ALIGN_COUNTS] + [
        ("sum_e2", C.c_double), ("H", C.c_double * 36), ("step_t", C.c_double), ("step_r", C.c_double)]


class EslDenseAlignResult(C.Structure):
    """esl_dense_align_result: status 3 / 4 = an invalid map (n_voxels = -1); the voxels with a valid normal; the passes run."""
    _fields_ = [("status", C.c_int32), ("n_voxels", C.c_int32), ("n_valid", C.c_int32), ("n_passes", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(EslDenseNormalParams) == 24 and C.sizeof(EslDenseNormalResult) == 16
assert C.sizeof(EslDenseAlignParams) == 80 and C.sizeof(EslDenseAlignFrame) == 384 and C.sizeof(EslDenseAlignResult) == 16

DENSE_NORMAL_DEFAULTS = dict(max_curvature=0.05, radius=1, min_count=1, min_neighbors=5)


def default_dense_normal_params(**kw):
    """esl_dense_normal_params_default: design choices, not values tuned on real data (include/esl.h)"""
    p = EslDenseNormalParams(pad=0, **DENSE_NORMAL_DEFAULTS)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_dense_align_params(**kw):
    """esl_dense_align_params_default (include/esl.h); a keyword that names a field of esl_dense_normal_params sets it in .normals"""
    p = EslDenseAlignParams(max_dist=0.0, damping=0.0, min_pivot_ratio=1e-6, tol_t=1e-5, tol_r=1e-5, iters=4, stride=2, reach=1, min_inliers=100,
                            normals=default_dense_normal_params())
    for k, v in kw.items():
        if k in DENSE_NORMAL_DEFAULTS:
            setattr(p.normals, k, v)
        elif k != "normals" and hasattr(p, k):
            setattr(p, k, v)
        else:
            raise AttributeError(k)
    return p


class EslDenseCarveParams(C.Structure):
    """esl_dense_carve_params: the depth gates, the window, the verdict's two thresholds and whether the carved samples are removed."""
    _fields_ = [("depth_scale", C.c_double), ("depth_min", C.c_double), ("depth_max", C.c_double), ("depth_tol", C.c_double),
                ("window", C.c_int32), ("min_through", C.c_int32), ("through_per_agree", C.c_int32), ("apply", C.c_int32)]


class EslDenseCarveResult(C.Structure):
    """esl_dense_carve_result: status 3 / 4 = an invalid map (n_voxels = -1); the voxels tested and carved, the owners' samples found and
    carved, and the removal's own result (zeros with apply = 0)."""
    _fields_ = [("status", C.c_int32), ("n_voxels", C.c_int32), ("n_tested", C.c_int32), ("n_carved", C.c_int32),
                ("samples_found", C.c_int64), ("samples_carved", C.c_int64), ("removed", EslDenseRemoveResult)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "removed"}
        d["removed"] = self.removed.as_dict()
        return d


assert C.sizeof(EslDenseCarveParams) == 48 and C.sizeof(EslDenseCarveResult) == 96

DENSE_CARVE_DEFAULTS = dict(depth_scale=5000.0, depth_min=0.1, depth_max=6.0, depth_tol=0.05, window=1, min_through=2, through_per_agree=1, apply=0)


def default_dense_carve_params(**kw):
    """esl_dense_carve_params_default: design choices, not values tuned on real data (include/esl.h)"""
    p = EslDenseCarveParams(**DENSE_CARVE_DEFAULTS)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class EslDenseCovisParams(C.Structure):
    """esl_dense_covis_params: the carving's depth gates and window, the redundancy rule (min_others, cover_num / cover_den) and the
    cull rounds at most."""
    _fields_ = [("depth_scale", C.c_double), ("depth_min", C.c_double), ("depth_max", C.c_double), ("depth_tol", C.c_double),
                ("window", C.c_int32), ("min_others", C.c_int32), ("cover_num", C.c_int32), ("cover_den", C.c_int32),
                ("max_cull", C.c_int32), ("reserved", C.c_int32)]


class EslDenseCovisResult(C.Structure):
    """esl_dense_covis_result: status 3 / 4 = an invalid map (n_voxels = -1); the voxels some frame sees, the frames culled, the sums of
    seen_f over the frames and of the pair counts over a < b."""
    _fields_ = [("status", C.c_int32), ("n_voxels", C.c_int32), ("n_seen", C.c_int32), ("n_culled", C.c_int32),
                ("sum_seen", C.c_int64), ("sum_pairs", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(EslDenseCovisParams) == 56 and C.sizeof(EslDenseCovisResult) == 32

DENSE_COVIS_DEFAULTS = dict(depth_scale=5000.0, depth_min=0.1, depth_max=6.0, depth_tol=0.05, window=1, min_others=3, cover_num=9, cover_den=10,
                            max_cull=0, reserved=0)


def default_dense_covis_params(**kw):
    """esl_dense_covis_params_default: design choices, not values tuned on real data (include/esl.h)"""
    p = EslDenseCovisParams(**DENSE_COVIS_DEFAULTS)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def dense_argtypes(L):
    """the esl_dense_* calls take nullable pointers: declared, so that None passes as NULL and a wrong type raises"""
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    up, bp = C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)
    L.esl_dense_covis_params_default.argtypes = [C.POINTER(EslDenseCovisParams)]
    L.esl_dense_covis_params_default.restype = None
    L.esl_dense_covis_frames.argtypes = [C.c_void_p, dp, C.c_int32, up, bp, dp, C.c_int32, C.c_int32, C.POINTER(EslDenseCovisParams), C.c_int64,
                                         ip, ip, ip, C.POINTER(EslDenseCovisResult)]
    L.esl_dense_covis_frames.restype = C.c_int
    L.esl_dense_carve_params_default.argtypes = [C.POINTER(EslDenseCarveParams)]
    L.esl_dense_carve_params_default.restype = None
    L.esl_dense_carve_frames.argtypes = [C.c_void_p, dp, C.c_int32, up, dp, C.c_int32, up, bp, ip, dp, C.c_int32, C.c_int32,
                                         C.POINTER(EslDenseCarveParams), C.c_int64, ip, bp, ip, up, bp, ip, C.POINTER(EslDenseCarveResult)]
    L.esl_dense_carve_frames.restype = C.c_int
    L.esl_dense_render_params_default.argtypes = [C.POINTER(EslDenseRenderParams)]
    L.esl_dense_render_params_default.restype = None
    L.esl_dense_render.argtypes = [C.c_void_p, dp, C.c_int32, dp, C.c_int32, C.c_int32, C.POINTER(C.c_uint16), C.POINTER(EslDenseRenderParams),
                                   dp, ip, C.POINTER(C.c_uint8), ip, ip, C.c_int64, ip, C.POINTER(EslDenseRenderResult)]
    L.esl_dense_render.restype = C.c_int
    L.esl_dense_normal_params_default.argtypes = [C.POINTER(EslDenseNormalParams)]
    L.esl_dense_normal_params_default.restype = None
    L.esl_dense_normals.argtypes = [C.c_void_p, C.POINTER(EslDenseNormalParams), C.c_int64, dp, dp, ip, C.POINTER(C.c_uint8),
                                    C.POINTER(EslDenseNormalResult)]
    L.esl_dense_normals.restype = C.c_int
    L.esl_dense_align_params_default.argtypes = [C.POINTER(EslDenseAlignParams)]
    L.esl_dense_align_params_default.restype = None
    L.esl_dense_align_frames.argtypes = [C.c_void_p, dp, C.c_int32, dp, C.c_int32, C.c_int32, C.POINTER(C.c_uint16), C.POINTER(EslDenseAlignParams),
                                         dp, C.POINTER(EslDenseAlignFrame), lp, C.POINTER(EslDenseAlignResult)]
    L.esl_dense_align_frames.restype = C.c_int
    L.esl_dense_params_default.argtypes = [C.POINTER(EslDenseParams)]
    L.esl_dense_params_default.restype = None
    L.esl_dense_begin.argtypes = [C.c_void_p, C.POINTER(EslDenseParams), C.c_int32, C.c_int32]
    L.esl_dense_add_frames.argtypes = [C.c_void_p, dp, C.c_int32, dp, C.c_int32, C.c_int32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8),
                                       ip, C.POINTER(EslDenseAddResult)]
    L.esl_dense_info_get.argtypes = [C.c_void_p, C.POINTER(EslDenseInfo)]
    L.esl_dense_extract.argtypes = [C.c_void_p, C.c_int64, ip, dp, ip, C.POINTER(C.c_uint8), ip, ip, lp]
    L.esl_dense_end.argtypes = [C.c_void_p]
    L.esl_debug_dense_allocs.argtypes = [C.c_void_p, lp, lp]
    L.esl_dense_obj_params_default.argtypes = [C.POINTER(EslDenseObjParams)]
    L.esl_dense_obj_params_default.restype = None
    L.esl_dense_objects.argtypes = [C.c_void_p, C.c_int32, dp, C.POINTER(EslDenseObjParams), dp, ip, C.c_int64, ip, C.c_int64, ip,
                                    C.POINTER(EslDenseObjResult)]
    L.esl_dense_plane_params_default.argtypes = [C.POINTER(EslDensePlaneParams)]
    L.esl_dense_plane_params_default.restype = None
    L.esl_dense_planes.argtypes = [C.c_void_p, C.POINTER(EslDensePlaneParams), dp, dp, ip, lp, dp, C.c_int64, ip, lp,
                                   C.POINTER(EslDensePlaneResult)]
    L.esl_debug_dense_planes_layout.argtypes = [ip, ip]
    img = [C.c_int32, dp, C.c_int32, C.c_int32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), ip]
    L.esl_dense_remove_frames.argtypes = [C.c_void_p, dp] + img + [C.POINTER(EslDenseRemoveResult)]
    L.esl_dense_move_frames.argtypes = [C.c_void_p, dp, dp] + img + [C.POINTER(EslDenseMoveResult)]
    L.esl_dense_slots_get.argtypes = [C.c_void_p, C.POINTER(EslDenseSlots)]
    L.esl_dense_purge.argtypes = [C.c_void_p, C.POINTER(EslDenseSlots), C.POINTER(EslDenseSlots)]
    for f in (L.esl_dense_begin, L.esl_dense_add_frames, L.esl_dense_info_get, L.esl_dense_extract, L.esl_dense_end,
              L.esl_debug_dense_allocs, L.esl_dense_objects, L.esl_dense_planes, L.esl_debug_dense_planes_layout,
              L.esl_dense_remove_frames, L.esl_dense_move_frames, L.esl_dense_slots_get, L.esl_dense_purge):
        f.restype = C.c_int


ROBUST_KINDS = {"none": 0, "huber": 1, "pseudo_huber": 2, "cauchy": 3, "tukey": 4}   # esl_robust_kind (include/esl.h)
EDGE_CLASSES = {"bbox": 0, "e3d": 1, "grav": 2, "odom": 3}                         # esl_edge_class


class EslRobustParams(C.Structure):
    """esl_robust_params: g2o robust kernel (kind, delta) per edge class (esl_lm_set_robust)."""
    _fields_ = [("kind", C.c_int32 * 4), ("delta", C.c_double * 4)]


def default_robust_params(**kw):
    """Every class without a kernel (the default).  Keywords bbox / e3d / grav / odom = (kind name, delta), e.g. ("huber", 1.0)."""
    p = EslRobustParams()
    for k in range(4):
        p.kind[k], p.delta[k] = 0, 1.0
    for cls, v in kw.items():
        if cls not in EDGE_CLASSES:
            raise ValueError(f"unknown edge class {cls!r}: one of {sorted(EDGE_CLASSES)}")
        if v is None:
            continue
        kind, delta = v
        if kind not in ROBUST_KINDS:
            raise ValueError(f"unknown robust kernel {kind!r}: one of {sorted(ROBUST_KINDS)}")
        p.kind[EDGE_CLASSES[cls]], p.delta[EDGE_CLASSES[cls]] = ROBUST_KINDS[kind], float(delta)
    return p


def default_lm_params(**kw):
    """Reference settings: optimize(10) (Optimizer.cpp:291), tau 1e-5, 10 trials
    (optimization_algorithm_levenberg.cpp:45-49), delta 1e-9 (base_binary_edge.hpp:147)."""
    p = EslLmParams(max_iters=10, max_trials=10, tau=1e-5, jacobian_mode=0, numeric_delta=1e-9,
                    linear_solver=0, drop_nan_bbox=1, bbox_residual=0, e3d_half_turn=0)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _arr(a, dtype, shape_tail=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape_tail is not None and a.size:
        a = a.reshape((-1,) + tuple(shape_tail))
    return a


class Graph:
    """Host-side SoA graph.  Keeps the numpy arrays alive and exposes an EslGraph view."""

    def __init__(self, K, n_cams, n_objs, cam_fixed=None,
                 bbox_cam=(), bbox_obj=(), bbox_meas=(), bbox_weight=(),
                 e3d_cam=(), e3d_obj=(), e3d_meas=(), e3d_weight=(),
                 grav_obj=(), grav_normal=(0, 0, 1, 0), grav_weight=0.0,
                 odom_i=(), odom_j=(), odom_meas=(), odom_info=None, check_visibility=0, image_rows=480, image_cols=640):
        self.K = tuple(float(k) for k in K)
        self.n_cams, self.n_objs = int(n_cams), int(n_objs)
        self.cam_fixed = None if cam_fixed is None else _arr(cam_fixed, np.uint8)
        self.bbox_cam = _arr(bbox_cam, np.int32); self.bbox_obj = _arr(bbox_obj, np.int32)
        self.bbox_meas = _arr(bbox_meas, np.float64, (4,)); self.bbox_weight = _arr(bbox_weight, np.float64)
        self.e3d_cam = _arr(e3d_cam, np.int32); self.e3d_obj = _arr(e3d_obj, np.int32)
        self.e3d_meas = _arr(e3d_meas, np.float64, (10,)); self.e3d_weight = _arr(e3d_weight, np.float64)
        self.grav_obj = _arr(grav_obj, np.int32)
        self.grav_normal = tuple(float(v) for v in grav_normal); self.grav_weight = float(grav_weight)
        self.odom_i = _arr(odom_i, np.int32); self.odom_j = _arr(odom_j, np.int32)
        self.odom_meas = _arr(odom_meas, np.float64, (7,))
        self.odom_info = None if odom_info is None else _arr(odom_info, np.float64, (6,))
        self.check_visibility, self.image_rows, self.image_cols = int(check_visibility), int(image_rows), int(image_cols)
        assert len(self.bbox_cam) == len(self.bbox_obj) == len(self.bbox_weight) == len(self.bbox_meas.reshape(-1, 4))
        assert len(self.e3d_cam) == len(self.e3d_obj) == len(self.e3d_weight) == len(self.e3d_meas.reshape(-1, 10))
        assert len(self.odom_i) == len(self.odom_j) == len(self.odom_meas.reshape(-1, 7))

    @staticmethod
    def _p(a, ptype):
        return a.ctypes.data_as(ptype) if a is not None and a.size else ptype()

    def c_struct(self):
        g = EslGraph()
        g.fx, g.fy, g.cx, g.cy = self.K
        g.n_cams, g.n_objs = self.n_cams, self.n_objs
        g.cam_fixed = self._p(self.cam_fixed, c_uint8_p)
        g.n_bbox = len(self.bbox_cam)
        g.bbox_cam = self._p(self.bbox_cam, c_int32_p); g.bbox_obj = self._p(self.bbox_obj, c_int32_p)
        g.bbox_meas = self._p(self.bbox_meas, c_double_p); g.bbox_weight = self._p(self.bbox_weight, c_double_p)
        g.n_e3d = len(self.e3d_cam)
        g.e3d_cam = self._p(self.e3d_cam, c_int32_p); g.e3d_obj = self._p(self.e3d_obj, c_int32_p)
        g.e3d_meas = self._p(self.e3d_meas, c_double_p); g.e3d_weight = self._p(self.e3d_weight, c_double_p)
        g.n_grav = len(self.grav_obj)
        g.grav_obj = self._p(self.grav_obj, c_int32_p)
        g.grav_normal = (C.c_double * 4)(*self.grav_normal); g.grav_weight = self.grav_weight
        g.n_odom = len(self.odom_i)
        g.odom_i = self._p(self.odom_i, c_int32_p); g.odom_j = self._p(self.odom_j, c_int32_p)
        g.odom_meas = self._p(self.odom_meas, c_double_p); g.odom_info = self._p(self.odom_info, c_double_p)
        g.check_visibility, g.image_rows, g.image_cols = self.check_visibility, self.image_rows, self.image_cols
        return g

    def subset_objects(self, keep):
        """Sub-graph holding only the ellipsoids in `keep` (ascending), re-indexed; cameras are kept.
        Used by the sharded driver (SURVEY.md §8 e) and by bench.py's bounded CPU sample."""
        keep = np.asarray(keep, dtype=np.int64)
        remap = -np.ones(self.n_objs, dtype=np.int64)
        remap[keep] = np.arange(len(keep))
        mb = remap[self.bbox_obj] >= 0 if len(self.bbox_obj) else np.zeros(0, bool)
        me = remap[self.e3d_obj] >= 0 if len(self.e3d_obj) else np.zeros(0, bool)
        mg = remap[self.grav_obj] >= 0 if len(self.grav_obj) else np.zeros(0, bool)
        return Graph(self.K, self.n_cams, len(keep), self.cam_fixed,
                     self.bbox_cam[mb], remap[self.bbox_obj[mb]] if mb.any() else (),
                     self.bbox_meas.reshape(-1, 4)[mb], self.bbox_weight[mb],
                     self.e3d_cam[me], remap[self.e3d_obj[me]] if me.any() else (),
                     self.e3d_meas.reshape(-1, 10)[me], self.e3d_weight[me],
                     remap[self.grav_obj[mg]] if mg.any() else (), self.grav_normal, self.grav_weight,
                     self.odom_i, self.odom_j, self.odom_meas, self.odom_info, self.check_visibility, self.image_rows, self.image_cols)

    def subset(self, cams, objs):
        """Sub-graph on the cameras `cams` and the ellipsoids `objs` (both ascending, re-indexed in that order): the edges whose
        two ends are both kept.  Used by the full-size parity tests (a sample of BASELINE configs[3] the CPU checker can hold)."""
        cams = np.asarray(cams, dtype=np.int64); objs = np.asarray(objs, dtype=np.int64)
        rc = -np.ones(self.n_cams, dtype=np.int64); rc[cams] = np.arange(len(cams))
        ro = -np.ones(self.n_objs, dtype=np.int64); ro[objs] = np.arange(len(objs))
        mb = (rc[self.bbox_cam] >= 0) & (ro[self.bbox_obj] >= 0) if len(self.bbox_cam) else np.zeros(0, bool)
        me = (rc[self.e3d_cam] >= 0) & (ro[self.e3d_obj] >= 0) if len(self.e3d_cam) else np.zeros(0, bool)
        mg = ro[self.grav_obj] >= 0 if len(self.grav_obj) else np.zeros(0, bool)
        mo = (rc[self.odom_i] >= 0) & (rc[self.odom_j] >= 0) if len(self.odom_i) else np.zeros(0, bool)
        fixed = None if self.cam_fixed is None else self.cam_fixed[cams]
        return Graph(self.K, len(cams), len(objs), fixed,
                     rc[self.bbox_cam[mb]], ro[self.bbox_obj[mb]], self.bbox_meas.reshape(-1, 4)[mb], self.bbox_weight[mb],
                     rc[self.e3d_cam[me]], ro[self.e3d_obj[me]], self.e3d_meas.reshape(-1, 10)[me], self.e3d_weight[me],
                     ro[self.grav_obj[mg]], self.grav_normal, self.grav_weight,
                     rc[self.odom_i[mo]], rc[self.odom_j[mo]], self.odom_meas.reshape(-1, 7)[mo],
                     None if self.odom_info is None else self.odom_info.reshape(-1, 6)[mo],
                     self.check_visibility, self.image_rows, self.image_cols)
