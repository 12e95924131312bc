"""Scenes for the relocalisation tests (tests/test_reloc_ref.py on the CPU, tests/test_gpu_reloc.py on the device): the synthetic
graphs' frames the issue names, and small hand-made rooms in which the candidate count, the decoys and the ground plane are
under control.  Every scene is a dict(map, map_labels, ground_world, det, det_labels, ground_cam, Twc, true_obj, params)."""
import numpy as np

CONDITION = 1e-9   # no compared quantity closer than this (relative) to its threshold, winner ahead of the runner-up by more


def _quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def plane_to_camera(plane_w, Rwc, twc):
    """pi_c = Twc^T pi_w: the world plane as the camera sees it"""
    n = np.asarray(plane_w[:3], dtype=np.float64)
    return np.concatenate([Rwc.T @ n, [n @ twc + plane_w[3]]])


def synth_scene(pkg, seed):
    """The frame with the most 3-D edges of synth.make_graph(40, 30, 600, seed, frac_3d=1.0): its e3d_meas as detections, the true
    ellipsoids as the map."""
    g, _, _, truth = pkg.synth.make_graph(40, 30, 600, seed=seed, frac_3d=1.0)
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 4, g.n_objs).astype(np.int32)
    frame = int(np.argmax(np.bincount(g.e3d_cam, minlength=g.n_cams)))
    sel = np.nonzero(g.e3d_cam == frame)[0]
    Tcw = truth["cams"][frame]
    Rcw = _quat_to_R(Tcw[3:7])
    Rwc, twc = Rcw.T, -Rcw.T @ Tcw[:3]
    gw = np.array([0.0, 0.0, 1.0, 0.0])
    return dict(map=truth["objs"].copy(), map_labels=labels, ground_world=gw, det=g.e3d_meas.reshape(-1, 10)[sel].copy(),
                det_labels=labels[g.e3d_obj[sel]], ground_cam=plane_to_camera(gw, Rwc, twc), Rwc=Rwc, twc=twc,
                true_obj=g.e3d_obj[sel].astype(np.int32), params={}, frame=frame, edges=sel, graph=g, truth=truth)


def _basis_with_third(n):
    n = np.asarray(n, dtype=np.float64); n = n / np.linalg.norm(n)
    a = np.cross(n, [1.0, 0, 0] if abs(n[0]) < 0.9 else [0, 1.0, 0]); a /= np.linalg.norm(a)
    return np.stack([a, np.cross(n, a), n], axis=1)   # columns: a rotation that carries z onto n


def room_scene(seed, counts, det_of, normal=(0, 0, 1), offset=0.0, noise=0.01, params=None, label_of=None, extra=None):
    """A 10 m room on the plane `normal` . x + offset = 0.  counts[l] map objects carry label l; detection k sees map object
    det_of[k] (index into the map, label block by label block) with `noise` m on its centre and permuted half-axes.
    extra(map, rng): last-minute edits of the map (decoys)."""
    rng = np.random.default_rng(seed)
    M = int(np.sum(counts))
    lab = np.concatenate([np.full(c, l, dtype=np.int32) for l, c in enumerate(counts)]) if label_of is None else np.asarray(label_of, np.int32)
    s = rng.uniform(0.15, 0.6, size=(M, 3))
    ctr = np.concatenate([rng.uniform(-5, 5, size=(M, 2)), s[:, 2:3]], axis=1)   # standing on z = 0 of the room's own frame
    if extra is not None:
        extra(ctr, s, rng)
    W = _basis_with_third(normal)
    n = W[:, 2]
    shift = -offset * n                       # n . (W x + shift) + offset = z
    mp = np.zeros((M, 10)); mp[:, :3] = ctr @ W.T + shift; mp[:, 6] = 1.0; mp[:, 7:10] = s
    gw = np.concatenate([n, [offset]])
    # camera: 1.2 m up, looking around with some pitch and roll (room frame), then into the world
    yaw, pitch, roll = rng.uniform(-np.pi, np.pi), rng.uniform(-0.4, 0.4), rng.uniform(-0.2, 0.2)
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]); Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Rwc = W @ Rz @ Ry @ Rx
    twc = W @ np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), 1.2]) + shift
    det_of = np.asarray(det_of, dtype=np.int32)
    D = len(det_of)
    det = np.zeros((D, 10)); det[:, 6] = 1.0
    if D:
        det[:, :3] = (mp[det_of, :3] - twc) @ Rwc + noise * rng.standard_normal((D, 3))
        for k in range(D):
            det[k, 7:10] = (mp[det_of[k], 7:10] * (1 + 0.02 * rng.standard_normal(3)))[rng.permutation(3)]
    return dict(map=mp, map_labels=lab, ground_world=gw, det=det, det_labels=lab[det_of] if D else np.zeros(0, np.int32),
                ground_cam=plane_to_camera(gw, Rwc, twc), Rwc=Rwc, twc=twc, true_obj=det_of, params=dict(params or {}))


def p_scene(P):
    """exactly P candidates: 5 detections with labels 0..4, counts[l] same-label map objects each, height and size gates open"""
    base, rest = divmod(P, 5)
    counts = [base + (1 if l < rest else 0) for l in range(5)]
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return room_scene(100 + P, counts, first, params=dict(height_tol=10.0, size_ratio=0.0))


def decoy_scene():
    """D = 3, M = 5: a decoy with detection 0's label sits at |q1 - q0| from object 1 -- a consistent 2-inlier hypothesis -- the
    3-inlier pose must win"""
    def extra(ctr, s, rng):
        dist = np.linalg.norm(ctr[1, :2] - ctr[0, :2])
        ang = rng.uniform(0, 2 * np.pi)
        ctr[3, :2] = ctr[1, :2] + dist * np.array([np.cos(ang), np.sin(ang)])
        s[3] = s[0]; ctr[3, 2] = s[3, 2]
    return room_scene(7, [1, 1, 1, 1, 1], [0, 1, 2], label_of=[0, 1, 2, 0, 3], extra=extra)


def repeated_scene():
    """two detections of the same map object: both are inliers of the winner, the association gives the object to the first"""
    return room_scene(11, [2, 2, 2], [0, 0, 2, 4], noise=0.02)


def open_gates_scene():
    """labels ignored, no size gate: every pair within the height gate is a candidate"""
    return room_scene(13, [3, 3, 2], [0, 3, 6, 7, 1], params=dict(match_labels=0, size_ratio=1.0))


TILTS = {"z": (0.10, 0.30, 0.90), "y": (0.30, 0.90, 0.10), "x": (0.90, 0.10, 0.30)}   # the normal is closest to this axis


def tilted_scene(axis):
    return room_scene(17, [2, 2, 2, 1], [0, 2, 4, 6, 1], normal=TILTS[axis], offset=0.7)


def check_conditions(r):
    """what makes a comparison of integers between two arithmetics meaningful"""
    assert r["margin"] > CONDITION, r["margin"]
    assert r["runner_gap"] > CONDITION, r["runner_gap"]
    assert r["refine_gap"] > CONDITION, r["refine_gap"]
