"""Scenes for the 2-D association tests (tests/test_assoc2d_ref.py on the CPU, tests/test_gpu_assoc2d.py on the device).  Pure numpy;
imports nothing of the product.  Every scene is a dict(cams (F, 7) Tcw, objs (M, 10), obj_labels, K, rows, cols, det_offsets,
det_boxes, det_labels, true_obj)."""
import numpy as np

import assoc2d_ref as ar

# The statement's unclipped boxes against oracle.pyoracle.project_bbox (the reference's route: inverse conic, ellipse parameters) over
# every eligible prediction of room_scene(0 .. 5): at most 1.02e-9 px (tests/test_assoc2d_ref.py measures it again and asserts it is
# below TOL).  The device agrees with the statement within ten times that, and not below 1e-9.
ORACLE_DISAGREEMENT_PX = 1.02e-9
TOL = max(10 * ORACLE_DISAGREEMENT_PX, 1e-9)
# No decision quantity closer than this to its threshold (check_conditions).  The rule asks for 1e-6 and for 100 times TOL; 100 TOL is
# 1.02e-6, so the checker demands 2e-6: the stricter of the two, rounded up.
CONDITION = 2e-6
assert CONDITION >= 1e-6 and CONDITION >= 100 * TOL
ROWS, COLS = 480, 640
K = (525.0, 525.0, 319.5, 239.5)
SEEDS = (0, 1, 2, 3, 4, 5)


def rot_to_quat(R):
    """rotation matrix -> x y z w, w >= 0"""
    v = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(v)); s = 2 * np.sqrt(v[k])
    if k == 0:
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, s / 4]
    elif k == 1:
        q = [s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif k == 2:
        q = [(R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4, (R[1, 0] - R[0, 1]) / s]
    q = np.array(q); q /= np.linalg.norm(q)
    return q if q[3] >= 0 else -q


def look_at(pos, target, up=(0.0, 0.0, 1.0)):
    """Tcw (7,) of a camera at pos looking at target: x right, y down, z forward"""
    pos = np.asarray(pos, dtype=np.float64)
    fwd = np.asarray(target, dtype=np.float64) - pos; fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    Rcw = np.stack([right, down, fwd], axis=0)
    return np.concatenate([-Rcw @ pos, rot_to_quat(Rcw)])


def sphere(center, r):
    return np.array([center[0], center[1], center[2], 0, 0, 0, 1.0, r, r, r])


IDENTITY_CAM = np.array([0, 0, 0, 0, 0, 0, 1.0])   # camera at the origin looking along +z


def detections_of(cams, objs, labels, rng, p=None, jitter=4.0):
    """a frame's detections: its non-occluded predictions in shuffled order, every coordinate moved by up to +-jitter px, each with the
    label of the map object it was generated from"""
    off, boxes, labs, true = [0], [], [], []
    for Tcw in cams:
        pr = ar.predict(Tcw, objs, K, ROWS, COLS, p)
        vis = np.nonzero(pr["flags"] == 1)[0]
        vis = vis[rng.permutation(len(vis))]
        boxes.append(pr["boxes"][vis] + rng.uniform(-jitter, jitter, size=(len(vis), 4)))
        labs.append(labels[vis]); true.append(vis)
        off.append(off[-1] + len(vis))
    return (np.array(off, np.int32), np.concatenate(boxes).reshape(-1, 4), np.concatenate(labs).astype(np.int32),
            np.concatenate(true).astype(np.int32))


def room_scene(seed, M=40, F=6, n_labels=5):
    """M ellipsoids standing on z = 0 in a 10 m room, F cameras on a circle of radius 4 m at height 1.2 m looking at (0, 0, 0.4)"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.15, 0.6, size=(M, 3))
    xy = rng.uniform(-5, 5, size=(M, 2))
    yaw = rng.uniform(-np.pi, np.pi, size=M)
    objs = np.zeros((M, 10))
    objs[:, :2] = xy; objs[:, 2] = s[:, 2]
    objs[:, 5] = np.sin(yaw / 2); objs[:, 6] = np.cos(yaw / 2)
    objs[:, 7:10] = s
    labels = rng.integers(0, n_labels, M).astype(np.int32)
    ang = 2 * np.pi * (np.arange(F) + rng.uniform(0, 1)) / F
    cams = np.stack([look_at([4 * np.cos(a), 4 * np.sin(a), 1.2], [0, 0, 0.4]) for a in ang])
    off, boxes, labs, true = detections_of(cams, objs, labels, rng)
    return dict(cams=cams, objs=objs, obj_labels=labels, K=K, rows=ROWS, cols=COLS, det_offsets=off, det_boxes=boxes, det_labels=labs,
                true_obj=true)


def grid_scene(n, n_det=30, seed=7):
    """one frame looking at the first n spheres of a 41 x 25 grid: 15 px apart, 10.6 to 11.8 px wide, every depth its own -- n eligible
    predictions, none occluded; n_det of them detected"""
    assert n <= 41 * 25
    rng = np.random.default_rng(seed)
    idx = np.arange(41 * 25)
    gx, gy = idx % 41, idx // 41
    z = 20.0 + 0.002 * rng.permutation(len(idx))
    u, v = 15.0 * gx + 19.75, 18.0 * gy + 23.5
    r = z * rng.uniform(0.0101, 0.0112, size=len(idx))               # 2 fx r / z = 10.6 to 11.8 px
    ctr = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    objs = np.stack([sphere(c, rr) for c, rr in zip(ctr, r)])[:n]
    labels = (idx % 3).astype(np.int32)[:n]
    cams = IDENTITY_CAM[None].copy()
    pr = ar.predict(cams[0], objs, K, ROWS, COLS)
    assert int((pr["flags"] == 1).sum()) == n
    pick = np.sort(rng.choice(min(n - 1, 1000), size=n_det, replace=False))   # of the first 1,000: a scene with fewer spheres keeps them
    rng2 = np.random.default_rng(seed + 1)
    boxes = pr["boxes"][pick] + rng2.uniform(-1.0, 1.0, size=(n_det, 4))
    return dict(cams=cams, objs=objs, obj_labels=labels, K=K, rows=ROWS, cols=COLS, det_offsets=np.array([0, n_det], np.int32),
                det_boxes=boxes, det_labels=labels[pick], true_obj=pick.astype(np.int32))


def reference(sc, **over):
    return ar.associate(sc["cams"], sc["objs"], sc["obj_labels"], sc["K"], sc["rows"], sc["cols"], sc["det_offsets"], sc["det_boxes"],
                        sc["det_labels"], over)


def check_conditions(ref):
    """what makes a comparison of integers between two arithmetics meaningful: the predicate's comparisons, C22 / du / dv against 0, the
    clipped sizes against min_box_px, every coverage ratio against occl_ratio, every depth pair, the best IoU against min_iou and the
    runner-up -- all at least CONDITION from their thresholds"""
    assert ref["margin"] > CONDITION, ref["margin"]
