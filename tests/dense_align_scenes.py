"""Scenes of the esl_dense_normals / esl_dense_align_frames tests: a 4 x 3 x 2.5 m box room seen from inside (its map from six frames, a
held-out frame looking into a corner, a frame that sees one wall only, an empty frame), maps whose samples are placed exactly at dyadic
points (1 x 1 frames), and the calls (CASES) the CPU test asserts its premises on and the GPU test runs.  Everything is generated from
fixed numbers; nothing here is imported by the package."""
import functools

import numpy as np

import dense_align_ref as dar
import dense_ref as dr
import dense_update_ref as dur

LEAF = 0.05
MAXV = 1 << 16
ROWS, COLS = 120, 160
K = (80.0, 80.0, 79.5, 59.5)
DEPTH_SCALE = 5000.0
# the room: walls in the middle of voxels, not on their boundaries
LO = np.array([0.023, 0.017, 0.031])
HI = LO + np.array([4.0, 3.0, 2.5])
MAP_PARAMS = dict(leaf=LEAF, max_voxels=MAXV, stride=1)
PLEAF = 1.0 / 64


def quat_of(R):
    """the quaternion (x, y, z, w), w >= 0, of a rotation matrix"""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-3:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:          # a half turn: the largest diagonal entry
        i = int(np.argmax(np.diag(R))); j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(max(0.0, 1.0 + R[i, i] - R[j, j] - R[k, k])) * 2
        q = np.zeros(4)
        q[i] = s / 4; q[j] = (R[j, i] + R[i, j]) / s; q[k] = (R[k, i] + R[i, k]) / s; q[3] = (R[k, j] - R[j, k]) / s
    return q / np.linalg.norm(q)


def look_at(o, target, up=(0.0, 0.0, 1.0)):
    """Tcw = (t, q) of a camera at o looking at target: z_c forward, x_c right, y_c down"""
    o, target = np.asarray(o, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (target - o) / np.linalg.norm(target - o)
    x = np.cross(z, -np.asarray(up)); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])          # rows: the camera's axes in the world = R_cw
    return np.concatenate([-R @ o, quat_of(R)])


def box_depth(cam, Kx, rows, cols, lo=LO, hi=HI):
    """the depth image of the room's inside from the pose cam: per pixel the nearest wall along its ray, in raw units"""
    R, t = dr.pose(cam)
    o = -R.T @ t
    fx, fy, cx, cy = Kx
    rr_, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    d_c = np.stack([(cc - cx) / fx, (rr_ - cy) / fy, np.ones_like(cc, dtype=np.float64)], axis=-1)
    d_w = d_c @ R          # R^T d_c per pixel
    z = np.full((rows, cols), np.inf)
    with np.errstate(all="ignore"):
        for a in range(3):
            for wall in (lo[a], hi[a]):
                s = (wall - o[a]) / d_w[..., a]
                z = np.where((s > 0) & (s < z), s, z)
    return np.clip(np.rint(z * DEPTH_SCALE), 1, 65535).astype(np.uint16)


CENTRE = LO + np.array([2.2, 1.6, 1.3])
CORNER = LO + np.array([0.0, 0.0, 0.0])
MAP_VIEWS = [((2.2, 1.6, 1.3), (0.3, 0.3, 0.2)), ((2.5, 1.3, 1.1), (0.2, 0.8, 0.5)), ((1.9, 1.9, 1.5), (0.9, 0.2, 0.4)),
             ((2.4, 1.8, 1.0), (0.1, 0.1, 1.0)), ((2.0, 1.4, 1.6), (0.6, 0.6, 0.0)), ((2.6, 1.7, 1.4), (0.0, 1.2, 0.9))]
HELD_OUT = ((2.3, 1.5, 1.2), (0.35, 0.4, 0.3))          # into the corner: two walls and the floor
ONE_WALL = ((1.0, 1.2, 1.1), (0.0, 1.2, 1.1))           # 1 m in front of the wall x = lo, straight at it: +-1 m x +-0.75 m of that wall
START_DELTA = [0.02, -0.02, 0.01, 0.006, -0.005, 0.00624]          # |v| = 30 mm, |omega| = 10.0 mrad


def moved(cam, delta):
    """the pose after the increment delta = (v, omega) of the statement's step d"""
    return np.array(dar.update(cam, list(delta)))


@functools.lru_cache(maxsize=None)
def views(rows=ROWS, cols=COLS):
    """the held-out frame, the one-wall frame and the empty frame at an image size (K scaled with it) -> dict(K, true (3, 7), depth)"""
    s = cols / COLS
    Kx = (K[0] * s, K[1] * s, (cols - 1) / 2, (rows - 1) / 2)
    cams = np.stack([look_at(LO + np.array(HELD_OUT[0]), LO + np.array(HELD_OUT[1])), look_at(LO + np.array(ONE_WALL[0]), LO + np.array(ONE_WALL[1])),
                     look_at(CENTRE, CORNER)])
    depth = np.stack([box_depth(cams[0], Kx, rows, cols), box_depth(cams[1], Kx, rows, cols), np.zeros((rows, cols), np.uint16)])
    depth[0, rows // 10:rows // 5, cols // 8:cols // 4] -= 4000          # a box 0.8 m in front of the walls that the map never saw: no match
    start = np.stack([moved(cams[0], START_DELTA), moved(cams[1], START_DELTA), moved(cams[2], START_DELTA)])
    return dict(K=Kx, rows=rows, cols=cols, true=cams, start=start, depth=depth)


def point_frames(points):
    """one 1 x 1 frame per sample (dense_objects_ref.voxel_frames' construction): K = (1, 1, 0, 0), raw depth 5000, identity rotation,
    t = (-X, -Y, 1 - Z) puts the sample at (X, Y, Z) exactly when the numbers are dyadic"""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cams = np.zeros((len(P), 7)); cams[:, 0] = -P[:, 0]; cams[:, 1] = -P[:, 1]; cams[:, 2] = 1.0 - P[:, 2]; cams[:, 6] = 1.0
    return dict(cams=cams, K=(1.0, 1.0, 0.0, 0.0), rows=1, cols=1, depth=np.full((len(P), 1, 1), 5000, np.uint16), bgr=None, inst=None)


def lattice_points(kind):
    """dyadic sample points, leaf 2^-6: `plane` a 9 x 9 patch of voxel centres at kz = 3; `tilted` z = x / 2 over 9 x 9 columns (two
    samples per column, inside one voxel); `edge` two voxels; `corner` three 5 x 5 faces meeting at a corner"""
    c = lambda k: (k + 0.5) / 64          # noqa: E731
    if kind == "plane":
        return [(c(i), c(j), c(3)) for i in range(9) for j in range(9)]
    if kind == "tilted":          # x = (i + 1/2) / 64, z = x / 2: voxel kz = floor(i / 2 + 1 / 4) -- a staircase whose centroids lie on the plane
        return [(c(i), c(j), c(i) / 2) for i in range(9) for j in range(9)]
    if kind == "edge":
        return [(c(0), c(0), c(0)), (c(1), c(0), c(0))]
    if kind == "corner":
        return ([(c(i), c(j), c(0)) for i in range(5) for j in range(5)] + [(c(i), c(0), c(k)) for i in range(5) for k in range(1, 5)]
                + [(c(0), c(j), c(k)) for j in range(1, 5) for k in range(1, 5)])
    raise KeyError(kind)


def build(frames, params, remove=None):
    m = dur.DenseUpdateMap(False, False, **params)
    if frames is not None:
        m.add_frames(frames["cams"], frames["K"], frames["rows"], frames["cols"], frames["depth"])
        for f in remove or []:
            m.remove_frames(frames["cams"][f:f + 1], frames["K"], frames["rows"], frames["cols"], frames["depth"][f:f + 1])
    return m


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict(frames (dense_add_frames' arguments), params (esl_dense_begin's), map (the statement's map), remove (frames then removed))"""
    if name in ("plane", "tilted", "edge", "corner"):
        fr = point_frames(lattice_points(name))
        params = dict(leaf=PLEAF, max_voxels=1 << 12)
        return dict(frames=fr, params=params, map=build(fr, params), remove=None)
    if name == "full":          # more voxels than the map may hold: status 3
        fr = point_frames(lattice_points("plane"))
        params = dict(leaf=PLEAF, max_voxels=8)
        return dict(frames=fr, params=params, map=build(fr, params), remove=None)
    if name in ("room", "removed", "without"):
        cams = np.stack([look_at(LO + np.array(o), LO + np.array(t)) for o, t in MAP_VIEWS])
        fr = dict(cams=cams, K=K, rows=ROWS, cols=COLS, depth=np.stack([box_depth(c, K, ROWS, COLS) for c in cams]), bgr=None, inst=None)
        if name == "without":          # the map of "removed", built from scratch
            keep = [0, 1, 2, 4, 5]
            fr = dict(fr, cams=cams[keep], depth=fr["depth"][keep])
        remove = [3] if name == "removed" else None
        return dict(frames=fr, params=dict(MAP_PARAMS), map=build(fr, MAP_PARAMS, remove), remove=remove)
    raise KeyError(name)


def extract(name):
    m = scene(name)["map"]
    e = m.extract()
    if e["n_voxels"] < 0:
        e["status"] = m.status
    return e


def case(name):
    """-> dict(map, cams (the start poses), true, K, rows, cols, depth, params): one esl_dense_align_frames call"""
    v = views()
    c = dict(map="room", frames=[0], view=v, params={})
    if name == "corner":
        pass
    elif name == "corner_s1":
        c.update(params=dict(stride=1))
    elif name in ("small", "small_odd"):          # 47 x 63 at stride 2: 24 x 32 samples; 45 x 61: 23 x 31 = 713, a multiple of neither 64 nor 256
        c.update(view=views(47, 63) if name == "small" else views(45, 61), params=dict(min_inliers=50))
    elif name in ("reach0", "reach2"):
        c.update(params=dict(reach=int(name[5:])))
    elif name == "radius2":
        c.update(params=dict(radius=2, min_neighbors=12))
    elif name == "far":          # a gate of 2 cm at a start error of 3 cm: many matches are too far
        c.update(params=dict(max_dist=0.02))
    elif name == "mixed":          # the good frame, the one-wall frame and the empty frame in one call
        c.update(frames=[0, 1, 2])
    elif name == "one_wall":
        c.update(frames=[1])
    elif name == "empty":
        c.update(frames=[2])
    elif name in ("removed", "without"):
        c.update(map=name)
    else:
        raise KeyError(name)
    v = c.pop("view"); f = c.pop("frames")
    c.update(cams=v["start"][f], true=v["true"][f], K=v["K"], rows=v["rows"], cols=v["cols"], depth=v["depth"][f])
    return c


CASES = ("corner", "corner_s1", "small", "small_odd", "reach0", "reach2", "radius2", "far", "mixed", "removed")
