"""Scenes of the esl_dense_carve_frames tests, everything from fixed numbers: dense_align_scenes' 4 x 3 x 2.5 m room seen from its six
map views with a box on the floor in the first three (`ghost`, `ghost_odd`, a stride-2 and a coloured / labelled form), and maps of a
few voxels placed exactly at dyadic points (point_frames) with tiny observer images whose every class is known by hand (EXACT).  The CPU
test asserts its premises on these, the GPU test runs them.  Nothing here is imported by the package."""
import functools

import numpy as np

import dense_align_scenes as das
import dense_ref as dr
import dense_update_ref as dur

LEAF = das.LEAF
# the box: 0.4 x 0.4 x 0.6 m, axis-aligned, on the floor, its faces in the middle of voxels like the room's walls
BOX_LO = das.LO + np.array([0.8, 0.9, 0.0])
BOX_HI = BOX_LO + np.array([0.4, 0.4, 0.6])
N_BOX_FRAMES = 3


def box_hit(cam, Kx, rows, cols, lo=BOX_LO, hi=BOX_HI):
    """per pixel the z at which its ray enters the box, inf where it misses (the slab test; the camera is outside the box)"""
    R, t = dr.pose(cam)
    o = -R.T @ t
    fx, fy, cx, cy = Kx
    rr_, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    d_c = np.stack([(cc - cx) / fx, (rr_ - cy) / fy, np.ones_like(cc, dtype=np.float64)], axis=-1)
    d_w = d_c @ R
    with np.errstate(all="ignore"):
        t1 = (lo - o) / d_w; t2 = (hi - o) / d_w
        near = np.minimum(t1, t2).max(axis=-1); far = np.maximum(t1, t2).min(axis=-1)
    return np.where((near <= far) & (near > 0), near, np.inf)


@functools.lru_cache(maxsize=None)
def ghost(rows=48, cols=64, stride=1, labelled=False):
    """-> dict(cams (6, 7), K, rows, cols, depth (6, rows, cols) with the box in the first three, hit (6, rows, cols) bool: the pixels
    that show the box, bgr, inst (None unless labelled), params (esl_dense_begin's), with_color, with_inst)"""
    s = cols / das.COLS
    Kx = (das.K[0] * s, das.K[1] * s, (cols - 1) / 2, (rows - 1) / 2)          # as dense_align_scenes.views scales it
    cams = np.stack([das.look_at(das.LO + np.array(o), das.LO + np.array(t)) for o, t in das.MAP_VIEWS])
    depth = np.stack([das.box_depth(c, Kx, rows, cols) for c in cams])
    hit = np.zeros(depth.shape, bool)
    for f in range(N_BOX_FRAMES):
        zb = box_hit(cams[f], Kx, rows, cols)
        raw = np.clip(np.rint(np.where(np.isfinite(zb), zb, 0.0) * das.DEPTH_SCALE), 1, 65535).astype(np.uint16)
        hit[f] = np.isfinite(zb) & (raw < depth[f])
        depth[f] = np.where(hit[f], raw, depth[f])
    bgr = inst = None
    if labelled:          # the box is instance 1, the room instance 0; a colour that depends on the pixel and the frame
        inst = hit.astype(np.int32)
        f_, r_, c_ = np.meshgrid(np.arange(6), np.arange(rows), np.arange(cols), indexing="ij")
        bgr = np.stack([(7 * r_ + f_) % 256, (5 * c_ + 3 * f_) % 256, np.where(hit, 200, 40)], axis=-1).astype(np.uint8)
    return dict(cams=cams, K=Kx, rows=rows, cols=cols, depth=depth, hit=hit, bgr=bgr, inst=inst,
                params=dict(das.MAP_PARAMS, stride=stride), with_color=labelled, with_inst=labelled)


GHOSTS = dict(ghost=(48, 64, 1, False), ghost_odd=(45, 61, 1, False), ghost_stride2=(48, 64, 2, False), ghost_labelled=(48, 64, 1, True))


def ghost_scene(name):
    return ghost(*GHOSTS[name])


def build(sc, frames=None):
    """a fresh statement map of the scene's frames (all of them, or the listed ones)"""
    m = dur.DenseUpdateMap(sc["with_color"], sc["with_inst"], **sc["params"])
    f = slice(None) if frames is None else list(frames)
    m.add_frames(sc["cams"][f], sc["K"], sc["rows"], sc["cols"], sc["depth"][f], None if sc["bgr"] is None else sc["bgr"][f],
                 None if sc["inst"] is None else sc["inst"][f])
    return m


def voxel_origin(sc, m):
    """per voxel of m.extract()'s order: (samples from box pixels, samples from other pixels) as two int arrays"""
    ext = m.extract()
    index = {int(k): i for i, k in enumerate(dr.pack(ext["key"]).tolist())}
    box = np.zeros(ext["n_voxels"], np.int64); other = np.zeros(ext["n_voxels"], np.int64)
    for f in range(len(sc["cams"])):
        s = dr.samples(sc["cams"][f], sc["K"], sc["rows"], sc["cols"], sc["depth"][f], m.p)
        i = np.array([index[int(k)] for k in dr.pack(s["k"]).tolist()], np.int64)
        h = sc["hit"][f][s["row"], s["col"]]
        np.add.at(box, i[h], 1); np.add.at(other, i[~h], 1)
    return box, other


# ---- exact scenes: voxels at dyadic points seen by an identity camera, so p_c = the point -------------------------------------------
IDENT = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
EXACT_PARAMS = dict(depth_scale=1024.0, depth_min=0.1, depth_max=6.0, depth_tol=0.0625, min_through=1)
A, N_, T_, Z = 1024, 512, 2048, 0          # raw values that agree with, lie nearer than, lie beyond z = 1, and no data


def _img(rows):
    return np.array(rows, np.uint16)


def exact(name):
    """-> dict(points, K, rows, cols, depth (F, rows, cols), params, want: {point: [class per frame]}); the map is point_frames(points)
    at leaf 1 / 64, every observer pose is the identity"""
    if name == "tol":          # |z_m - z| == depth_tol on both sides agrees, one raw unit more does not; then no data
        return dict(points=[(0, 0, 1)], K=(1.0, 1.0, 0.0, 0.0), depth=_img([[[1088]], [[1089]], [[960]], [[959]], [[0]]]),
                    params=dict(window=0), want={(0, 0, 1): [0, 2, 0, 1, 3]})
    if name == "gate":         # z == depth_min and z == depth_max are in; one voxel beyond each is out.  z_m = 1.5 m
        return dict(points=[(0, 0, 0.984375), (0, 0, 1), (0, 0, 2), (0, 0, 2.015625)], K=(1.0, 1.0, 0.0, 0.0), depth=_img([[[1536]]]),
                    params=dict(window=0, depth_min=1.0, depth_max=2.0), want={(0, 0, 0.984375): [4], (0, 0, 1): [2], (0, 0, 2): [1], (0, 0, 2.015625): [4]})
    if name == "half":         # u + 0.5 = v + 0.5 = 1 exactly: the upper pixel, which alone agrees
        return dict(points=[(0, 0, 1)], K=(1.0, 1.0, 0.5, 0.5), depth=_img([[[T_, T_], [T_, A]]]), params=dict(window=0), want={(0, 0, 1): [0]})
    if name == "border":       # the centre pixel on each border of a 3 x 3 image, the window clipped; one column / row beyond: outside
        pts = [(-1, 0, 1), (1, 0, 1), (0, -1, 1), (0, 1, 1), (2, 0, 1), (-2, 0, 1), (0, 2, 1), (0, -2, 1)]
        d = _img([[[Z, Z, A], [Z, Z, A], [Z, Z, A]],          # only column 2 holds data: the voxel at column 0 reads columns 0 and 1
                  [[Z, Z, Z], [Z, Z, Z], [T_, T_, T_]],       # only row 2: the voxel at row 0 reads rows 0 and 1
                  [[N_, Z, Z], [N_, Z, Z], [N_, Z, Z]],       # only column 0
                  [[A, A, A], [Z, Z, Z], [Z, Z, Z]]])         # only row 0
        return dict(points=pts, K=(1.0, 1.0, 1.0, 1.0), depth=d, params=dict(window=1),
                    want={(-1, 0, 1): [3, 2, 1, 0], (1, 0, 1): [0, 2, 3, 0], (0, -1, 1): [0, 3, 1, 0], (0, 1, 1): [0, 2, 1, 3],
                          (2, 0, 1): [5] * 4, (-2, 0, 1): [5] * 4, (0, 2, 1): [5] * 4, (0, -2, 1): [5] * 4})
    if name in ("mix", "mix_w0"):          # a window with agree + farther, with nearer + farther, with only zeros, with only farther
        d = _img([[[A, T_, T_], [T_, T_, T_], [T_, T_, T_]], [[T_, T_, T_], [T_, T_, T_], [T_, T_, N_]], [[Z] * 3] * 3, [[T_] * 3] * 3])
        w = 1 if name == "mix" else 0
        return dict(points=[(0, 0, 1)], K=(1.0, 1.0, 1.0, 1.0), depth=d, params=dict(window=w), want={(0, 0, 1): [0, 1, 3, 2] if w else [2, 2, 3, 2]})
    raise KeyError(name)


EXACT = ("tol", "gate", "half", "border", "mix", "mix_w0")
EXACT_MAP = dict(leaf=das.PLEAF, max_voxels=1 << 12)


@functools.lru_cache(maxsize=None)
def exact_scene(name):
    e = exact(name)
    fr = das.point_frames(e["points"])
    F, rows, cols = e["depth"].shape
    sc = dict(cams=fr["cams"], K=fr["K"], rows=fr["rows"], cols=fr["cols"], depth=fr["depth"], bgr=None, inst=None, hit=None,
              params=dict(EXACT_MAP), with_color=False, with_inst=False)
    return dict(map=sc, cams_obs=np.tile(np.array(IDENT), (F, 1)), depth_obs=e["depth"], K=e["K"], rows=rows, cols=cols,
                params=dict(EXACT_PARAMS, **e["params"]), want=e["want"], points=e["points"])


def exact_classes(name, m):
    """the hand-made classes as an (F, n) array in m.extract()'s order"""
    e = exact_scene(name)
    ext = m.extract()
    index = {tuple(k): i for i, k in enumerate(ext["key"].tolist())}
    F = len(e["depth_obs"])
    out = np.full((F, ext["n_voxels"]), -1, np.int64)
    for pt, cls in e["want"].items():
        key = tuple(int(np.floor(v / das.PLEAF)) for v in pt)
        out[:, index[key]] = cls
    assert (out >= 0).all()
    return out


def full_scene():
    """dense_align_scenes' map over its capacity (status 3) with the `tol` observers"""
    s = das.scene("full")
    fr = s["frames"]
    return dict(cams=fr["cams"], K=fr["K"], rows=fr["rows"], cols=fr["cols"], depth=fr["depth"], bgr=None, inst=None, hit=None,
                params=dict(s["params"]), with_color=False, with_inst=False)
