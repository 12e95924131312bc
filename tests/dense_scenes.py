"""Scenes of the esl_dense_* tests, and the conditions under which the device may be held to the numpy statement exactly
(tests/dense_ref.py).  Everything is generated from a seed; nothing here is imported by the package."""
import numpy as np

import dense_ref as dr
import render_ref as rr
import render_scenes as rs

ROWS, COLS = 48, 64
K = (60.0, 60.0, 31.5, 23.5)
ROOM_SEEDS = (2, 4)                      # of the seeds 0-7 these (and 1, 6, 7) pass check_conditions at every leaf and stride of the tests;
                                         # seed 0 passes at stride 1 and is the scene of the other tests
DEPTH_SCALE = 5000.0
NEGATIVE_SHIFT = (-3.0, -2.5, -6.0)         # room_scene(shift=...): the wall at negative world coordinates on all axes

# check_conditions: a scene in which a decision sits closer than this to its threshold is refused
MIN_KEY = 1e-9           # |p_w[a] / leaf - nearest integer|: which voxel
MIN_FIX = 1e-5           # |p_w[a] 2^30 - nearest half-integer|: which way the fixed-point term rounds


def wall_depth(cam, Kx, rows, cols, n_w, d_w):
    """z of the world plane n_w . p = d_w along the ray of every pixel of the camera Tcw = cam"""
    R, t = dr.pose(cam)
    n_c = R @ n_w
    dx, dy = rr.pixel_rays(Kx, rows, cols)
    return (d_w + n_c @ t) / (n_c[0] * dx + n_c[1] * dy + n_c[2])


def room_scene(seed, n_cams=3, rows=ROWS, cols=COLS, Kx=K, shift=None):
    """F = 3 poses a few centimetres and degrees apart looking at a slanted wall 2 m away, three ellipsoids in front of it whose
    pixels carry their index as label (esl_render_map's statement), the wall labelled in patches so that voxels get mixed votes, 5 % of
    the depth set to 0, random colours.  shift: the whole world (wall, bodies, camera centres) moved by this vector"""
    rng = np.random.default_rng(7000 + seed)
    shift = np.zeros(3) if shift is None else np.asarray(shift, dtype=np.float64)
    cams = np.zeros((n_cams, 7))
    for f in range(n_cams):
        cams[f, :3] = rng.uniform(-0.04, 0.04, 3)
        cams[f, 3:] = rs.quat(rng.normal(size=3), rng.uniform(-0.05, 0.05)) * rng.uniform(0.5, 2.0)          # not normalised
        cams[f, :3] -= dr.pose(cams[f])[0] @ shift          # p_c = R (p_w + shift) + t
    n_w = np.array([0.25, -0.1, 1.0]); n_w /= np.linalg.norm(n_w)
    objs = np.stack([rs.ell([-0.5, -0.2, 1.5], [0.25, 0.3, 0.2], rs.quat([0, 1, 0], 0.3)),
                     rs.ell([0.1, 0.15, 1.3], [0.3, 0.2, 0.25], rs.quat([1, 0, 1], 0.5)),
                     rs.ell([0.45, -0.1, 1.6], [0.2, 0.35, 0.2], rs.quat([0, 0, 1], 0.8))])
    objs[:, :3] += shift
    ren = rr.render(cams, objs, Kx, rows, cols, margins=False)
    depth = np.zeros((n_cams, rows, cols), np.uint16); inst = np.full((n_cams, rows, cols), -1, np.int32)
    for f in range(n_cams):
        zw = wall_depth(cams[f], Kx, rows, cols, n_w, 2.0 * n_w[2] + n_w @ shift)
        ze = np.where(np.isnan(ren["depth"][f]), np.inf, ren["depth"][f])
        front = ze < zw
        z = np.where(front, ze, zw)
        depth[f] = np.clip(np.rint(z * DEPTH_SCALE), 1, 65535).astype(np.uint16)
        rw, cl = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        wall = np.where(rw % 11 == 0, -1, 10 + (cl // 5 + rw // 7) % 3)          # the wall in patches of three ids, some rows unlabelled
        inst[f] = np.where(front, ren["inst"][f], wall)
    depth[rng.random(depth.shape) < 0.05] = 0
    bgr = rng.integers(0, 256, (n_cams, rows, cols, 3), dtype=np.uint8)
    return dict(cams=cams, K=Kx, rows=rows, cols=cols, depth=depth, bgr=bgr, inst=inst)


def reference(scene, calls=None, with_color=True, with_inst=True, **over):
    """the statement's map of a scene; calls: lists of frame indices, one list per esl_dense_add_frames call (default: one call)"""
    m = dr.DenseMap(with_color, with_inst, **over)
    F = len(scene["cams"])
    adds = []
    for idx in (calls if calls is not None else [list(range(F))]):
        adds.append(m.add_frames(scene["cams"][idx], scene["K"], scene["rows"], scene["cols"], scene["depth"][idx], scene["bgr"][idx],
                                 scene["inst"][idx]))
    return m, adds


def check_conditions(m, two_frames=True, min_largest=0):
    """on the reference alone: the conditions that make exact equality a fair demand"""
    mg = m.margins()
    assert mg["key"] >= MIN_KEY, ("a sample on a voxel boundary", mg)
    assert mg["fix"] >= MIN_FIX, ("a fixed-point term at a rounding tie", mg)
    if two_frames:
        _, inv = np.unique(m.key, return_inverse=True)
        lo = np.full(inv.max() + 1, np.iinfo(np.int64).max); hi = np.full(inv.max() + 1, -1)
        np.minimum.at(lo, inv, m.frame); np.maximum.at(hi, inv, m.frame)
        assert (hi > lo).any(), "no voxel receives samples from two different frames"
    if min_largest:
        assert np.unique(m.key, return_counts=True)[1].max() >= min_largest, "the largest count is too small"
    return m
