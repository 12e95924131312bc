"""Voxel sets of the esl_dense_planes tests, shared by the CPU tests of the statement and the GPU tests: the CPU side asserts on the
statement alone what the GPU side relies on.  Each scene is (keys (n, 3), repeat (n,) samples per voxel or None, labels (n,)), placed
through dense_objects_ref.voxel_frames; everything is generated from fixed seeds.  Nothing here is imported by the package."""
import functools

import numpy as np

import dense_ref as dr
import dense_objects_ref as dor
import dense_scenes as sc

LEAF = 0.01
MAXV = 65536
PLANTED = dict(dist_tol=0.004, min_baseline=4, min_inliers=50)          # the parameters of the planted scene


def grid(nx, ny):
    return np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), axis=-1).reshape(-1, 2)


def slab_z(nx, ny, z=0, origin=(0, 0)):
    g = grid(nx, ny) + np.array(origin)
    return np.concatenate([g, np.full((len(g), 1), z)], axis=-1)


def planted_keys():
    """slabs kz = 0 (40 x 40), kx + kz = 60 (30 x 30), ky = 45 (20 x 20) and 150 clutter voxels: 3,047 voxels"""
    A = slab_z(40, 40)
    B = np.array([(x, y, 60 - x) for x in range(20, 50) for y in range(30)])
    C = np.array([(x, 45, z) for x in range(20) for z in range(5, 25)])
    D = np.random.default_rng(1).integers(0, 50, size=(150, 3))
    return np.unique(np.concatenate([A, B, C, D]), axis=0)


def planted_truth(keys):
    """per voxel the set of planted planes that contain it: bit 0 kz = 0, bit 1 kx + kz = 60, bit 2 ky = 45 (inside the slabs' extents)"""
    k = keys
    a = (k[:, 2] == 0) & (k[:, 0] < 40) & (k[:, 1] < 40)
    b = (k[:, 0] + k[:, 2] == 60) & (k[:, 0] >= 20) & (k[:, 0] < 50) & (k[:, 1] < 30)
    c = (k[:, 1] == 45) & (k[:, 0] < 20) & (k[:, 2] >= 5) & (k[:, 2] < 25)
    return a.astype(int) | (b.astype(int) << 1) | (c.astype(int) << 2)


def thick_slab_keys():
    """two voxels thick around the plane x + 2 y + 5 z = 0 over 30 x 30 columns: z = round(-(x + 2 y) / 5) and the voxel above"""
    g = grid(30, 30)
    z = np.rint(-(g[:, 0] + 2 * g[:, 1]) / 5.0).astype(int)
    return np.concatenate([np.concatenate([g, z[:, None]], axis=-1), np.concatenate([g, z[:, None] + 1], axis=-1)])


def rejected_keys():
    """the slab kz = 0 (30 x 30) with a strip of a second layer at one end and a few voxels below at the other: the least-squares
    plane tilts and loses inliers that the winner, a lattice plane, holds (the CPU test asserts refined = 2)"""
    return np.concatenate([slab_z(30, 30), slab_z(3, 30, 1, (27, 0)), slab_z(2, 30, 2, (28, 0)), slab_z(2, 30, -2, (0, 0))])


def build(name):
    """-> (keys, repeat or None, labels, with_inst)"""
    rep, inst = None, True
    if name == "planted":
        keys = planted_keys()
    elif name == "slab":
        keys = slab_z(40, 40)
    elif name == "diag":
        keys = np.array([(x, y, 60 - x) for x in range(20, 50) for y in range(30)])
    elif name.startswith("len"):          # len<n>: a slab of n - 5 voxels in rows of 32 and 5 voxels off it
        n = int(name[3:]) - 5
        g = np.stack([np.arange(n) % 32, np.arange(n) // 32, np.zeros(n, int)], axis=-1)
        keys = np.concatenate([g, np.array([[3, 3, 7], [9, 1, 12], [14, 5, 9], [20, 2, 15], [27, 4, 6]])])
    elif name.startswith("few"):          # few<n>: the first n of four voxels, the first three of them not collinear
        keys = np.array([[0, 0, 0], [9, 0, 0], [0, 9, 1], [5, 5, 5]])[:int(name[3:])]
    elif name == "line3":
        keys = np.array([[0, 0, 0], [9, 9, 0], [18, 18, 0]])
    elif name == "layers":
        keys = np.concatenate([slab_z(30, 30, 0), slab_z(30, 30, 1)])
    elif name == "twins_samples":          # two congruent slabs, the second with two samples per voxel
        keys = np.concatenate([slab_z(20, 20, 0), slab_z(20, 20, 30, (25, 0))])
        rep = np.array([1] * 400 + [2] * 400)
    elif name == "twins":
        keys = np.concatenate([slab_z(20, 20, 0), slab_z(20, 20, 30, (25, 0))])
    elif name == "gates":          # a slab whose voxels carry 1 or 2 samples in stripes; a second, labelled slab; unlabelled clutter
        keys = np.concatenate([slab_z(24, 24, 0), slab_z(20, 20, 12), np.random.default_rng(2).integers(0, 24, (40, 3)) + np.array([0, 0, 20])])
        keys = keys[np.unique(keys, axis=0, return_index=True)[1]]
        rep = np.where((keys[:, 2] == 0) & (keys[:, 0] % 3 == 0), 1, 2)
        lab = np.where(keys[:, 2] == 12, 4, -1)
        return keys, rep, lab, True
    elif name == "gates_nolabels":
        keys, rep, _, _ = build("gates")
        return keys, rep, np.full(len(keys), -1), False
    elif name == "thick":
        keys = thick_slab_keys()
    elif name == "rejected":
        keys = rejected_keys()
    else:
        raise KeyError(name)
    assert len(np.unique(keys, axis=0)) == len(keys), name
    return keys, rep, np.full(len(keys), -1), inst


@functools.lru_cache(maxsize=None)
def scene(name, shuffle=11):
    """-> dict(frames = the arguments of dense_add_frames in a shuffled order, ext = the statement's extract, with_inst, leaf)"""
    if name == "room":
        s = sc.room_scene(0)
        m, _ = sc.reference(s, leaf=0.05, max_voxels=MAXV)
        sc.check_conditions(m)
        return dict(frames=s, ext=m.extract(), with_inst=True, leaf=0.05)
    keys, rep, lab, inst = build(name)
    s = dor.voxel_frames(keys, LEAF, lab, rep)
    idx = np.random.default_rng(shuffle).permutation(len(s["cams"]))
    s = dict(s, cams=s["cams"][idx], depth=s["depth"][idx], bgr=s["bgr"][idx], inst=s["inst"][idx])
    m = dr.DenseMap(True, inst, leaf=LEAF, max_voxels=MAXV)
    m.add_frames(s["cams"], s["K"], 1, 1, s["depth"], s["bgr"], s["inst"])
    sc.check_conditions(m, two_frames=False)
    e = m.extract()
    assert e["n_voxels"] == len(keys)
    return dict(frames=s, ext=e, with_inst=inst, leaf=LEAF)


# room_scene has no floor: its one surface is the slanted wall 2 m in front of the cameras.  The tests take "towards the cameras" as up,
# so that the wall is the ground; with the scene's own up, (0, -1, 0), no plane is a candidate, which the GPU test asserts too.
ROOM_UP = (0.0, 0.0, -1.0)
ROOM = dict(dist_tol=0.03, min_inliers=200, n_hypotheses=128, up=ROOM_UP)
