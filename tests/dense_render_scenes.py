"""Scenes of the esl_dense_render tests: maps whose voxels are placed exactly through dense_objects_ref.voxel_frames (1 x 1 frames at
voxel centres, leaf 2^-6 so that every centre is a dyadic number), the small room of dense_scenes.room_scene, and the views (CASES) the
CPU test asserts its premises on and the GPU test renders.  Nothing here is imported by the package."""
import functools

import numpy as np

import dense_objects_ref as dor
import dense_ref as dr
import dense_scenes as sc
import dense_update_ref as dur

LEAF = 1.0 / 64
MAXV = 1 << 14
ROWS, COLS = 48, 64
KD = (256.0, 256.0, 32.0, 24.0)          # dyadic: at z = 1 a leaf is 4 pixels wide and a voxel at x = k / 64 lands on u = 4 k + 32 exactly
KH = (256.0, 256.0, 31.5, 23.5)          # ... on u + 0.5 = an integer exactly
ROOM_LEAF = 0.05
ROOM_SEED = 1          # of the seeds 0-7 the one whose views keep every margin of test_dense_render_ref.py (round, ceil, floor, zq, tol)

# the probe map (index = position in ascending packed-key order, asserted in the CPU test)
PROBE_KEYS = [(-9, 0, 63),    # 0: u = -4, footprint [-6, -2]: outside
              (-8, 0, 63),    # 1: u = 0: clipped by the left edge
              (0, -6, 63),    # 2: v = 0: clipped by the top edge
              (0, 0, -64),    # 3: behind the camera
              (0, 0, 63),     # 4: on the optical axis at z = 1
              (0, 0, 127),    # 5: on the optical axis at z = 2, hidden by 4
              (0, 6, 63),     # 6: v = 48: clipped by the bottom edge
              (3, 3, 63),     # 7: free-standing: u = 44, v = 36
              (8, 0, 63)]     # 8: u = 64: clipped by the right edge


def cam_at(x, y, z):
    """Tcw of a camera at (x, y, z) looking down the world's z axis: p_c = p - centre"""
    return [-x, -y, -z, 0.0, 0.0, 0.0, 1.0]


EYE = (0.5 / 64, 0.5 / 64, 63.5 / 64 - 1.0)          # voxel (0, 0, 63) at p_c = (0, 0, 1), voxel (kx, ky, 63) at (kx / 64, ky / 64, 1)
CAM = cam_at(*EYE)


def placed(keys, repeat=None, nudge_z=None, **over):
    """a map of voxels at the centres of `keys` (repeat[i] samples each); nudge_z[i] moves voxel i's samples along z (inside the voxel)"""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    fr = dor.voxel_frames(keys, LEAF, [i % 5 for i in range(len(keys))], repeat)
    if nudge_z is not None:
        rep = np.ones(len(keys), np.int64) if repeat is None else np.asarray(repeat)
        fr["cams"][:, 2] -= np.repeat(np.asarray(nudge_z, dtype=np.float64), rep)          # t_z = 1 - Z
    order = np.random.default_rng(len(keys)).permutation(len(fr["cams"]))
    fr = {k: (v[order] if isinstance(v, np.ndarray) else v) for k, v in fr.items()}
    over.setdefault("leaf", LEAF); over.setdefault("max_voxels", MAXV)
    m = dr.DenseMap(True, True, **over)
    if len(keys):
        m.add_frames(fr["cams"], fr["K"], fr["rows"], fr["cols"], fr["depth"], fr["bgr"], fr["inst"])
    return dict(frames=fr if len(keys) else None, params=over, map=m)


def grid_keys(n):
    """n voxels at z = 1 in rows of 17: columns u = 4 (i % 17 - 8) + 32, rows v = 4 (i // 17 - 6) + 24; the last rows leave the image"""
    return [(i % 17 - 8, i // 17 - 6, 63) for i in range(n)]


LIST_LENGTHS = (0, 1, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict(frames (dense_add_frames' arguments or None), params (esl_dense_begin's), map (the statement's DenseMap))"""
    if name == "probe":
        return placed(PROBE_KEYS)
    if name == "tie":          # voxel 0 farther than voxel 1 by 2^-25 m: zq ties, the lower index wins (viewed with footprint 1.5: they overlap)
        return placed([(0, 0, 63), (1, 0, 63)], nudge_z=[2.0 ** -25, 0.0])
    if name == "one":
        return placed([(0, 0, 63)])
    if name == "counts":          # samples per voxel: 1 2 3 1 (in key order)
        return placed([(-2, 0, 63), (0, 0, 63), (2, 0, 63), (4, 0, 63)], repeat=[1, 2, 3, 1])
    if name.startswith("grid"):
        return placed(grid_keys(int(name[4:])))
    if name == "overdraw":          # 3,200 voxels in two layers, seen from 100 m: a handful of pixels, every one a tie of many
        return placed([(i, j, kz) for i in range(40) for j in range(40) for kz in (63, 64)])
    if name == "full":          # one voxel more than the map may hold: status 3
        return placed(grid_keys(9), max_voxels=8)
    if name in ("room", "removed"):
        s = sc.room_scene(ROOM_SEED)
        over = dict(leaf=ROOM_LEAF, max_voxels=MAXV)
        m = dur.DenseUpdateMap(True, True, **over)
        m.add_frames(s["cams"], s["K"], s["rows"], s["cols"], s["depth"], s["bgr"], s["inst"])
        if name == "removed":
            m.remove_frames(s["cams"][1:2], s["K"], s["rows"], s["cols"], s["depth"][1:2], s["bgr"][1:2], s["inst"][1:2])
        return dict(frames=s, params=over, map=m, remove=[1] if name == "removed" else None)
    raise KeyError(name)


def extract(name):
    m = scene(name)["map"]
    e = m.extract()
    if e["n_voxels"] < 0:
        e["status"] = m.status
    return e


def leaf_of(name):
    return scene(name)["params"]["leaf"]


def shifted_depth(depth):
    """the room's depth images with frame 1 changed so that every class appears: the left third 0.3 m nearer, the middle untouched,
    the right third 0.3 m farther, four rows without data"""
    d = depth.astype(np.int64)
    c = depth.shape[2] // 3
    d[1, :, :c] -= 1500; d[1, :, 2 * c:] += 1500
    d[1, 10:14] = 0
    return np.clip(d, 0, 65535).astype(np.uint16)


def tol_depth():
    """five frames of constant depth around the one voxel at z = 1 with depth_scale 1024 and depth_tol 2^-4: |z_meas - z| == depth_tol
    exactly (agree), one raw unit beyond on either side (farther, nearer), and no data"""
    return np.stack([np.full((ROWS, COLS), r, np.uint16) for r in (1088, 1089, 960, 959, 0)])


def case(name):
    """-> dict(map, cams, K, rows, cols, depth_meas, params): one esl_dense_render call"""
    c = dict(map="probe", cams=[CAM], K=KD, rows=ROWS, cols=COLS, depth_meas=None, params={})
    far = cam_at(EYE[0], EYE[1], EYE[2] - 1.0)
    if name == "axis":          # the same view from 1 m and from 2 m
        c.update(cams=[CAM, far])
    elif name == "half_pixel":
        c.update(K=KH)
    elif name in ("radius0", "radius1", "radius8"):
        c.update(params=dict(max_radius=int(name[6:])))
    elif name == "footprint0":
        c.update(params=dict(footprint=0.0))
    elif name == "footprint15":
        c.update(params=dict(footprint=1.5))
    elif name == "depth_max":
        c.update(params=dict(depth_max=1.5))
    elif name == "depth_min_exact":
        c.update(params=dict(depth_min=1.0))
    elif name == "nonfinite":          # voxel 4 at p_c = (0, 0, 0): 0 / 0
        c.update(cams=[cam_at(EYE[0], EYE[1], 63.5 / 64)], params=dict(depth_min=0.0))
    elif name == "tie":
        c.update(map="tie", params=dict(footprint=1.5))
    elif name == "tol":
        c.update(map="one", cams=[CAM] * 5, depth_meas=tol_depth(), params=dict(depth_scale=1024.0, depth_tol=0.0625))
    elif name == "min_count2":
        c.update(map="counts", params=dict(min_count=2))
    elif name.startswith("grid"):
        c.update(map=name, cams=[CAM, far])
    elif name == "overdraw":
        c.update(map="overdraw", cams=[cam_at(EYE[0], EYE[1], EYE[2] - 99.0), cam_at(EYE[0] + 0.2, EYE[1] - 0.1, EYE[2] - 48.7)],
                 params=dict(depth_max=200.0))
    elif name in ("room", "room_shift", "removed"):
        s = scene("room")["frames"]
        c.update(map="removed" if name == "removed" else "room", cams=s["cams"], K=s["K"], rows=s["rows"], cols=s["cols"],
                 depth_meas=shifted_depth(s["depth"]) if name == "room_shift" else s["depth"])
    else:
        raise KeyError(name)
    c["cams"] = np.asarray(c["cams"], dtype=np.float64).reshape(-1, 7)
    return c


KNOWN = ("axis", "half_pixel", "radius0", "radius1", "radius8", "footprint0", "footprint15", "depth_max", "depth_min_exact", "nonfinite", "tie",
         "tol", "min_count2")          # dyadic scenes: decisions sit exactly on their boundaries
GENERAL = ("room", "room_shift", "removed", "overdraw")          # decisions keep the margins of dense_scenes.py
GRIDS = tuple(f"grid{n}" for n in LIST_LENGTHS)
