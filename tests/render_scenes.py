"""Scenes of the esl_render_map tests, and the conditions under which the device may be held to the numpy statement exactly
(tests/render_ref.py).  Everything is generated from a seed; nothing here is imported by the package."""
import numpy as np

import render_ref as rr

ROWS, COLS = 50, 70                      # no multiple of the 16 x 16 tile in either direction
K = (60.0, 60.0, 35.0, 25.0)             # an integer principal point
ROOM_SEEDS = tuple(range(6))             # the generator's own seeds 0-19 pass check_conditions without a search (test_render_ref.py)
ALL_ROOM_SEEDS = tuple(range(20))
CROWD_M = 257                            # one more than the kernel's chunk of 256 records

# The two formulations of step 3 (render_ref.quadric_hits, render_ref.sphere_hits) disagree by at most this much in depth over every
# scene of this file (1.20e-12 m over 130,091 hits): measured by tests/test_render_ref.py::test_two_formulations, which asserts it.
FORMULATION_GAP = 1.2e-12
# The device is compared with the statement within ten times the statements' own disagreement, and not below what closed-form double
# arithmetic on metres gives: 1e-9 m.
TOL = max(10 * FORMULATION_GAP, 1e-9)

# check_conditions: a scene in which a decision sits closer than this to its threshold is refused
MIN_DELTA = 1e-8          # |Delta| / (beta^2 + alpha |c0|) of any pixel-object pair: hit or no hit
MIN_C0 = 1e-6             # |c0|: camera inside or outside
MIN_GAP = 1e-6            # metres between the two nearest hits of a pixel (bit-identical duplicates excepted): who wins
MIN_TOL = 1e-5            # ||z_meas - z| - depth_tol| in metres: agree or not
MIN_C22 = 1e-9            # |C22| / (tco_z^2 + max s^2): which flag (wholly in front / behind / across the principal plane)


def check_conditions(ref):
    m = ref["margins"]
    assert m["delta"] >= MIN_DELTA, ("a ray grazes a body", m)
    assert m["c0"] >= MIN_C0, ("a camera centre on a body's surface", m)
    assert m["gap"] >= MIN_GAP, ("two bodies at one depth on one pixel", m)
    assert m["tol"] >= MIN_TOL, ("a measured sample at the edge of the tolerance", m)
    assert m["c22"] >= MIN_C22, ("a body tangent to the principal plane", m)
    return ref


def quat(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])


def ell(c, s, q=(0, 0, 0, 1.0)):
    return np.concatenate([np.asarray(c, dtype=np.float64), np.asarray(q, dtype=np.float64), np.asarray(s, dtype=np.float64)])


def sphere(c, r):
    return ell(c, [r, r, r])


IDENTITY_CAM = np.array([0, 0, 0, 0, 0, 0, 1.0])


def random_cams(rng, n):
    """Tcw of cameras near the origin looking along +z: up to 0.2 m off, up to 0.1 rad turned"""
    cams = np.zeros((n, 7))
    for f in range(n):
        cams[f, :3] = rng.uniform(-0.2, 0.2, 3)
        cams[f, 3:] = quat(rng.normal(size=3), rng.uniform(-0.1, 0.1))
    return cams


def room_scene(seed, n_objs=12, n_cams=3):
    """12 ellipsoids at z = 1.5 .. 6 m in front of 3 cameras: they overlap in the image, some only partly inside it"""
    rng = np.random.default_rng(1000 + seed)
    objs = np.zeros((n_objs, 10))
    for m in range(n_objs):
        z = rng.uniform(1.5, 6.0)
        c = [rng.uniform(-0.6, 0.6) * z, rng.uniform(-0.45, 0.45) * z, z]
        objs[m] = ell(c, rng.uniform(0.15, 0.6, 3), quat(rng.normal(size=3), rng.uniform(0, np.pi)))
    return dict(cams=random_cams(rng, n_cams), objs=objs, K=K, rows=ROWS, cols=COLS)


def crowd_scene(seed=0):
    """257 small ellipsoids, 30 of them planted on the rays of the tile of columns 16-31, rows 16-31; one camera"""
    rng = np.random.default_rng(2000 + seed)
    objs = np.zeros((CROWD_M, 10))
    for m in range(CROWD_M):
        z = rng.uniform(1.5, 6.0)
        if m % 8 == 0 and m < 240:          # spread over both chunks' worth of indices
            u, v = rng.uniform(18, 29), rng.uniform(18, 29)
        else:
            u, v = rng.uniform(-5, COLS + 5), rng.uniform(-5, ROWS + 5)
        c = [(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z]
        objs[m] = ell(c, rng.uniform(0.03, 0.12, 3) * z / 2, quat(rng.normal(size=3), rng.uniform(0, np.pi)))
    return dict(cams=IDENTITY_CAM[None, :].copy(), objs=objs, K=K, rows=ROWS, cols=COLS)


def occluder_scene():
    """B, a sphere of radius 0.5 at (0, 0, 4), behind two thin ellipsoids at z = 2 and 2.1 that each hide about 0.6 of it and together
    all of it; worked by hand, the premises are asserted by the tests through the statements.  The second occluder and the principal
    point are moved off the symmetric position: there the two occluders tie in depth where they overlap and rays graze exactly."""
    objs = np.stack([sphere([0, 0, 4.0], 0.5), ell([-0.45, 0, 2.0], [0.5, 1.0, 0.05]), ell([0.47, 0.01, 2.1], [0.5, 1.0, 0.05])])
    return dict(cams=IDENTITY_CAM[None, :].copy(), objs=objs, K=(120.0, 120.0, 80.37, 60.21), rows=120, cols=160)


def across_scene():
    """a long ellipsoid that crosses the camera's principal plane (the camera outside it), a sphere behind it in the image"""
    objs = np.stack([ell([0.4, 0.1, 0.5], [0.15, 0.12, 2.0], quat([0, 1, 0], 0.15)), sphere([-0.3, 0.0, 3.0], 0.6)])
    return dict(cams=IDENTITY_CAM[None, :].copy(), objs=objs, K=K, rows=ROWS, cols=COLS)


def nothing_scene():
    """camera inside; NaN, zero axis, zero quaternion; wholly behind"""
    objs = np.stack([sphere([0.1, 0, 0.2], 1.0), sphere([0, 0, 3.0], 0.5), sphere([0, 0, 3.0], 0.5), sphere([0, 0, 3.0], 0.5),
                     sphere([0.2, 0.1, -3.0], 0.5)])
    objs[1, 1] = np.nan; objs[2, 8] = 0.0; objs[3, 3:7] = 0.0
    return dict(cams=IDENTITY_CAM[None, :].copy(), objs=objs, K=K, rows=ROWS, cols=COLS)


def reference(scene, depth_meas=None, **over):
    return rr.render(scene["cams"], scene["objs"], scene["K"], scene["rows"], scene["cols"], depth_meas, **over)


def planted_depth(ref, seed=0):
    """A measured depth for the statement's render `ref`: on the pixels an object wins z, z + 3 tol, z - 3 tol, raw 0, a sample beyond
    depth_max, in turn along the pixels of each frame; elsewhere raw 0.  Quantised to uint16; the planted offsets (3 tol = 0.15 m) stand
    far from the tolerance after quantisation (1 / depth_scale = 0.2 mm)."""
    p = ref["params"]
    F, rows, cols = ref["depth"].shape
    raw = np.zeros((F, rows, cols), dtype=np.uint16)
    rng = np.random.default_rng(3000 + seed)
    for f in range(F):
        ys, xs = np.nonzero(ref["inst"][f] >= 0)
        kind = rng.integers(0, 5, len(ys))
        z = ref["depth"][f][ys, xs]
        zm = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [z, z + 3 * p["depth_tol"], z - 3 * p["depth_tol"], 0.0],
                       p["depth_max"] + 1.0)
        raw[f][ys, xs] = np.clip(np.rint(zm * p["depth_scale"]), 0, 65535).astype(np.uint16)
    return raw
