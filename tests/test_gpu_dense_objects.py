"""esl_dense_objects on the device against its numpy statement (tests/dense_objects_ref.py).

Voxel sets are placed exactly through esl_dense_add_frames: one 1 x 1 frame per sample at a voxel's centre (dense_objects_ref.voxel_frames),
so every sample is half a voxel from a boundary; the frames are given in a shuffled order and dense_scenes.check_conditions runs on every
scene.  Integer outputs (stats, comp, voxel_comp, result) are compared exactly.  objs is compared at 1e-9 absolute (metres, quaternion
components): both sides start from identical integers and identical IEEE operations and can differ only by the last-place rounding of
atan2, cos, sin and sqrt between two math libraries -- about 1e-15 m on a coordinate of a few metres; 1e-9 is six orders above that and
seven below a voxel.  That holds where the planar covariance is clearly anisotropic, which is asserted on the statement's side."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as dr                # noqa: E402
import dense_objects_ref as dor       # noqa: E402
import dense_scenes as sc             # noqa: E402

pytestmark = pytest.mark.gpu

MAXV = 65536
LEAF = 0.05
FLOOR = (0.0, 0.0, 1.0, 0.0)
TILTED = (0.1, -0.05, 1.0, 0.2)
OBJ_TOL = 1e-9
MIN_ANISOTROPY = 0.05          # sqrt((C_uu - C_vv)^2 + 4 C_uv^2) / (C_uu + C_vv): a yaw error of 1e-16 / this, times a few metres
INTS = ("stats", "comp", "voxel_comp")


def block(n, origin=(0, 0, 0)):
    k = np.stack(np.meshgrid(*[np.arange(c) for c in n], indexing="ij"), axis=-1).reshape(-1, 3)
    return k + np.array(origin)


# ---- scenes: (keys, labels, repeat) -----------------------------------------------------------------------------------------------------------
def snake_keys(n=1500):
    """a one-voxel-wide serpentine: rows along x, 4 voxels apart in y, walked to and fro with axis, edge-diagonal and corner-diagonal
    steps (y and z wobble by one inside a row), joined at their ends by axis steps in y; starts at negative x and y"""
    moves = [(1, 0, 0), (1, 1, 1), (1, 0, 0), (1, -1, -1), (1, 0, 1), (1, 0, -1)]
    k, out, sgn = [-60, -22, 2], [], 1
    out.append(tuple(k))
    while len(out) < n:
        for s in range(102):          # a multiple of the cycle: the row ends with the wobble at rest
            m = moves[s % len(moves)]
            k = [k[0] + sgn * m[0], k[1] + m[1], k[2] + m[2]]
            out.append(tuple(k))
        for _ in range(4):
            k = [k[0], k[1] + 1, k[2]]
            out.append(tuple(k))
        sgn = -sgn
    out = np.array(out[:n], dtype=np.int64)
    assert len(np.unique(out, axis=0)) == n
    return out


def gates_scene():
    keys = [block((4, 3, 5)), block((4, 3, 5), (8, 0, 0)), block((4, 3, 1), (4, 0, 0))]          # two towers and a bridge in the lowest layer
    n = sum(len(k) for k in keys)
    labels = [[0, 0, 0]] * n
    keys.append(np.array([[1, 1, 5], [9, 1, 5], [20, 0, 3], [20, 5, 3]]))
    labels += [[0, 0, 1], [0], [-1, -1, -1], [5, 5, 5]]          # votes 2 : 1; one sample; unlabelled; a label beyond N
    return np.concatenate(keys), labels


def box_scene():
    """the voxels whose centre lies in a 0.6 x 0.4 x 0.3 m box, yawed by 0.4 rad in the gravity frame of TILTED, its base 0.1 m above it"""
    n, d, u, v = dor.plane(TILTED)
    n, u, v = np.array(n), np.array(u), np.array(v)
    x = np.cos(0.4) * u + np.sin(0.4) * v
    y = np.cross(n, x)
    c0 = 0.7 * u - 0.4 * v + (0.25 - d) * n          # height 0.25: the base at 0.1
    g = block((40, 40, 40), np.floor(c0 / LEAF).astype(int) - 20)
    p = (g + 0.5) * LEAF - c0
    inside = (np.abs(p @ x) <= 0.3) & (np.abs(p @ y) <= 0.2) & (np.abs(p @ n) <= 0.15)
    return g[inside], c0


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict(frames = the arguments of dense_add_frames in a shuffled order, map = the statement's map, ext = its extract)"""
    if name == "room":
        s = sc.room_scene(0)
        m, _ = sc.reference(s, leaf=LEAF, max_voxels=MAXV)
        sc.check_conditions(m)
        return dict(frames=s, map=m, ext=m.extract())
    rep = None
    if name == "snake":
        keys = snake_keys(); lab = np.zeros(len(keys), int)
    elif name.startswith("gap"):          # gap<g>: two 3 x 3 x 3 blobs whose nearest voxels are at Chebyshev distance g (and 1 in y)
        g = int(name[3:])
        keys = np.concatenate([block((3, 3, 3), (-1, 0, 2)), block((3, 3, 3), (1 + g, 3, 2))]); lab = np.zeros(len(keys), int)
    elif name == "slabs":          # two labels in face contact, interleaved along x
        keys = block((8, 6, 4), (-3, -2, 1)); lab = (keys[:, 0] - keys[:, 0].min()) % 2
    elif name == "tie":          # two components of equal size in label 0, a larger one in label 1
        keys = np.concatenate([block((5, 3, 2), (6, 0, 2)), block((5, 3, 2), (-9, 4, 2)), block((6, 3, 2), (0, 20, 2))])
        lab = np.array([0] * 60 + [1] * 36)
    elif name == "gates":
        keys, lab = gates_scene()
    elif name == "box":
        keys = box_scene()[0]; lab = np.full(len(keys), 1)
    elif name == "block":
        keys = block((12, 8, 6)); lab = np.zeros(len(keys), int)
    else:
        raise KeyError(name)
    s = dor.voxel_frames(keys, LEAF, lab, rep)
    idx = np.random.default_rng(11).permutation(len(s["cams"]))
    s = dict(s, cams=s["cams"][idx], depth=s["depth"][idx], bgr=s["bgr"][idx], inst=s["inst"][idx])
    m = dr.DenseMap(leaf=LEAF, max_voxels=MAXV)
    m.add_frames(s["cams"], s["K"], 1, 1, s["depth"], s["bgr"], s["inst"])
    sc.check_conditions(m, two_frames=False)
    e = m.extract()
    assert e["n_voxels"] == len(np.unique(keys, axis=0))
    return dict(frames=s, map=m, ext=e)


def dev_add(cx, s, idx=None):
    idx = slice(None) if idx is None else idx
    return cx.dense_add_frames(s["cams"][idx], s["K"], s["rows"], s["cols"], s["depth"][idx], s["bgr"][idx], s["inst"][idx])


def dev_build(pkg, cx, name, **over):
    over.setdefault("leaf", LEAF); over.setdefault("max_voxels", MAXV)
    cx.dense_begin(pkg.abi.default_dense_params(**over))
    dev_add(cx, scene(name)["frames"])


def ref_objects(name, N, ground, **kw):
    return dor.objects(scene(name)["ext"], LEAF, N, ground, **kw)


def split(kw):
    caps = {k: kw[k] for k in ("comp_cap", "voxel_cap") if k in kw}
    return caps, {k: v for k, v in kw.items() if k not in caps}


def assert_same(dev, ref, objs=True):
    assert dev["result"] == ref["result"]
    for k in INTS:
        assert dev[k].dtype == np.int32 and dev[k].shape == ref[k].shape, k
        if not np.array_equal(dev[k], ref[k]):
            bad = np.argwhere(dev[k] != ref[k])[:5]
            raise AssertionError((k, bad.tolist(), dev[k][tuple(bad[0])], ref[k][tuple(bad[0])]))
    assert dev["objs"].shape == ref["objs"].shape
    if objs:
        assert ref["margins"]["height"] >= 1e-9, "a voxel centre on the plane_dist threshold"
        for o, an in ref["margins"]["anisotropy"].items():
            assert an >= MIN_ANISOTROPY, ("an isotropic footprint: the yaw is not determined", o, an)
        err = np.abs(dev["objs"] - ref["objs"])
        print("max |objs - statement| =", err.max() if err.size else 0.0)
        assert (err <= OBJ_TOL).all(), err.max()


def check(pkg, cx, name, N, ground=FLOOR, objs=True, **kw):
    caps, par = split(kw)
    dev = cx.dense_objects(N, ground, pkg.abi.default_dense_obj_params(**par), **caps)
    ref = ref_objects(name, N, ground, **kw)
    assert_same(dev, ref, objs)
    return dev, ref


def same_bytes(a, b):
    assert a["result"] == b["result"]
    for k in INTS + ("objs",):
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- components -------------------------------------------------------------------------------------------------------------------------------
def test_snake(pkg, ctx):
    dev_build(pkg, ctx, "snake")
    dev, ref = check(pkg, ctx, "snake", 1, reach=1)
    assert dev["result"] == dict(status=0, n_voxels=1500, n_in_range=1500, n_gated=1500, n_kept=1500, n_components_all=1, n_components=1, n_ok=1)
    assert dev["comp"][0, :3].tolist() == [0, 1500, 1500] and (dev["voxel_comp"] == 0).all()
    e = scene("snake")["ext"]
    assert dev["comp"][0, 3:].tolist() == e["key"][0].tolist() and (e["key"][:, :2] < 0).any() and (e["key"][:, :2] > 0).any()


@pytest.mark.parametrize("reach", [1, 2, 3])
def test_reach_boundary(pkg, ctx, reach):
    for gap, want in ((reach, 1), (reach + 1, 2)):
        dev_build(pkg, ctx, f"gap{gap}")
        dev, _ = check(pkg, ctx, f"gap{gap}", 1, reach=reach, min_component=1, objs=False)
        assert dev["result"]["n_components_all"] == want == dev["result"]["n_components"], (reach, gap)
        assert dev["comp"][:, 1].tolist() == ([54] if want == 1 else [27, 27])


def test_two_labels_in_contact(pkg, ctx):
    dev_build(pkg, ctx, "slabs")
    dev, _ = check(pkg, ctx, "slabs", 2, reach=2, min_component=1)          # slabs of one label are two voxels apart: they join each other only
    assert dev["comp"][:, :3].tolist() == [[0, 96, 96], [1, 96, 96]]
    dev, _ = check(pkg, ctx, "slabs", 2, reach=1, min_component=1, objs=False)
    assert dev["comp"][:, :2].tolist() == [[0, 24]] * 4 + [[1, 24]] * 4
    dev, _ = check(pkg, ctx, "slabs", 2, reach=3, min_component=1)
    assert dev["result"]["n_components_all"] == 2


def test_size_tie_takes_the_lower_key(pkg, ctx):
    dev_build(pkg, ctx, "tie")
    dev, _ = check(pkg, ctx, "tie", 2, min_component=30)
    assert dev["comp"].tolist() == [[0, 30, 30, -9, 4, 2], [0, 30, 30, 6, 0, 2], [1, 36, 36, 0, 20, 2]]
    assert dev["stats"].tolist() == [[0, 60, 2, 0, 30, 30], [0, 36, 1, 2, 36, 36]]
    assert np.abs(dev["objs"][0, :3] - [(-9 + 2.5) * LEAF, (4 + 1.5) * LEAF, 3 * LEAF]).max() < 1e-9


def test_gates(pkg, ctx):
    dev_build(pkg, ctx, "gates")
    T = 2 * 60 + 12 + 4
    assert scene("gates")["ext"]["n_voxels"] == T
    dev, _ = check(pkg, ctx, "gates", 2, min_votes=3, min_component=10)
    assert dev["result"] == dict(status=0, n_voxels=T, n_in_range=T - 2, n_gated=T - 4, n_kept=T - 4 - 36, n_components_all=2, n_components=2, n_ok=1)
    assert dev["comp"][:, :3].tolist() == [[0, 48, 144], [0, 48, 144]] and dev["stats"][1].tolist() == [1, 0, 0, -1, 0, 0]
    dev, _ = check(pkg, ctx, "gates", 2, min_count=2, plane_dist=0.0, min_component=10)          # the bridge stays: one component, with the 2 : 1 voxel
    assert dev["result"]["n_gated"] == T - 3 == dev["result"]["n_kept"] and dev["comp"][:, :3].tolist() == [[0, T - 3, 3 * (T - 3)]]
    dev, _ = check(pkg, ctx, "gates", 2, plane_dist=0.0, min_component=10)          # nothing gated but the labels
    assert dev["result"]["n_kept"] == T - 2 and dev["comp"][0, 2] == 3 * (T - 3) + 1
    dev, _ = check(pkg, ctx, "gates", 6, min_component=1, objs=False)          # label 5 is an object now; 1 .. 4 have no voxel
    assert dev["stats"][:, 0].tolist() == [0, 1, 1, 1, 1, 0] and dev["result"]["n_in_range"] == T - 1
    dev, _ = check(pkg, ctx, "gates", 2, plane_dist=0.3, min_component=10)          # everything below: statuses 1
    assert dev["result"]["n_kept"] == 0 and dev["stats"][:, 0].tolist() == [1, 1] and (dev["voxel_comp"] == -1).all()


# ---- ellipsoids -------------------------------------------------------------------------------------------------------------------------------
def test_yawed_box_on_a_tilted_plane(pkg, ctx):
    dev_build(pkg, ctx, "box")
    dev, ref = check(pkg, ctx, "box", 2, TILTED)
    c0 = box_scene()[1]
    o = dev["objs"][1]
    assert dev["stats"][:, 0].tolist() == [1, 0] and 450 < dev["stats"][1, 4] <= 12 * 8 * 6 + 150
    assert np.abs(o[:3] - c0).max() < 0.03 and np.abs(o[7:] - [0.3, 0.2, 0.15]).max() < 0.06          # the box itself, to a voxel
    n, _, u, v = dor.plane(TILTED)
    R = dr.pose([0, 0, 0, *o[3:7]])[0]
    assert np.abs(R[:, 2] - n).max() < 1e-9 and abs(np.arctan2(R[:, 0] @ np.array(v), R[:, 0] @ np.array(u)) - 0.4) < 0.05
    assert ref["margins"]["anisotropy"][1] > 0.2


def test_axis_aligned_block(pkg, ctx):
    dev_build(pkg, ctx, "block")
    dev, _ = check(pkg, ctx, "block", 1, plane_dist=0.0)
    assert np.abs(dev["objs"][0] - [0.30, 0.20, 0.15, 0, 0, 0, 1, 0.30, 0.20, 0.15]).max() <= 1e-9
    dev, _ = check(pkg, ctx, "block", 1, (0.0, 0.0, 3.0, 0.0), plane_dist=0.0)          # a normal of length 3
    assert np.abs(dev["objs"][0] - [0.30, 0.20, 0.15, 0, 0, 0, 1, 0.30, 0.20, 0.15]).max() <= 1e-9


ROOM_GROUND = (0.0, -1.0, 0.0, 0.6)          # the image's y axis points down: the floor 0.6 m below the cameras


def test_room(pkg, ctx):
    dev_build(pkg, ctx, "room")
    dev, ref = check(pkg, ctx, "room", 13, ROOM_GROUND, min_component=20, objs=False)
    assert dev["result"]["n_ok"] >= 4 and dev["result"]["n_components_all"] > dev["result"]["n_components"] >= 4
    assert (dev["voxel_comp"] == -1).any() and (dev["voxel_comp"] >= 0).any()
    ok = [o for o, a in ref["margins"]["anisotropy"].items() if a >= MIN_ANISOTROPY]
    assert len(ok) >= 3
    assert np.abs(dev["objs"][ok] - ref["objs"][ok]).max() <= OBJ_TOL
    assert (dev["objs"][dev["stats"][:, 0] != 0] == 0).all()
    check(pkg, ctx, "room", 3, ROOM_GROUND, reach=1, min_component=5, min_votes=2, objs=False)
    check(pkg, ctx, "room", 13, ROOM_GROUND, reach=3, min_component=50, min_count=2, plane_dist=0.4, objs=False)


# ---- invariance ---------------------------------------------------------------------------------------------------------------------------------
def test_runs_and_frame_orders_give_the_same_bytes(pkg, ctx):
    s = scene("room")["frames"]
    P = pkg.abi.default_dense_obj_params(min_component=20)
    dev_build(pkg, ctx, "room")
    a = ctx.dense_objects(13, ROOM_GROUND, P)
    same_bytes(a, ctx.dense_objects(13, ROOM_GROUND, P))
    ext = ctx.dense_extract()          # an extract between two object calls changes nothing
    same_bytes(a, ctx.dense_objects(13, ROOM_GROUND, P))
    assert ext["inst"].tobytes() == ctx.dense_extract()["inst"].tobytes() == scene("room")["ext"]["inst"].tobytes()
    cx = pkg.Context(0)
    try:
        cx.dense_begin(pkg.abi.default_dense_params(leaf=LEAF, max_voxels=MAXV))
        dev_add(cx, s, [2])
        part = cx.dense_objects(13, ROOM_GROUND, P)          # add -> objects -> add -> objects
        m1, _ = sc.reference(s, [[2]], leaf=LEAF, max_voxels=MAXV)
        assert_same(part, dor.objects(m1.extract(), LEAF, 13, ROOM_GROUND, min_component=20), objs=False)
        dev_add(cx, s, [1, 0])
        same_bytes(a, cx.dense_objects(13, ROOM_GROUND, P))
    finally:
        cx.close()
    f = scene("box")["frames"]
    dev_build(pkg, ctx, "box")
    b = ctx.dense_objects(2, TILTED)
    ctx.dense_begin(pkg.abi.default_dense_params(leaf=LEAF, max_voxels=MAXV))
    dev_add(ctx, f, np.arange(len(f["cams"]))[::-1])
    same_bytes(b, ctx.dense_objects(2, TILTED))


# ---- capacity, statuses, caps ---------------------------------------------------------------------------------------------------------------
def raw(pkg, cx, N=2, ground=FLOOR, params=None, objs="own", stats="own", comp_cap=4, comp="own", voxel_cap=8, vox="own", out=True, ctx_h=True,
        fill=77):
    """the C-ABI itself, every argument free: 'own' = a buffer of the stated size filled with `fill`, None = NULL"""
    L = pkg.lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    own = lambda a, shape, dt: np.full(shape, fill, dt) if isinstance(a, str) else a          # noqa: E731
    buf = dict(objs=own(objs, (max(N, 1), 10), np.float64), stats=own(stats, (max(N, 1), 6), np.int32),
               comp=own(comp, (max(comp_cap, 1), 6), np.int32), vox=own(vox, max(voxel_cap, 1), np.int32))
    g = None if ground is None else np.ascontiguousarray(ground, dtype=np.float64)
    res = pkg.abi.EslDenseObjResult()
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)          # noqa: E731
    rc = L.esl_dense_objects(cx._h if ctx_h else None, N, ptr(g, dp), None if params is None else ctypes.byref(params), ptr(buf["objs"], dp),
                             ptr(buf["stats"], ip), comp_cap, ptr(buf["comp"], ip), voxel_cap, ptr(buf["vox"], ip), ctypes.byref(res) if out else None)
    return rc, res.as_dict(), buf, L.esl_last_error().decode()


def test_capacity_statuses_and_caps(pkg, ctx):
    P = pkg.abi.default_dense_obj_params
    dev_build(pkg, ctx, "tie")
    dev, _ = check(pkg, ctx, "tie", 2, min_component=30, max_components=2, objs=False)          # three qualifying components
    assert dev["result"]["status"] == 3 and dev["result"]["n_components"] == 3 and dev["result"]["n_ok"] == 0
    assert not dev["objs"].any() and not dev["stats"].any() and not dev["comp"].any() and (dev["voxel_comp"] == -1).all()
    check(pkg, ctx, "tie", 2, min_component=30, max_components=3)
    check(pkg, ctx, "tie", 2, min_component=31, max_components=1)          # only label 1's component qualifies: label 0 has status 2
    dev, _ = check(pkg, ctx, "tie", 3, min_component=31)
    assert dev["stats"][:, 0].tolist() == [2, 0, 1] and dev["stats"][0].tolist() == [2, 60, 0, -1, 0, 0]
    # caps smaller than the counts: the rows past them stay as they were
    full = ctx.dense_objects(2, FLOOR, P(min_component=30))
    rc, res, buf, _ = raw(pkg, ctx, params=P(min_component=30), comp_cap=2, voxel_cap=50)
    assert rc == 0 and res == full["result"]
    assert np.array_equal(buf["comp"], full["comp"][:2]) and np.array_equal(buf["vox"], full["voxel_comp"][:50])
    rc, res, buf, _ = raw(pkg, ctx, params=P(min_component=30), comp_cap=0, comp=np.full((3, 6), 77, np.int32), voxel_cap=0, vox=np.full(5, 77, np.int32))
    assert rc == 0 and (buf["comp"] == 77).all() and (buf["vox"] == 77).all() and buf["objs"].tobytes() == full["objs"].tobytes()
    check(pkg, ctx, "tie", 2, min_component=30, comp_cap=1, voxel_cap=7)
    rc, res, buf, _ = raw(pkg, ctx, params=None, stats=None, comp_cap=0, comp=None, voxel_cap=0, vox=None)          # NULL = defaults; the optional outputs
    assert rc == 0 and res["n_components"] == 0 and res["n_components_all"] == 3
    # N = 0: no label is an object
    dev, _ = check(pkg, ctx, "tie", 0, min_component=30)
    assert dev["result"]["n_in_range"] == 0 and dev["result"]["n_voxels"] == 96 and dev["objs"].shape == (0, 10)
    rc, res, _, _ = raw(pkg, ctx, N=0, objs=None, stats=None)
    assert rc == 0 and res["n_kept"] == 0
    # an empty map
    ctx.dense_begin(pkg.abi.default_dense_params(leaf=LEAF, max_voxels=MAXV))
    dev = ctx.dense_objects(2, FLOOR)
    assert dev["result"] == dict(dict.fromkeys(dor.RESULT, 0)) and dev["stats"].tolist() == [[1, 0, 0, -1, 0, 0]] * 2 and not dev["objs"].any()
    assert len(dev["comp"]) == 0 and len(dev["voxel_comp"]) == 0
    assert_same(dev, dor.objects(dr.DenseMap(leaf=LEAF).extract(), LEAF, 2, FLOOR))
    # a map over its own capacity: a result, nothing is written
    dev_build(pkg, ctx, "tie", max_voxels=95)
    assert ctx.dense_info()["status"] == 3
    rc, res, buf, _ = raw(pkg, ctx)
    assert rc == 0 and res == dict(dict.fromkeys(dor.RESULT, 0), status=3, n_voxels=-1)
    assert all((b == 77).all() for b in buf.values())
    dev = ctx.dense_objects(2, FLOOR)
    assert dev["result"]["n_voxels"] == -1 and len(dev["objs"]) == 0


def test_errors(pkg):
    P = pkg.abi.default_dense_obj_params
    nan, inf = float("nan"), float("inf")
    cx = pkg.Context(0)
    try:
        rc, _, _, msg = raw(pkg, cx)
        assert rc == 4 and "esl_dense_objects: no esl_dense_begin" in msg
        cx.dense_begin(pkg.abi.default_dense_params(leaf=LEAF, max_voxels=MAXV), True, False)
        rc, _, _, msg = raw(pkg, cx)
        assert rc == 4 and "without labels" in msg
        cx.dense_begin(pkg.abi.default_dense_params(leaf=LEAF, max_voxels=MAXV))
        dev_add(cx, scene("tie")["frames"])
        before = cx.dense_objects(2, FLOOR, P(min_component=30))
        cases = [(dict(ctx_h=False), "ctx"), (dict(ground=None), "ground_world"), (dict(out=False), "out"), (dict(N=-1), "N"),
                 (dict(comp_cap=-1), "comp_cap"), (dict(voxel_cap=-1), "voxel_cap"), (dict(objs=None), "objs_out"), (dict(comp=None), "comp_out"),
                 (dict(vox=None), "voxel_comp_out"), (dict(ground=(0, nan, 1, 0)), "ground_world"), (dict(ground=(0, 0, 1, inf)), "ground_world"),
                 (dict(ground=(0, 0, 1e-13, 0)), "ground_world"), (dict(ground=(0, 0, 0, 0)), "ground_world"),
                 (dict(params=P(reach=0)), "reach"), (dict(params=P(reach=4)), "reach"), (dict(params=P(min_votes=0)), "min_votes"),
                 (dict(params=P(min_count=0)), "min_count"), (dict(params=P(min_component=0)), "min_component"),
                 (dict(params=P(max_components=0)), "max_components"), (dict(params=P(max_components=(1 << 20) + 1)), "max_components"),
                 (dict(params=P(plane_dist=nan)), "plane_dist"), (dict(params=P(plane_dist=-inf)), "plane_dist")]
        for over, word in cases:
            rc, _, buf, msg = raw(pkg, cx, **over)
            assert rc == 2 and msg.startswith("esl_dense_objects: ") and word in msg, (over, msg)
            assert all(b is None or (b == 77).all() for b in buf.values())
        with pytest.raises(pkg.EslError, match="esl_status 2: esl_dense_objects: .*reach"):
            cx.dense_objects(2, FLOOR, P(reach=7))
        # every refused call left the map and the call as they were; the limits themselves are valid
        same_bytes(before, cx.dense_objects(2, FLOOR, P(min_component=30)))
        assert raw(pkg, cx, params=P(max_components=1 << 20, reach=3, plane_dist=-5.0))[0] == 0
        cx.dense_end()
        assert raw(pkg, cx)[0] == 4
    finally:
        cx.close()


# ---- buffers and profile ----------------------------------------------------------------------------------------------------------------------
def test_warm_call_allocates_nothing(pkg):
    cx = pkg.Context(0)
    try:
        P = pkg.abi.default_dense_obj_params(min_component=20)
        assert cx.dense_allocs() == (0, 0)
        dev_build(pkg, cx, "tie")          # many small frames: the largest pose buffer
        cx.dense_objects(2, FLOOR, P)
        dev_build(pkg, cx, "room")          # few large frames: the largest images and the most voxels
        a = cx.dense_objects(13, ROOM_GROUND, P)
        allocs = cx.dense_allocs()
        assert allocs[0] > 0 and allocs[1] > 0
        same_bytes(a, cx.dense_objects(13, ROOM_GROUND, P))
        cx.dense_objects(5, ROOM_GROUND, pkg.abi.default_dense_obj_params(min_component=50, reach=3), comp_cap=1, voxel_cap=10)          # no larger
        assert cx.dense_allocs() == allocs
        dev_build(pkg, cx, "tie")          # a smaller map after a larger one reads nothing the larger one left behind
        check(pkg, cx, "tie", 2, min_component=30)
        dev_build(pkg, cx, "room")
        same_bytes(a, cx.dense_objects(13, ROOM_GROUND, P))
        assert cx.dense_allocs() == allocs
        for owner in cx.SCRATCH_OWNERS:
            assert cx.scratch_allocs(owner) == (0, 0), owner
    finally:
        cx.close()


def test_profile_class_4(pkg):
    cx = pkg.Context(0)
    try:
        dev_build(pkg, cx, "tie")
        cx.profile_enable(2)
        cx.dense_objects(2, FLOOR, pkg.abi.default_dense_obj_params(min_component=30))
        prof = cx.profile_get()
        assert set(prof) == {"reduce"} and prof["reduce"]["count"] >= 3 and prof["reduce"]["total_ms"] > 0
    finally:
        cx.close()
