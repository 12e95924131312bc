"""esl_dense_planes on the device against its numpy statement (tests/dense_planes_ref.py).

Voxel sets are placed exactly through esl_dense_add_frames: one 1 x 1 frame per sample at a voxel's centre (dense_objects_ref.voxel_frames),
frames shuffled (tests/dense_planes_scenes.py; the conditions the scenes rely on are asserted on the statement alone in
tests/test_dense_planes_ref.py).  Every integer output is compared exactly, hyp -- every hypothesis of every round -- included.  planes,
centroid and ground are compared at 1e-9 absolute, the tolerance of esl_dense_objects' ellipsoids: both sides start from identical
integers and run identical IEEE operations (+ - * / sqrt are correctly rounded everywhere), so they agree far below that; the integer
outputs would show a different decision first."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as dr                # noqa: E402
import dense_objects_ref as dor       # noqa: E402
import dense_planes_ref as dpr        # noqa: E402
import dense_planes_scenes as ps      # noqa: E402
import dense_scenes as sc             # noqa: E402

pytestmark = pytest.mark.gpu

LEAF = ps.LEAF
MAXV = ps.MAXV
TOL = 1e-9
INTS = ("stats", "samples", "voxel_plane", "hyp")
FLOATS = ("planes", "centroid", "ground")
LATTICE = dict(dist_tol=0.004, n_hypotheses=128, min_inliers=50, min_baseline=4)


def dev_add(cx, s, idx=None, inst=True):
    idx = slice(None) if idx is None else idx
    return cx.dense_add_frames(s["cams"][idx], s["K"], s["rows"], s["cols"], s["depth"][idx], s["bgr"][idx], s["inst"][idx] if inst else None)


def dev_build(pkg, cx, name, **over):
    s = ps.scene(name)
    over.setdefault("leaf", s["leaf"]); over.setdefault("max_voxels", MAXV)
    cx.dense_begin(pkg.abi.default_dense_params(**over), True, s["with_inst"])
    dev_add(cx, s["frames"], inst=s["with_inst"])


def assert_same(dev, ref):
    assert dev["result"] == ref["result"]
    for k in INTS:
        assert dev[k].dtype == ref[k].dtype and dev[k].shape == ref[k].shape, (k, dev[k].shape, ref[k].shape)
        if not np.array_equal(dev[k], ref[k]):
            bad = np.argwhere(dev[k] != ref[k])[:5]
            raise AssertionError((k, bad.tolist(), dev[k][tuple(bad[0])], ref[k][tuple(bad[0])]))
    for k in FLOATS:
        assert dev[k].shape == ref[k].shape, k
        err = np.abs(dev[k] - ref[k])
        print(f"max |{k} - statement| =", err.max() if err.size else 0.0)
        assert (err <= TOL).all(), (k, err.max())


def check(pkg, cx, name, voxel_cap=None, **kw):
    dev = cx.dense_planes(pkg.abi.default_dense_plane_params(**kw), voxel_cap=voxel_cap, hyp=True)
    s = ps.scene(name)
    ref = dpr.planes(s["ext"], s["leaf"], voxel_cap=voxel_cap, **kw)
    assert_same(dev, ref)
    return dev, ref


def same_bytes(a, b):
    assert a["result"] == b["result"]
    for k in INTS + FLOATS:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- the planted scene ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hyp", [256, 70])
@pytest.mark.parametrize("seed", [0, 3])
def test_planted_scene(pkg, ctx, seed, n_hyp):
    dev_build(pkg, ctx, "planted")
    dev, _ = check(pkg, ctx, "planted", n_hypotheses=n_hyp, seed=seed, **ps.PLANTED)
    assert dev["result"] == dict(status=0, n_voxels=3047, n_eligible=3047, n_planes=3, n_assigned=2904, ground_index=-1, rounds=4, stop_reason=3)
    assert dev["stats"][:, 0].tolist() == [1600, 901, 403]
    truth = ps.planted_truth(ps.scene("planted")["ext"]["key"].astype(np.int64))
    vp = dev["voxel_plane"]
    assert ((truth[truth != 0] >> vp[truth != 0]) & 1).all()
    s2 = np.sqrt(0.5)
    assert np.abs(dev["planes"] - np.array([[0, 0, -1, 0.005], [-s2, 0, -s2, 0.61 * s2], [0, -1, 0, 0.455]])).max() <= 1e-9


# ---- list lengths and hypothesis counts ---------------------------------------------------------------------------------------------------------
def test_short_lists(pkg, ctx):
    kw = dict(dist_tol=0.004, n_hypotheses=64, min_inliers=3, min_baseline=1)
    ctx.dense_begin(pkg.abi.default_dense_params(leaf=LEAF, max_voxels=MAXV))
    dev = ctx.dense_planes(pkg.abi.default_dense_plane_params(**kw), hyp=True)
    assert_same(dev, dpr.planes(dr.DenseMap(leaf=LEAF).extract(), LEAF, **kw))
    assert dev["result"] == dict(dict.fromkeys(dpr.RESULT, 0), ground_index=-1, stop_reason=1)
    for n in (1, 2):
        dev_build(pkg, ctx, f"few{n}")
        dev, _ = check(pkg, ctx, f"few{n}", **kw)
        assert dev["result"]["stop_reason"] == 1 and dev["result"]["rounds"] == 0 and (dev["voxel_plane"] == -2).all()
    dev_build(pkg, ctx, "line3")
    dev, _ = check(pkg, ctx, "line3", **kw)
    assert dev["result"]["stop_reason"] == 2 and dev["result"]["rounds"] == 1
    dev_build(pkg, ctx, "few3")
    dev, _ = check(pkg, ctx, "few3", **kw)
    assert dev["result"]["n_planes"] == 1 and dev["stats"][0, 0] == 3 and dev["result"]["stop_reason"] == 1
    dev_build(pkg, ctx, "few4")          # the fourth voxel is off the plane of the first three: eligible, unassigned
    dev, _ = check(pkg, ctx, "few4", **kw)
    assert sorted(dev["voxel_plane"].tolist()) == [-2, 0, 0, 0]
    dev, _ = check(pkg, ctx, "few4", min_count=2, **kw)          # nothing is eligible: n_0 = 0
    assert dev["result"]["n_eligible"] == 0 and (dev["voxel_plane"] == -1).all() and dev["result"]["stop_reason"] == 1


def list_lengths(pkg):
    tile, _ = pkg.Context.dense_planes_layout()
    return [63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1]


def test_list_lengths_around_the_wave_and_the_tile(pkg, ctx):
    for n in list_lengths(pkg):
        dev_build(pkg, ctx, f"len{n}")
        dev, _ = check(pkg, ctx, f"len{n}", dist_tol=0.004, n_hypotheses=96, min_inliers=20, min_baseline=4, max_planes=2)
        assert dev["stats"][0].tolist()[:2] == [n - 5, n] and dev["result"]["n_eligible"] == n, n


def test_hypothesis_counts_around_the_wave_and_the_group(pkg, ctx):
    _, group = pkg.Context.dense_planes_layout()
    dev_build(pkg, ctx, "planted")
    for n_hyp in (1, 63, 64, 65, group + 1):          # below 64 k_dpl_few scores them, lane = voxel; from 64 on k_dpl_score
        dev, _ = check(pkg, ctx, "planted", n_hypotheses=n_hyp, seed=5, max_planes=2, **ps.PLANTED)
        assert dev["hyp"].shape[1] == n_hyp
    assert dev["result"]["n_planes"] == 2


# ---- what decides ---------------------------------------------------------------------------------------------------------------------------------
def test_two_parallel_layers(pkg, ctx):
    dev_build(pkg, ctx, "layers")
    dev, _ = check(pkg, ctx, "layers", **dict(LATTICE, dist_tol=0.4 * LEAF))
    assert dev["stats"][:, 0].tolist() == [900, 900] and abs(dev["planes"][0, 3] - dev["planes"][1, 3]) == pytest.approx(LEAF, abs=1e-12)
    dev, _ = check(pkg, ctx, "layers", **dict(LATTICE, dist_tol=1.2 * LEAF))
    assert dev["stats"][:, 0].tolist() == [1800]


def test_ties(pkg, ctx):
    dev_build(pkg, ctx, "twins_samples")
    dev, _ = check(pkg, ctx, "twins_samples", **LATTICE)
    assert dev["samples"].tolist() == [800, 400] and dev["stats"][:, 0].tolist() == [400, 400]          # samples decide
    assert (dev["voxel_plane"][ps.scene("twins_samples")["ext"]["count"] == 2] == 0).all()
    dev_build(pkg, ctx, "twins")
    dev, _ = check(pkg, ctx, "twins", **LATTICE)
    full = np.flatnonzero(dev["hyp"][0][:, 1] == 400)
    assert len(full) > 2 and dev["stats"][0, 3] == full[0]          # equal voxels and samples: the smaller h


def test_gates(pkg, ctx):
    g = ps.scene("gates")["ext"]
    dev_build(pkg, ctx, "gates")
    dev, _ = check(pkg, ctx, "gates", **LATTICE)
    assert dev["result"]["n_eligible"] == g["n_voxels"]
    dev, _ = check(pkg, ctx, "gates", min_count=2, **LATTICE)
    assert dev["result"]["n_eligible"] == int((g["count"] >= 2).sum()) < g["n_voxels"] and (dev["voxel_plane"][g["count"] < 2] == -1).all()
    dev, _ = check(pkg, ctx, "gates", skip_labelled=1, **LATTICE)
    assert dev["result"]["n_eligible"] == g["n_voxels"] - 400 and (dev["voxel_plane"][g["votes"] > 0] == -1).all()
    assert ctx.dense_extract()["votes"].tobytes() == g["votes"].tobytes()          # the best words are rebuilt by whoever needs them
    dev_build(pkg, ctx, "gates_nolabels")
    dev, _ = check(pkg, ctx, "gates_nolabels", skip_labelled=1, **LATTICE)
    assert dev["result"]["n_eligible"] == g["n_voxels"] and dev["result"]["n_planes"] == 2


def test_refit_kept_and_rejected(pkg, ctx):
    kw = dict(dist_tol=1.5 * LEAF, n_hypotheses=128, min_inliers=100, max_planes=2)
    dev_build(pkg, ctx, "thick")
    d1, _ = check(pkg, ctx, "thick", **kw)
    d0, _ = check(pkg, ctx, "thick", refine=0, **kw)
    assert d1["stats"][0, 5] == 1 and d0["stats"][0, 5] == 0 and np.abs(d1["planes"][0] - d0["planes"][0]).max() > 1e-4
    dev_build(pkg, ctx, "rejected")
    dev, _ = check(pkg, ctx, "rejected", dist_tol=1.2 * LEAF, n_hypotheses=128, min_inliers=100, max_planes=1)
    assert dev["stats"][0].tolist()[4:6] == [1008, 2] and dev["stats"][0, 0] == 1008


# ---- the ground -------------------------------------------------------------------------------------------------------------------------------------
def test_ground_on_the_room_feeds_the_objects(pkg, ctx):
    """dense_scenes.room_scene holds one surface, a slanted wall, and no floor: with up = towards the cameras the wall is the ground
    that esl_dense_objects measures heights from; with the scene's own up there is none.  A real floor is found on slabs only
    (the planted scene's kz = 0 in the invariance test, the twins below)."""
    dev_build(pkg, ctx, "room")
    dev, ref = check(pkg, ctx, "room", **ps.ROOM)
    assert dev["result"]["ground_index"] == 0 and dev["ground"][2] < -0.9 and dev["stats"][0, 0] > 1000
    P = pkg.abi.default_dense_obj_params(min_component=20)
    a = ctx.dense_objects(13, dev["ground"], P)
    b = ctx.dense_objects(13, ref["ground"], P)
    assert a["result"] == b["result"] and a["result"]["n_ok"] >= 3
    for k in ("objs", "stats", "comp", "voxel_comp"):
        assert a[k].tobytes() == b[k].tobytes(), k
    # the room's own up, (0, -1, 0): it has no floor, the wall is no candidate
    dev, _ = check(pkg, ctx, "room", **dict(ps.ROOM, up=(0.0, -1.0, 0.0)))
    assert dev["result"]["ground_index"] == -1 and not dev["ground"].any() and dev["result"]["n_planes"] == 1
    # a floor above the origin: planes_out and ground_out differ in sign
    dev_build(pkg, ctx, "twins")
    dev, _ = check(pkg, ctx, "twins", up=(0.0, 0.0, 2.0), max_planes=1, **dict(LATTICE, seed=1))
    assert dev["result"]["ground_index"] == 0 and (dev["ground"] == -dev["planes"][0]).all() and dev["ground"][2] == 1.0
    dev, _ = check(pkg, ctx, "twins", up=(0.0, 1.0, 0.0), **LATTICE)
    assert dev["result"]["ground_index"] == -1 and not dev["ground"].any()


# ---- invariance and alternation -----------------------------------------------------------------------------------------------------------------
def test_orders_splits_and_runs_give_the_same_bytes(pkg, ctx):
    P = pkg.abi.default_dense_plane_params(n_hypotheses=70, seed=3, up=(0.0, 0.0, -1.0), **ps.PLANTED)
    f = ps.scene("planted")["frames"]
    dev_build(pkg, ctx, "planted")
    a = ctx.dense_planes(P, hyp=True)
    same_bytes(a, ctx.dense_planes(P, hyp=True))          # two runs
    F = len(f["cams"])
    cx = pkg.Context(0)
    try:
        cx.dense_begin(pkg.abi.default_dense_params(leaf=LEAF, max_voxels=MAXV))
        order = np.random.default_rng(5).permutation(F)          # another frame order, in three calls
        for part in (order[:F // 3], order[F // 3:F // 2], order[F // 2:]):
            dev_add(cx, f, part)
        same_bytes(a, cx.dense_planes(P, hyp=True))
    finally:
        cx.close()


def test_alternation_with_objects_and_extract(pkg, ctx):
    s = ps.scene("room")
    P = pkg.abi.default_dense_plane_params(**ps.ROOM)
    O = pkg.abi.default_dense_obj_params(min_component=20)
    ground = (0.0, -1.0, 0.0, 0.6)
    dev_build(pkg, ctx, "room")
    clean = ctx.dense_objects(13, ground, O)          # a map that never saw a plane call
    dev_build(pkg, ctx, "room")
    first = ctx.dense_planes(P, hyp=True)
    objs = ctx.dense_objects(13, ground, O)
    ext = ctx.dense_extract()
    last = ctx.dense_planes(P, hyp=True)
    same_bytes(first, last)
    assert objs["result"] == clean["result"]
    for k in ("objs", "stats", "comp", "voxel_comp"):
        assert objs[k].tobytes() == clean[k].tobytes(), k
    for k in ("key", "count", "inst", "votes"):
        assert ext[k].tobytes() == s["ext"][k].tobytes(), k
    skip = pkg.abi.default_dense_plane_params(skip_labelled=1, **ps.ROOM)          # the plane call that needs the votes, after one that does not
    ctx.dense_planes(P)
    assert_same(ctx.dense_planes(skip, hyp=True), dpr.planes(s["ext"], s["leaf"], skip_labelled=1, **ps.ROOM))


# ---- capacity, caps, errors -------------------------------------------------------------------------------------------------------------------------
def raw(pkg, cx, params=None, planes="own", cen="own", stats="own", smp="own", ground="own", voxel_cap=8, vox="own", hyp="own", out=True, ctx_h=True,
        fill=77, P=8, Hn=1024):
    """the C-ABI itself, every argument free: 'own' = a buffer of the stated size filled with `fill`, None = NULL"""
    L = pkg.lib.load()
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    own = lambda a, shape, dt: np.full(shape, fill, dt) if isinstance(a, str) else a          # noqa: E731
    buf = dict(planes=own(planes, (P, 4), np.float64), cen=own(cen, (P, 3), np.float64), stats=own(stats, (P, 8), np.int32), smp=own(smp, P, np.int64),
               ground=own(ground, 4, np.float64), vox=own(vox, max(voxel_cap, 1), np.int32), hyp=own(hyp, (P, Hn, 3), np.int64))
    res = pkg.abi.EslDensePlaneResult()
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)          # noqa: E731
    rc = L.esl_dense_planes(cx._h if ctx_h else None, None if params is None else ctypes.byref(params), ptr(buf["planes"], dp), ptr(buf["cen"], dp),
                            ptr(buf["stats"], ip), ptr(buf["smp"], lp), ptr(buf["ground"], dp), voxel_cap, ptr(buf["vox"], ip), ptr(buf["hyp"], lp),
                            ctypes.byref(res) if out else None)
    return rc, res.as_dict(), buf, L.esl_last_error().decode()


def test_capacity_and_caps(pkg, ctx):
    Pm = pkg.abi.default_dense_plane_params
    dev_build(pkg, ctx, "twins")
    kw = dict(LATTICE, max_planes=3, n_hypotheses=96)
    full, _ = check(pkg, ctx, "twins", **kw)
    check(pkg, ctx, "twins", voxel_cap=7, **kw)
    check(pkg, ctx, "twins", voxel_cap=0, **kw)
    # a cap smaller than the map: the rows past it stay as they were; the optional outputs may be NULL
    rc, res, buf, _ = raw(pkg, ctx, params=Pm(**kw), voxel_cap=50, vox=np.full(60, 77, np.int32), P=3, Hn=96)
    assert rc == 0 and res == full["result"] and np.array_equal(buf["vox"][:50], full["voxel_plane"][:50]) and (buf["vox"][50:] == 77).all()
    assert buf["planes"][:2].tobytes() == full["planes"].tobytes() and not buf["planes"][2].any() and not buf["stats"][2].any()
    assert np.array_equal(buf["hyp"][:res["rounds"]], full["hyp"]) and not buf["hyp"][res["rounds"]:].any() and not buf["ground"].any()
    rc, res, buf, _ = raw(pkg, ctx, params=Pm(**kw), cen=None, stats=None, smp=None, ground=None, voxel_cap=0, vox=None, hyp=None, P=3)
    assert rc == 0 and res == full["result"] and buf["planes"][:2].tobytes() == full["planes"].tobytes()
    # a map over its capacity: a result, nothing is written
    dev_build(pkg, ctx, "twins", max_voxels=799)
    assert ctx.dense_info()["status"] == 3
    rc, res, buf, _ = raw(pkg, ctx, params=Pm(**kw), P=3, Hn=96)
    assert rc == 0 and res == dict(dict.fromkeys(dpr.RESULT, 0), status=3, n_voxels=-1)
    assert all((b == 77).all() for b in buf.values())
    dev = ctx.dense_planes(Pm(**kw), hyp=True)
    assert dev["result"]["n_voxels"] == -1 and len(dev["planes"]) == 0 and len(dev["voxel_plane"]) == 0
    assert dpr.planes(dict(n_voxels=-1), LEAF, **kw)["result"] == dev["result"]


def test_errors(pkg):
    Pm = pkg.abi.default_dense_plane_params
    nan, inf = float("nan"), float("inf")
    cx = pkg.Context(0)
    try:
        rc, _, _, msg = raw(pkg, cx)
        assert rc == 4 and "esl_dense_planes: no esl_dense_begin" in msg
        dev_build(pkg, cx, "twins")
        small = dict(LATTICE, max_planes=2)
        before = cx.dense_planes(Pm(**small), hyp=True)
        cases = [(dict(ctx_h=False), "ctx"), (dict(out=False), "out"), (dict(planes=None), "planes_out"), (dict(voxel_cap=-1), "voxel_cap"),
                 (dict(vox=None), "voxel_plane_out"), (dict(params=Pm(dist_tol=0.0)), "dist_tol"), (dict(params=Pm(dist_tol=-1.0)), "dist_tol"),
                 (dict(params=Pm(dist_tol=nan)), "dist_tol"), (dict(params=Pm(dist_tol=inf)), "dist_tol"), (dict(params=Pm(up=(0, nan, 1))), "up"),
                 (dict(params=Pm(up=(inf, 0, 0))), "up"), (dict(params=Pm(up=(0, 1e-13, 0))), "up"), (dict(params=Pm(up_min_cos=-0.1)), "up_min_cos"),
                 (dict(params=Pm(up_min_cos=1.5)), "up_min_cos"), (dict(params=Pm(up_min_cos=nan)), "up_min_cos"),
                 (dict(params=Pm(n_hypotheses=0)), "n_hypotheses"), (dict(params=Pm(n_hypotheses=65537)), "n_hypotheses"),
                 (dict(params=Pm(max_planes=0)), "max_planes"), (dict(params=Pm(max_planes=65)), "max_planes"),
                 (dict(params=Pm(min_inliers=2)), "min_inliers"), (dict(params=Pm(min_baseline=0)), "min_baseline")]
        for over, word in cases:
            rc, _, buf, msg = raw(pkg, cx, **over)
            assert rc == 2 and msg.startswith("esl_dense_planes: ") and word in msg, (over, msg)
            assert all(b is None or (b == 77).all() for b in buf.values())
        with pytest.raises(pkg.EslError, match="esl_status 2: esl_dense_planes: .*max_planes"):
            cx.dense_planes(Pm(max_planes=100))
        # every refused call left the map and the call as they were; the limits themselves are valid
        same_bytes(before, cx.dense_planes(Pm(**small), hyp=True))
        lim = Pm(n_hypotheses=65536, max_planes=64, min_inliers=3, min_baseline=1, up=(0, 1e-11, 0), up_min_cos=1.0, dist_tol=1e-300)
        assert raw(pkg, cx, params=lim, P=64, Hn=65536)[0] == 0
        cx.dense_end()
        assert raw(pkg, cx)[0] == 4
    finally:
        cx.close()


# ---- buffers and profile ----------------------------------------------------------------------------------------------------------------------
def test_warm_call_allocates_nothing(pkg):
    cx = pkg.Context(0)
    try:
        Pm = pkg.abi.default_dense_plane_params
        assert cx.dense_allocs() == (0, 0)
        dev_build(pkg, cx, "planted")          # the most voxels and frames
        a = cx.dense_planes(Pm(n_hypotheses=256, **ps.PLANTED), hyp=True)
        allocs = cx.dense_allocs()
        assert allocs[0] > 0 and allocs[1] > 0
        same_bytes(a, cx.dense_planes(Pm(n_hypotheses=256, **ps.PLANTED), hyp=True))
        cx.dense_planes(Pm(n_hypotheses=70, max_planes=2, refine=0, **ps.PLANTED), voxel_cap=10)          # no larger
        assert cx.dense_allocs() == allocs
        dev_build(pkg, cx, "twins")          # a smaller map after a larger one reads nothing the larger one left behind
        check(pkg, cx, "twins", **LATTICE)
        dev_build(pkg, cx, "planted")
        same_bytes(a, cx.dense_planes(Pm(n_hypotheses=256, **ps.PLANTED), hyp=True))
        assert cx.dense_allocs() == allocs
        for owner in cx.SCRATCH_OWNERS:
            assert cx.scratch_allocs(owner) == (0, 0), owner
    finally:
        cx.close()


def test_profile_class_4(pkg):
    cx = pkg.Context(0)
    try:
        dev_build(pkg, cx, "twins")
        cx.profile_enable(2)
        cx.dense_planes(pkg.abi.default_dense_plane_params(**LATTICE))
        prof = cx.profile_get()
        assert set(prof) == {"reduce"} and prof["reduce"]["count"] >= 3 and prof["reduce"]["total_ms"] > 0
    finally:
        cx.close()
