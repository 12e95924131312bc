"""esl_dense_normals and esl_dense_align_frames on the device against their numpy statement (tests/dense_align_ref.py).

The maps are built through esl_dense_add_frames (tests/dense_align_scenes.py; the premises the scenes rely on are asserted on the
statement alone in tests/test_dense_align_ref.py).  Every output is compared byte for byte (a NaN curvature with a NaN): both sides run
identical correctly rounded operations in the same order, and every sum over samples is an integer sum."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_align_ref as dar          # noqa: E402
import dense_align_scenes as s         # noqa: E402

pytestmark = pytest.mark.gpu

ALIGN_OUTS = ("cams", "status", "iters", "counts", "sum_e2", "H", "step", "sums")
NORMAL_OUTS = ("normal", "curvature", "neighbors", "valid")


def dev_build(pkg, cx, name):
    sc = s.scene(name)
    cx.dense_begin(pkg.abi.default_dense_params(**sc["params"]), False, False)
    fr = sc["frames"]
    cx.dense_add_frames(fr["cams"], fr["K"], fr["rows"], fr["cols"], fr["depth"])
    for f in sc["remove"] or []:
        cx.dense_remove_frames(fr["cams"][f:f + 1], fr["K"], fr["rows"], fr["cols"], fr["depth"][f:f + 1])


@pytest.fixture(scope="module")
def refs():
    """the statement's result of every case, computed once and left unchanged"""
    cache = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in cache:
            c = s.case(name)
            sc = s.scene(c["map"])
            cache[key] = dar.align(s.extract(c["map"]), sc["params"]["leaf"], sc["params"], c["cams"], c["K"], c["rows"], c["cols"], c["depth"],
                                   **dict(c["params"], **kw))
        return cache[key]
    return get


def dev_of(pkg, cx, name, frames=None, **kw):
    c = s.case(name)
    f = slice(None) if frames is None else frames
    return cx.dense_align_frames(c["cams"][f], c["K"], c["rows"], c["cols"], c["depth"][f], pkg.abi.default_dense_align_params(**dict(c["params"], **kw)))


def same_bytes(a, b, outs=ALIGN_OUTS):
    for k in outs:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (k, a[k].dtype, b[k].dtype, a[k].shape, b[k].shape)
        if a[k].tobytes() != b[k].tobytes():
            bad = np.argwhere(~((a[k] == b[k]) | ((a[k] != a[k]) & (b[k] != b[k]))))[:5]
            raise AssertionError((k, bad.tolist(), a[k][tuple(bad[0])] if len(bad) else None, b[k][tuple(bad[0])] if len(bad) else None))


def assert_same(dev, ref):
    assert dev["result"] == ref["result"]
    same_bytes(dev, ref)


def snapshot(cx):
    e = cx.dense_extract()
    return [cx.dense_info(), cx.dense_slots()] + [e[k].tobytes() if k != "n_voxels" else e[k] for k in sorted(e)]


# ---- the normals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plane", "tilted", "edge", "corner", "room", "removed"])
def test_normals(pkg, ctx, name):
    dev_build(pkg, ctx, name)
    for over in (dict(), dict(radius=2, min_neighbors=12), dict(min_count=2), dict(max_curvature=0.0)):
        ref = dar.normals(s.extract(name), **over)
        dev = ctx.dense_normals(pkg.abi.default_dense_normal_params(**over))
        assert dev["result"] == ref["result"], over
        same_bytes(dev, ref, NORMAL_OUTS)
    if name == "plane":
        e = ctx.dense_extract()
        i = [list(k) for k in e["key"].tolist()].index([4, 4, 3])
        d = ctx.dense_normals()
        assert d["normal"][i].tolist() == [0.0, 0.0, 1.0] and d["curvature"][i] == 0.0 and d["neighbors"][i] == 9 and d["valid"][i] == 1
        cap = ctx.dense_normals(cap=10)
        assert len(cap["normal"]) == 10 and cap["result"] == d["result"] and cap["normal"].tobytes() == d["normal"][:10].tobytes()
        assert ctx.dense_normals(cap=0)["result"] == d["result"]


def test_normals_leave_the_map_alone_and_allocate_once(pkg, ctx):
    dev_build(pkg, ctx, "room")
    before = snapshot(ctx)
    a = ctx.dense_normals()
    warm = ctx.dense_allocs()
    b = ctx.dense_normals()
    assert ctx.dense_allocs() == warm and a["result"] == b["result"]
    same_bytes(a, b, NORMAL_OUTS)
    assert snapshot(ctx) == before


# ---- the aligner: shapes, reach, radius --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corner", "corner_s1", "small", "small_odd", "reach0", "reach2", "radius2", "far"])
def test_cases(pkg, ctx, refs, name):
    dev_build(pkg, ctx, "room")
    dev = dev_of(pkg, ctx, name)
    assert_same(dev, refs(name))
    assert dev["status"].tolist() == [dar.CONVERGED]
    if name == "far":
        assert (dev["sums"][0, 0, 34:37] > 0).all()


def test_mixed_frames_batching_order_and_repeat(pkg, ctx, refs):
    dev_build(pkg, ctx, "room")
    before = snapshot(ctx)
    a0 = ctx.dense_allocs()
    dev = dev_of(pkg, ctx, "mixed")
    assert_same(dev, refs("mixed"))
    assert dev["status"].tolist() == [dar.CONVERGED, dar.DEGENERATE, dar.TOO_FEW]
    warm = ctx.dense_allocs()
    assert warm[0] > a0[0]
    again = dev_of(pkg, ctx, "mixed")          # a warm call of the same shape: the same bytes, no allocation
    assert ctx.dense_allocs() == warm and again["result"] == dev["result"]
    same_bytes(again, dev)
    assert snapshot(ctx) == before          # the call does not change the map
    # the good frame alone: its rows do not change
    alone = dev_of(pkg, ctx, "corner")
    assert_same(alone, refs("corner"))
    for k in ALIGN_OUTS:
        assert alone[k].tobytes() == dev[k][:1].tobytes(), k
    # F calls of one frame = one call of F; any frame order gives the same rows
    parts = [dev_of(pkg, ctx, "mixed", frames=slice(f, f + 1)) for f in range(3)]
    for k in ALIGN_OUTS:
        assert np.concatenate([p[k] for p in parts]).tobytes() == dev[k].tobytes(), k
    order = [2, 0, 1]
    perm = dev_of(pkg, ctx, "mixed", frames=order)
    for k in ALIGN_OUTS:
        assert perm[k].tobytes() == dev[k][order].tobytes(), k
    # iters = 0 only evaluates; without the per-pass rows the rest is the same
    ev = dev_of(pkg, ctx, "mixed", iters=0)
    assert_same(ev, refs("mixed", iters=0))
    assert ev["cams"].tobytes() == s.case("mixed")["cams"].tobytes() and ev["result"]["n_passes"] == 1
    c = s.case("mixed")
    bare = ctx.dense_align_frames(c["cams"], c["K"], c["rows"], c["cols"], c["depth"], iters_out=False)
    assert "sums" not in bare
    same_bytes(bare, dev, ALIGN_OUTS[:-1])
    none = ctx.dense_align_frames(np.zeros((0, 7)), c["K"], c["rows"], c["cols"], np.zeros((0, c["rows"], c["cols"]), np.uint16))          # F = 0
    assert none["result"] == dict(dev["result"], n_passes=0) and none["cams"].shape == (0, 7)


def test_after_remove_and_purge(pkg, ctx, refs):
    dev_build(pkg, ctx, "removed")
    assert ctx.dense_slots()["dead_voxels"] > 0
    ref = refs("removed")
    a = dev_of(pkg, ctx, "removed")
    assert_same(a, ref)
    n_a = ctx.dense_normals()
    ctx.dense_purge()
    assert ctx.dense_slots()["dead_voxels"] == 0
    b = dev_of(pkg, ctx, "removed")
    assert_same(b, ref)
    same_bytes(ctx.dense_normals(), n_a, NORMAL_OUTS)
    dev_build(pkg, ctx, "without")          # the map built from scratch without that frame
    w = dev_of(pkg, ctx, "without")
    assert w["result"] == a["result"]
    same_bytes(w, a)


# ---- an invalid map -----------------------------------------------------------------------------------------------------------------------
def raw_align(pkg, cx, cams, F, K, rows, cols, depth, p=None, out=True, bufs=None):
    """esl_dense_align_frames through ctypes alone -> (rc, result)"""
    L = pkg.lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    bufs = bufs or {}
    cams = None if cams is None else np.ascontiguousarray(cams, dtype=np.float64)
    Kc = None if K is None else np.ascontiguousarray(K, dtype=np.float64)
    depth = None if depth is None else np.ascontiguousarray(depth, dtype=np.uint16)
    res = pkg.abi.EslDenseAlignResult(7, 7, 7, 7)
    rc = L.esl_dense_align_frames(cx._h if cx is not None else None, None if cams is None else cams.ctypes.data_as(dp), F,
                                  None if Kc is None else Kc.ctypes.data_as(dp), rows, cols,
                                  None if depth is None else depth.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                                  None if p is None else ctypes.byref(p), bufs["cams"].ctypes.data_as(dp) if "cams" in bufs else None,
                                  bufs.get("frames"), bufs["sums"].ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if "sums" in bufs else None,
                                  ctypes.byref(res) if out else None)
    return rc, res.as_dict()


def test_invalid_maps_write_nothing(pkg, ctx):
    c = s.case("corner")
    dev_build(pkg, ctx, "full")
    assert ctx.dense_info()["status"] == 3
    fr = s.scene("room")["frames"]
    for status in (3, 4):
        if status == 4:          # a frame removed that was never added: the map is inconsistent
            dev_build(pkg, ctx, "plane")
            ctx.dense_remove_frames(fr["cams"][:1], fr["K"], fr["rows"], fr["cols"], fr["depth"][:1])
            assert ctx.dense_info()["status"] == 4
        bufs = dict(cams=np.full((1, 7), 7.5), frames=(pkg.abi.EslDenseAlignFrame * 1)(), sums=np.full((1, 5, 37), 77, np.int64))
        bufs["frames"][0].status = 77
        rc, res = raw_align(pkg, ctx, c["cams"], 1, c["K"], c["rows"], c["cols"], c["depth"], bufs=bufs)
        assert rc == 0 and res == dict(status=status, n_voxels=-1, n_valid=0, n_passes=0)
        assert (bufs["cams"] == 7.5).all() and (bufs["sums"] == 77).all() and bufs["frames"][0].status == 77
        n = ctx.dense_normals(cap=4)
        assert n["result"] == dict(status=status, n_voxels=-1, n_eligible=0, n_valid=0) and len(n["normal"]) == 0
    assert dar.align(s.extract("full"), s.PLEAF, s.scene("full")["params"], c["cams"], c["K"], c["rows"], c["cols"], c["depth"])["result"]["status"] == 3


# ---- the resident cameras and the errors ---------------------------------------------------------------------------------------------------
def test_resident_cameras_and_errors(pkg, refs):
    g, cam0, obj0, _ = pkg.synth.make_graph(5, 8, 40, seed=3)
    c = s.case("corner")
    cx = pkg.Context(0)
    P = pkg.abi.default_dense_align_params
    try:
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_align_frames: no esl_dense_begin before"):
            cx.dense_align_frames(c["cams"], c["K"], c["rows"], c["cols"], c["depth"])
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_normals: no esl_dense_begin before"):
            cx.dense_normals(cap=1)
        dev_build(pkg, cx, "room")
        before = snapshot(cx)
        L = pkg.lib.load()

        def refused(status, what, **kw):
            a = dict(cams=c["cams"], F=1, K=c["K"], rows=c["rows"], cols=c["cols"], depth=c["depth"])
            a.update(kw)
            rc, _ = raw_align(pkg, cx, a["cams"], a["F"], a["K"], a["rows"], a["cols"], a["depth"], p=a.get("p"), out=a.get("out", True))
            msg = L.esl_last_error().decode()
            assert rc == status and msg.startswith("esl_dense_align_frames: ") and what in msg, (rc, msg)
        refused(4, "NULL cams needs a resident graph with states", cams=None)
        cx.upload_graph(g); cx.upload_states(cam0, obj0)
        c0, _ = cx.download_states()
        F = len(c0)
        depth = np.repeat(c["depth"], F, axis=0)
        given = cx.dense_align_frames(c0, c["K"], c["rows"], c["cols"], depth)
        res = cx.dense_align_frames(None, c["K"], c["rows"], c["cols"], depth)          # the resident camera states: the same bytes
        assert res["result"] == given["result"]
        same_bytes(res, given)
        refused(2, "F differs from the resident graph's n_cams", cams=None, F=F - 1, depth=depth)
        refused(2, "null out", out=False)
        refused(2, "negative F", F=-1)
        refused(2, "null K", K=None)
        refused(2, "null depth", depth=None)
        refused(2, "rows", rows=0); refused(2, "cols", cols=16385)
        refused(2, "fx", K=(0.0, 60.0, 1.0, 1.0)); refused(2, "fy", K=(60.0, np.inf, 1.0, 1.0)); refused(2, "cx or cy", K=(60.0, 60.0, np.nan, 1.0))
        refused(2, "max_dist", p=P(max_dist=-1.0)); refused(2, "damping", p=P(damping=np.nan)); refused(2, "min_pivot_ratio", p=P(min_pivot_ratio=-1e-9))
        refused(2, "tol_t", p=P(tol_t=np.inf)); refused(2, "tol_r", p=P(tol_r=-1.0))
        refused(2, "iters", p=P(iters=-1)); refused(2, "iters", p=P(iters=65)); refused(2, "stride", p=P(stride=0))
        refused(2, "reach", p=P(reach=-1)); refused(2, "reach", p=P(reach=3)); refused(2, "min_inliers", p=P(min_inliers=0))
        refused(2, "max_curvature", p=P(max_curvature=-0.1)); refused(2, "radius", p=P(radius=0)); refused(2, "radius", p=P(radius=3))
        refused(2, "min_count", p=P(min_count=0)); refused(2, "min_neighbors", p=P(min_neighbors=0))
        bad = c["cams"].copy(); bad[0, 3:] = 0
        refused(2, "a pose", cams=bad)
        # the bound of step c: a gate of 2^16 m squares to 2^32, times 2^30: one sample would reach 2^62 (the statement refuses it too)
        refused(2, "2^62", p=P(max_dist=65536.0))
        assert not dar.sums_fit(4800, dar.bound(c["K"], c["rows"], c["cols"], 6.0, 65536.0 ** 2))
        assert raw_align(pkg, None, c["cams"], 1, c["K"], c["rows"], c["cols"], c["depth"])[0] == 2
        rcn = L.esl_dense_normals(cx._h, ctypes.byref(pkg.abi.default_dense_normal_params(radius=3)), 0, None, None, None, None,
                                  ctypes.byref(pkg.abi.EslDenseNormalResult()))
        assert rcn == 2 and L.esl_last_error().decode().startswith("esl_dense_normals: radius")
        assert L.esl_dense_normals(cx._h, None, -1, None, None, None, None, ctypes.byref(pkg.abi.EslDenseNormalResult())) == 2
        assert L.esl_dense_normals(cx._h, None, 0, None, None, None, None, None) == 2
        # iters 64, reach 2, radius 2 are the last valid values; every refused call left the map alone
        assert snapshot(cx) == before
        ok = cx.dense_align_frames(c["cams"], c["K"], c["rows"], c["cols"], c["depth"], P(iters=64, reach=2, radius=2, min_neighbors=12))
        assert_same(ok, refs("corner", iters=64, reach=2, radius=2, min_neighbors=12))
        cx.dense_end()
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_align_frames: no esl_dense_begin before"):
            cx.dense_align_frames(c["cams"], c["K"], c["rows"], c["cols"], c["depth"])
    finally:
        cx.close()


# ---- the refusal ladder: every argument wrong at once, repaired one rung at a time, in the entry's order ----------------------------------------
def test_refusal_ladder(pkg):
    """esl_dense_align_frames with every argument wrong at once: the status and the whole text of the first refusal, that argument
    repaired, the next refusal, through the entry's sequence.  No map until "no esl_dense_begin before" has come out, then a map of
    one 4 x 4 frame; no kernel of the entry runs until the last call."""
    who = "esl_dense_align_frames"
    P = pkg.abi.default_dense_align_params
    L = pkg.lib.load()
    good = np.array([[0, 0, 0, 0, 0, 0, 1.0]] * 8)
    bad = good.copy(); bad[5, 3:] = 0
    depth = np.full((1, 4, 4), 5000, np.uint16)
    K = (60.0, 60.0, 1.5, 1.5)
    a = dict(cx=None, out=False, cams=None, F=-1, K=None, rows=0, cols=16385, depth=None)          # every argument wrong
    p = dict(max_dist=-1.0, damping=np.nan, min_pivot_ratio=-1e-9, tol_t=np.inf, tol_r=-1.0, iters=65, stride=0, reach=3, min_inliers=0,
             max_curvature=-0.1, radius=3, min_count=0, min_neighbors=0)
    ladder = [          # (status, text, the repair of an argument or (in a tuple) of a parameter); 16384 x 16384 x 8 frames hold 2^31 samples
        (2, "null ctx", "ctx"),
        (2, "null out", dict(out=True)),
        (2, "negative F", dict(F=8)),
        (2, "null K", dict(K=(0.0, np.inf, np.nan, 1.5))),
        (2, "rows < 1 or > 16384", dict(rows=16384)),
        (2, "cols < 1 or > 16384", dict(cols=16384)),
        (2, "fx not finite or <= 0", dict(K=(60.0, np.inf, np.nan, 1.5))),
        (2, "fy not finite or <= 0", dict(K=(60.0, 60.0, np.nan, 1.5))),
        (2, "cx or cy not finite", dict(K=K)),
        (2, "null depth", dict(depth=depth)),
        (2, "max_dist not finite or negative", (dict(max_dist=65536.0),)),
        (2, "damping not finite or negative", (dict(damping=0.0),)),
        (2, "min_pivot_ratio not finite or negative", (dict(min_pivot_ratio=1e-6),)),
        (2, "tol_t not finite or negative", (dict(tol_t=1e-5),)),
        (2, "tol_r not finite or negative", (dict(tol_r=1e-5),)),
        (2, "iters outside 0 .. 64", (dict(iters=64),)),
        (2, "stride < 1", (dict(stride=1),)),
        (2, "reach outside 0 .. 2", (dict(reach=2),)),
        (2, "min_inliers < 1", (dict(min_inliers=1),)),
        (2, "max_curvature not finite or negative", (dict(max_curvature=0.05),)),
        (2, "radius outside 1 .. 2", (dict(radius=2),)),
        (2, "min_count < 1", (dict(min_count=1),)),
        (2, "min_neighbors < 1", (dict(min_neighbors=1),)),
        (4, "no esl_dense_begin before", "map"),
        (4, "NULL cams needs a resident graph with states", dict(cams=bad)),
        (2, "a pose with a non-finite number or a quaternion of norm 0", dict(cams=good)),
        (2, "more samples than a map holds: 2^31", dict(rows=4, cols=4, F=1)),
        (2, "the sums of a frame could reach 2^62", (dict(max_dist=0.0),)),
    ]
    cx = pkg.Context(0)

    def call():
        return raw_align(pkg, a["cx"], a["cams"], a["F"], a["K"], a["rows"], a["cols"], a["depth"], p=P(**p), out=a["out"])
    try:
        for status, text, repair in ladder:
            rc, _ = call()
            assert (rc, L.esl_last_error().decode()) == (status, f"{who}: {text}")
            if repair == "ctx":
                a["cx"] = cx
            elif repair == "map":
                cx.dense_begin()
                cx.dense_add_frames(good[:1], K, 4, 4, depth, np.full((1, 4, 4, 3), 9, np.uint8), np.zeros((1, 4, 4), np.int32))
                before = snapshot(cx)
            elif isinstance(repair, tuple):
                p.update(repair[0])
            else:
                a.update(repair)
        assert snapshot(cx) == before          # every refused call left the map alone
        rc, res = call()
        assert rc == 0 and res["status"] == 0 and res["n_voxels"] > 0 and 1 <= res["n_passes"] <= 65 and snapshot(cx) == before
    finally:
        cx.close()
