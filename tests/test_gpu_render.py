"""esl_render_map on the device against its numpy statement (tests/render_ref.py).

Comparison rule (tests/render_scenes.py): inst, cover, cmp and flags are exact; depth is NaN in the same places and agrees within
TOL = 1e-9 m where finite (ten times the disagreement of the statement's own two formulations, and not below closed-form double
arithmetic).  Every scene is first checked, on the reference alone, for the conditions that make the exact part a fair demand
(check_conditions); the reference of a scene is computed once and shared."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as rr          # noqa: E402
import render_scenes as sc       # noqa: E402

pytestmark = pytest.mark.gpu

ALL = ("depth", "inst", "cover", "flags")


@functools.lru_cache(maxsize=None)
def scene_ref(name, seed=0):
    s = dict(room=sc.room_scene, crowd=sc.crowd_scene)[name](seed) if name in ("room", "crowd") else getattr(sc, name + "_scene")()
    return s, sc.check_conditions(sc.reference(s))


def dev_render(ctx, s, depth_meas=None, params=None, want=ALL):
    return ctx.render_map(s["cams"], s["objs"], s["K"], s["rows"], s["cols"], depth_meas, params, want)


def assert_render(dev, ref, keys=None):
    keys = set(dev) if keys is None else set(keys)
    assert keys <= set(dev)
    for k in keys - {"depth"}:
        assert dev[k].shape == ref[k].shape and dev[k].dtype == np.int32, k
        assert np.array_equal(dev[k], ref[k]), (k, np.argwhere(dev[k] != ref[k])[:5])
    if "depth" in keys:
        assert dev["depth"].shape == ref["depth"].shape
        nan = np.isnan(ref["depth"])
        assert np.array_equal(np.isnan(dev["depth"]), nan)
        if not nan.all():
            err = np.abs(dev["depth"][~nan] - ref["depth"][~nan]).max()
            assert err <= sc.TOL, err


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def check_scene(pkg, ctx, s, depth_meas=None, **over):
    ref = sc.check_conditions(sc.reference(s, depth_meas, **over))
    dev = dev_render(ctx, s, depth_meas, pkg.abi.default_render_params(**over))
    assert_render(dev, ref)
    return dev, ref


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sc.ROOM_SEEDS)
def test_rooms(ctx, seed):
    s, ref = scene_ref("room", seed)
    assert (ref["cover"][:, :, 1] < ref["cover"][:, :, 0]).any() and (ref["inst"] >= 0).sum() > 1000          # bodies hide each other
    assert_render(dev_render(ctx, s), ref)


def test_more_records_than_a_chunk(ctx):
    s, ref = scene_ref("crowd")
    tile = ref["inst"][0, 16:32, 16:32]
    assert len(s["objs"]) == 257 and len(np.unique(tile[tile >= 0])) >= 20
    assert ref["cover"][0, 256, 0] > 0 or ref["flags"][0, 256] & rr.DRAWN          # the record of the second chunk takes part
    assert_render(dev_render(ctx, s), ref)


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 17), (17, 1)])
def test_small_images(pkg, ctx, rows, cols):
    s = dict(sc.room_scene(0), rows=rows, cols=cols, K=(60.0, 60.0, (cols - 1) / 2 + 0.25, (rows - 1) / 2 + 0.3))
    s["objs"] = np.concatenate([s["objs"], sc.sphere([0.02, 0.01, 2.0], 0.3)[None, :]])          # something on the axis
    _, ref = check_scene(pkg, ctx, s)
    assert (ref["inst"] >= 0).any()


def test_degenerate_shapes(ctx):
    s, ref = scene_ref("room", 0)
    F, M = len(s["cams"]), len(s["objs"])
    d = ctx.render_map(np.zeros((0, 7)), s["objs"], s["K"], s["rows"], s["cols"])
    assert d["depth"].shape == (0, s["rows"], s["cols"]) and d["cover"].shape == (0, M, 2) and d["flags"].shape == (0, M)
    d = ctx.render_map(s["cams"], np.zeros((0, 10)), s["K"], s["rows"], s["cols"], np.zeros((F, s["rows"], s["cols"]), np.uint16))
    assert np.isnan(d["depth"]).all() and (d["inst"] == -1).all() and d["depth"].shape == (F, s["rows"], s["cols"])
    assert d["cover"].shape == (F, 0, 2) and d["cmp"].shape == (F, 0, 4) and d["flags"].shape == (F, 0)
    assert dev_render(ctx, s, want=()) == {}          # all outputs NULL
    raw = sc.planted_depth(ref)
    refc = sc.check_conditions(sc.reference(s, raw))
    for k in ALL:          # each output alone
        d = dev_render(ctx, s, want=(k,))
        assert set(d) == {k}
        assert_render(d, ref)
    d = dev_render(ctx, s, raw, want=())          # cmp alone
    assert set(d) == {"cmp"}
    assert_render(d, refc)


def test_union_of_occluders(pkg, ctx):
    """B stands behind two neighbours that each hide about 0.6 of it: esl_predict_boxes, which knows single occluders only, keeps it as a
    candidate; the ray cast finds no pixel of it"""
    s, ref = scene_ref("occluder")
    dev = dev_render(ctx, s)
    assert_render(dev, ref)
    n = dev["cover"][0, 0, 0]
    assert n > 500 and dev["cover"][0, 0, 1] == 0 and not (dev["inst"] == 0).any()
    p = pkg.abi.default_assoc_params()
    boxes, _, flags = ctx.predict_boxes(s["cams"][0], s["objs"], s["K"], s["rows"], s["cols"], p)
    assert list(flags) == [1, 1, 1]          # eligible, NOT occluded
    area = lambda b: max(b[2] - b[0], 0.0) * max(b[3] - b[1], 0.0)          # noqa: E731
    for k in (1, 2):
        inter = [max(boxes[0][0], boxes[k][0]), max(boxes[0][1], boxes[k][1]), min(boxes[0][2], boxes[k][2]), min(boxes[0][3], boxes[k][3])]
        share = area(inter) / area(boxes[0])
        assert 0.45 < share < p.occl_ratio - 0.05, share
    # the boxes are those of the statement's conic
    for k in range(3):
        Rco, tco = rr.camera_frame(s["cams"][0], s["objs"][k])
        _, box = rr.conic_box(Rco, tco, np.abs(s["objs"][k][7:]), s["K"])
        assert np.abs(np.clip(box, 0, [s["cols"], s["rows"]] * 2) - boxes[k]).max() < 1e-6


def test_ties_go_to_the_lower_index(pkg, ctx):
    s = sc.room_scene(1)
    s["objs"] = np.concatenate([s["objs"], s["objs"][[4, 0]]])          # rows 12 and 13: bit-identical copies of 4 and 0
    dev, ref = check_scene(pkg, ctx, s)
    for copy, orig in ((12, 4), (13, 0)):
        assert (dev["cover"][:, copy, 0] == dev["cover"][:, orig, 0]).all() and dev["cover"][:, orig, 0].sum() > 0
        assert not dev["cover"][:, copy, 1].any() and not (dev["inst"] == copy).any()
    assert dev["cover"][:, [4, 0], 1].sum() > 0


def test_nothing_drawn(ctx):
    s, ref = scene_ref("nothing")
    dev = dev_render(ctx, s)
    assert_render(dev, ref)
    assert list(dev["flags"][0]) == [rr.INSIDE, rr.INVALID, rr.INVALID, rr.INVALID, 0]
    assert np.isnan(dev["depth"]).all() and (dev["inst"] == -1).all() and not dev["cover"].any()


def test_body_across_the_principal_plane(ctx):
    s, ref = scene_ref("across")
    dev = dev_render(ctx, s)
    assert_render(dev, ref)
    assert dev["flags"][0, 0] == rr.DRAWN and dev["flags"][0, 1] == rr.DRAWN | rr.BOUNDED and dev["cover"][0, 0, 1] > 50


def test_depth_comparison(pkg, ctx):
    s, ref = scene_ref("room", 2)
    raw = sc.planted_depth(ref)
    dev, refc = check_scene(pkg, ctx, s, raw)
    assert (refc["cmp"].sum((0, 1)) > 50).all()          # all four categories occur
    assert np.array_equal(dev["cmp"].sum(-1), dev["cover"][:, :, 1])
    # other parameters: a tighter tolerance and a nearer far limit move samples between the categories
    dev2, _ = check_scene(pkg, ctx, s, raw, depth_tol=0.2, depth_max=4.0, depth_scale=5000.0, depth_min=0.1)
    assert not np.array_equal(dev2["cmp"], dev["cmp"]) and np.array_equal(dev2["cmp"].sum(-1), dev2["cover"][:, :, 1])


# ---- the resident forms ---------------------------------------------------------------------------------------------------------------------------
def test_resident_forms_leave_the_graph_alone(pkg):
    g, c, o, _ = pkg.synth.make_graph(12, 30, 200, seed=3)
    K = tuple(0.1 * k for k in g.K)
    p = pkg.default_lm_params(jacobian_mode=1)
    cx, plain = pkg.Context(0), pkg.Context(0)
    try:
        for k in (cx, plain):
            k.upload_graph(g); k.upload_states(c, o)
        c0, o0 = cx.download_states()
        given = cx.render_map(c0, o0, K, 48, 64)
        assert (given["inst"] >= 0).sum() > 100
        same_bits(given, cx.render_map(None, None, K, 48, 64))
        same_bits(given, cx.render_map(None, o0, K, 48, 64))
        same_bits(given, cx.render_map(c0, None, K, 48, 64))
        c1, o1 = cx.download_states()
        assert c0.tobytes() == c1.tobytes() and o0.tobytes() == o1.tobytes()
        ra, rb = cx.optimize_resident(p), plain.optimize_resident(p)
        assert ra["trace_chi2"] == rb["trace_chi2"] and ra["chi2_final"] == rb["chi2_final"]
        ca, oa = cx.download_states()
        cb, ob = plain.download_states()
        assert ca.tobytes() == cb.tobytes() and oa.tobytes() == ob.tobytes()
        with pytest.raises(pkg.EslError, match="esl_status 2.*n_cams"):
            load_call(pkg, cx, cams=None, F=g.n_cams - 1, objs=None, M=g.n_objs)
        with pytest.raises(pkg.EslError, match="esl_status 2.*n_objs"):
            load_call(pkg, cx, cams=None, F=g.n_cams, objs=None, M=g.n_objs - 1)
    finally:
        cx.close(); plain.close()


def load_call(pkg, cx, cams, F, objs, M, K=(60.0, 60.0, 35.0, 25.0), rows=8, cols=8, meas=None, p=None, depth=None, inst=None, cover=None,
              cmp_=None, flags=True, ctx_h=True):
    """the C-ABI itself, every argument free; raises like the binding"""
    L = pkg.lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    keep = []

    def arr(a, dt, t):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt); keep.append(a)
        return a.ctypes.data_as(t)
    Kp = None if K is None else arr(K, np.float64, dp)
    fl = np.zeros(max(F * M, 1), np.int32) if flags is True else flags
    rc = L.esl_render_map(cx._h if ctx_h else None, arr(cams, np.float64, dp), F, arr(objs, np.float64, dp), M, Kp, rows, cols,
                          arr(meas, np.uint16, ctypes.POINTER(ctypes.c_uint16)), None if p is None else ctypes.byref(p),
                          arr(depth, np.float64, dp), arr(inst, np.int32, ip), arr(cover, np.int32, ip), arr(cmp_, np.int32, ip),
                          arr(fl, np.int32, ip))
    if rc != 0:
        raise pkg.EslError(f"esl_render_map failed with esl_status {rc}: {L.esl_last_error().decode()}")
    return fl


# ---- repeats and buffers ----------------------------------------------------------------------------------------------------------------------------
def test_repeats_and_grow_only_buffers(pkg):
    big, _ = scene_ref("crowd")
    small, ref_small = scene_ref("room", 3)
    raw = sc.planted_depth(ref_small)
    cx = pkg.Context(0)
    try:
        assert cx.render_allocs() == (0, 0)
        a0 = dev_render(cx, big)
        b0 = dev_render(cx, small, raw)
        allocs = cx.render_allocs()
        assert allocs[0] > 0 and allocs[1] > 0
        a1 = dev_render(cx, big)          # warm: the same shapes again, and the smaller one after the larger
        b1 = dev_render(cx, small, raw)
        assert cx.render_allocs() == allocs          # nothing allocated
        same_bits(a0, a1); same_bits(b0, b1)
        assert_render(b1, sc.check_conditions(sc.reference(small, raw)))
        half = dict(small, cams=small["cams"][:1], objs=small["objs"][:5])
        check_scene(pkg, cx, half)          # a smaller call after a larger one reads nothing the larger one left behind
        assert cx.render_allocs() == allocs
    finally:
        cx.close()


def test_profiling_class_4(pkg):
    s, _ = scene_ref("room", 0)
    cx = pkg.Context(0)
    try:
        cx.profile_enable(2)
        dev_render(cx, s)
        prof = cx.profile_get()
        assert set(prof) == {"reduce"} and prof["reduce"]["count"] >= 1 and prof["reduce"]["total_ms"] > 0
    finally:
        cx.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------------
def test_errors(pkg):
    s, _ = scene_ref("room", 0)
    cams, objs = s["cams"], s["objs"]
    F, M = len(cams), len(objs)
    cx = pkg.Context(0)
    P = pkg.abi.default_render_params
    try:
        ok = dict(cams=cams, F=F, objs=objs, M=M)
        load_call(pkg, cx, **ok)
        nan, inf = float("nan"), float("inf")
        cases = [
            (dict(ctx_h=False), "ctx"), (dict(F=-1), "F"), (dict(M=-1), "M"), (dict(K=None), "K"),
            (dict(rows=0), "rows"), (dict(rows=16385), "rows"), (dict(cols=0), "cols"), (dict(cols=16385), "cols"), (dict(rows=-3), "rows"),
            (dict(K=(0.0, 60, 4, 4)), "fx"), (dict(K=(nan, 60, 4, 4)), "fx"), (dict(K=(inf, 60, 4, 4)), "fx"), (dict(K=(-60.0, 60, 4, 4)), "fx"),
            (dict(K=(60, 0.0, 4, 4)), "fy"), (dict(K=(60, nan, 4, 4)), "fy"), (dict(K=(60, -1.0, 4, 4)), "fy"),
            (dict(p=P(depth_scale=0.0)), "depth_scale"), (dict(p=P(depth_scale=-1.0)), "depth_scale"), (dict(p=P(depth_scale=nan)), "depth_scale"),
            (dict(p=P(depth_scale=inf)), "depth_scale"),
            (dict(p=P(depth_min=-0.1)), "depth_min"), (dict(p=P(depth_min=nan)), "depth_min"),
            (dict(p=P(depth_max=inf)), "depth_max"), (dict(p=P(depth_max=nan)), "depth_max"),
            (dict(p=P(depth_tol=-1e-3)), "depth_tol"), (dict(p=P(depth_tol=nan)), "depth_tol"),
            (dict(p=P(depth_min=3.0, depth_max=2.0)), "depth_min > depth_max"),
            (dict(cmp_=np.zeros(F * M * 4, np.int32)), "cmp_out needs depth_meas"),
        ]
        for over, word in cases:
            with pytest.raises(pkg.EslError, match="esl_status 2: esl_render_map: .*" + word):
                load_call(pkg, cx, **dict(ok, **over))
        # a NULL source without a resident graph
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_render_map: NULL cams"):
            load_call(pkg, cx, **dict(ok, cams=None))
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_render_map: NULL objs"):
            load_call(pkg, cx, **dict(ok, objs=None))
        with pytest.raises(pkg.EslError, match="esl_status 4"):
            load_call(pkg, cx, cams=None, F=1, objs=None, M=1)
        # valid all the same: nothing to do
        load_call(pkg, cx, cams=None, F=0, objs=objs, M=M)
        load_call(pkg, cx, cams=cams, F=F, objs=None, M=0)
        load_call(pkg, cx, cams=None, F=0, objs=None, M=0, flags=None)
        load_call(pkg, cx, **dict(ok, p=P(depth_min=2.0, depth_max=2.0, depth_tol=0.0)))
        # the binding's own checks
        with pytest.raises(ValueError):
            cx.render_map(cams, objs, s["K"], 8, 8, depth_meas=np.zeros((F, 8, 9), np.uint16))
        with pytest.raises(ValueError):
            cx.render_map(cams, objs, s["K"], 8, 8, want=("colour",))
    finally:
        cx.close()
