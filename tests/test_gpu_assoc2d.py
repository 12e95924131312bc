"""esl_predict_boxes / esl_associate_boxes on the device against their numpy statement (tests/assoc2d_ref.py).

Comparison rule: assoc, flags and frame_stats are exact; boxes, depth and iou agree within assoc2d_scenes.TOL = 1.02e-8 -- ten times
the 1.02e-9 px by which the numpy statement itself differs from the C oracle's projection (measured and asserted on the CPU in
tests/test_assoc2d_ref.py), and not below the 1e-9 of closed-form double arithmetic.  Every scene is first checked for the condition
that makes the exact part a fair demand (assoc2d_scenes.check_conditions: no decision quantity within 2e-6 of its threshold, at least
100 times the tolerance); the reference of a scene is computed once and shared."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc2d_ref as ar        # noqa: E402
import assoc2d_scenes as sc     # noqa: E402

pytestmark = pytest.mark.gpu

K, ROWS, COLS = sc.K, sc.ROWS, sc.COLS
TILE = 1024   # kAssocTile of csrc/esl_assoc.hip (include/esl.h names it)


@functools.lru_cache(maxsize=None)
def room(seed):
    return sc.room_scene(seed)


@functools.lru_cache(maxsize=None)
def grid(n):
    s = sc.grid_scene(n)
    return s, sc.reference(s)


def dev_of(pkg, ctx, s, **over):
    return ctx.associate_boxes(s["cams"], s["objs"], s["obj_labels"], s["K"], s["rows"], s["cols"], s["det_offsets"], s["det_boxes"],
                               s["det_labels"], pkg.abi.default_assoc_params(**over))


def assert_same(dev, ref):
    assoc, iou, stats = dev
    assert np.array_equal(assoc, ref["assoc"]), (assoc, ref["assoc"])
    assert np.array_equal(stats[:, :3], ref["frame_stats"][:, :3]), (stats, ref["frame_stats"])
    assert iou.shape == ref["iou"].shape and (len(iou) == 0 or np.abs(iou - ref["iou"]).max() <= sc.TOL)
    assert np.array_equal(iou == 0, assoc < 0)


def assert_same_prediction(dev, pr):
    boxes, depth, flags = dev
    assert np.array_equal(flags, pr["flags"]), (flags, pr["flags"])
    el = (flags & 1).astype(bool)
    assert np.isnan(boxes[~el]).all() and np.isnan(depth[~el]).all()
    if el.any():
        assert np.abs(boxes[el] - pr["boxes"][el]).max() <= sc.TOL
        assert np.abs(depth[el] - pr["depth"][el]).max() <= sc.TOL


def check(pkg, ctx, s, **over):
    ref = sc.reference(s, **over)
    sc.check_conditions(ref)
    dev = dev_of(pkg, ctx, s, **over)
    assert_same(dev, ref)
    return dev, ref


def test_params_default_and_size(pkg):
    p = pkg.abi.EslAssocParams()
    pkg.lib.load().esl_assoc_params_default(ctypes.byref(p))
    d = pkg.abi.default_assoc_params()
    assert ctypes.sizeof(p) == 32
    for k, _ in pkg.abi.EslAssocParams._fields_:
        assert getattr(p, k) == getattr(d, k) == ar.DEFAULTS[k], k
    assert sc.CONDITION >= 100 * sc.TOL and sc.TOL >= 1e-9


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_room_scenes(pkg, ctx, seed):
    s = room(seed)
    (assoc, _, stats), _ = check(pkg, ctx, s)
    assert np.array_equal(assoc, s["true_obj"]) and (stats[:, 3] == 0).all()


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_predict_frame_0(pkg, ctx, seed):
    s = room(seed)
    pr = ar.predict(s["cams"][0], s["objs"], K, ROWS, COLS)
    assert pr["margin"] > sc.CONDITION
    dev = ctx.predict_boxes(s["cams"][0], s["objs"], K, ROWS, COLS)
    assert_same_prediction(dev, pr)
    assert (dev[2] == 3).any() and (dev[2] == 1).any() and (dev[2] == 0).any()


def test_switches(pkg, ctx):
    s = room(1)
    (a0, _, st0), _ = check(pkg, ctx, s)
    # labels ignored: same boxes, so the same answer here, through the other candidate set
    lab = dict(s); lab["det_labels"] = (s["det_labels"] + 1).astype(np.int32)
    (a1, _, _), _ = check(pkg, ctx, lab, match_labels=0)
    assert np.array_equal(a1, a0)
    (a2, _, _), _ = check(pkg, ctx, lab)
    assert (a2 != a0).any()
    # occlusion off: nothing is hidden, so hidden predictions compete for the detections
    (_, _, st3), _ = check(pkg, ctx, s, occlusion=0)
    assert (st3[:, 1] == 0).all() and (st0[:, 1] > 0).all() and np.array_equal(st3[:, 0], st0[:, 0])
    pr = ar.predict(s["cams"][2], s["objs"], K, ROWS, COLS, dict(occlusion=0))
    assert_same_prediction(ctx.predict_boxes(s["cams"][2], s["objs"], K, ROWS, COLS, pkg.abi.default_assoc_params(occlusion=0)), pr)
    # a higher bar: fewer assignments
    (a4, _, st4), _ = check(pkg, ctx, room(0), min_iou=0.6)
    assert (a4 < 0).any() and st4[:, 2].sum() == (a4 >= 0).sum()
    # a larger smallest box and another coverage ratio, through predict
    for over in (dict(min_box_px=40.0), dict(occl_ratio=0.4)):
        pr = ar.predict(s["cams"][0], s["objs"], K, ROWS, COLS, over)
        assert pr["margin"] > sc.CONDITION
        assert_same_prediction(ctx.predict_boxes(s["cams"][0], s["objs"], K, ROWS, COLS, pkg.abi.default_assoc_params(**over)), pr)


def test_empty_inputs_and_degenerate_boxes(pkg, ctx):
    s = dict(room(2))
    off = s["det_offsets"].copy()
    # frame 1 loses its detections
    n1 = off[2] - off[1]
    keep = np.r_[0:off[1], off[2]:off[-1]]
    s["det_boxes"], s["det_labels"] = s["det_boxes"][keep], s["det_labels"][keep]
    s["det_offsets"] = np.concatenate([off[:2], off[2:] - n1]).astype(np.int32)
    (_, _, st), _ = check(pkg, ctx, s)
    assert st[1, 2] == 0 and st[1, 0] > 0
    # M = 0: every detection -1
    e = dict(s); e["objs"] = np.zeros((0, 10)); e["obj_labels"] = np.zeros(0, np.int32)
    assoc, iou, st = dev_of(pkg, ctx, e)
    assert (assoc == -1).all() and (iou == 0).all() and (st == 0).all() and len(assoc) == len(s["det_boxes"])
    b, d, f = ctx.predict_boxes(s["cams"][0], np.zeros((0, 10)), K, ROWS, COLS)
    assert b.shape == (0, 4) and len(d) == 0 and len(f) == 0
    # F = 0, and no detections at all
    assoc, iou, st = ctx.associate_boxes(np.zeros((0, 7)), s["objs"], s["obj_labels"], K, ROWS, COLS, [0], np.zeros((0, 4)), [])
    assert len(assoc) == 0 and len(iou) == 0 and st.shape == (0, 4)
    z = dict(s); z["det_offsets"] = np.zeros(len(s["cams"]) + 1, np.int32); z["det_boxes"] = np.zeros((0, 4)); z["det_labels"] = np.zeros(0, np.int32)
    (_, _, st), _ = check(pkg, ctx, z)
    assert (st[:, 0] > 0).all() and (st[:, 2] == 0).all()
    # degenerate detections: no width, no height, NaN, infinity -- -1, and the good box behind them still finds its object
    g = dict(room(3))
    o = g["det_offsets"]
    bad = g["det_boxes"].copy()
    first = bad[o[0]].copy()
    rows_bad = [[first[0], first[1], first[0], first[3]], [first[0], first[3], first[2], first[1]], [np.nan, first[1], first[2], first[3]],
                [first[0], first[1], np.inf, first[3]]]
    g["det_boxes"] = np.concatenate([np.array(rows_bad), bad]); g["det_labels"] = np.concatenate([[g["det_labels"][0]] * 4, g["det_labels"]]).astype(np.int32)
    g["det_offsets"] = np.concatenate([[0], o[1:] + 4]).astype(np.int32)
    (assoc, iou, _), _ = check(pkg, ctx, g)
    assert (assoc[:4] == -1).all() and (iou[:4] == 0).all() and np.array_equal(assoc[4:], g["true_obj"])


def test_behind_and_enclosing(pkg, ctx):
    objs = np.stack([sc.sphere([0, 0, -3.0], 0.4), sc.sphere([0.1, 0, 0.2], 1.0), sc.sphere([0, 0, 3.0], 0.4),
                     sc.sphere([0, 0, 30.0], 0.2), sc.sphere([0, 0, 6.0], 0.3)])
    pr = ar.predict(sc.IDENTITY_CAM, objs, K, ROWS, COLS)
    assert list(pr["flags"]) == [0, 0, 1, 0, 3] and pr["margin"] > sc.CONDITION
    assert_same_prediction(ctx.predict_boxes(sc.IDENTITY_CAM, objs, K, ROWS, COLS), pr)
    box = pr["boxes"][2]
    det = np.stack([box + [3, 0, 3, 0], box])
    assoc, iou, st = ctx.associate_boxes(sc.IDENTITY_CAM[None], objs, np.zeros(5, np.int32), K, ROWS, COLS, [0, 2], det, [0, 0])
    ref = ar.associate(sc.IDENTITY_CAM[None], objs, np.zeros(5, np.int32), K, ROWS, COLS, [0, 2], det, [0, 0])
    assert_same((assoc, iou, st), ref)
    assert list(assoc) == [2, -1] and list(st[0]) == [2, 1, 1, 0]      # row-order greedy: the first detection takes it


def test_overflow_path(pkg, ctx):
    """TILE + 1 eligible predictions go through the global scratch; the same scene with one sphere fewer stays on chip and gives
    identical results on the common detections"""
    s, ref = grid(TILE + 1)
    sc.check_conditions(ref)
    dev = dev_of(pkg, ctx, s)
    assert_same(dev, ref)
    assert list(dev[2][0]) == [TILE + 1, 0, 30, 1] and np.array_equal(dev[0], s["true_obj"])
    pr = ref["frames"][0]
    assert_same_prediction(ctx.predict_boxes(s["cams"][0], s["objs"], K, ROWS, COLS), pr)
    t, ref_t = grid(TILE)
    assert np.array_equal(t["det_boxes"], s["det_boxes"])
    dev_t = dev_of(pkg, ctx, t)
    assert_same(dev_t, ref_t)
    assert list(dev_t[2][0]) == [TILE, 0, 30, 0]
    assert np.array_equal(dev_t[0], dev[0]) and np.array_equal(dev_t[1], dev[1])      # bit for bit, the IoUs included
    # occlusion on the overflow path: a wall in front of the top-left corner of the grid hides the spheres behind it
    w = dict(s)
    w["objs"] = np.concatenate([s["objs"], sc.sphere([-4.0, -3.2, 10.0], 1.0)[None]]); w["obj_labels"] = np.append(s["obj_labels"], 9).astype(np.int32)
    (_, _, st), _ = check(pkg, ctx, w)
    assert st[0, 0] == TILE + 2 and st[0, 1] > 20 and st[0, 3] == 1


def test_resident_sources_leave_the_graph_alone(pkg, ctx):
    g, c, o, _ = pkg.synth.make_graph(12, 30, 200, seed=3, slam=True)
    p = pkg.default_lm_params(jacobian_mode=1, max_iters=3)
    rng = np.random.default_rng(0)
    labels = rng.integers(0, 3, g.n_objs).astype(np.int32)
    Kg = g.K
    ctx.upload_graph(g); ctx.upload_states(c, o); ctx.snapshot_states()
    rep_a = ctx.optimize_resident(p); ca, oa = ctx.download_states()
    ctx.restore_states()
    cd, od = ctx.download_states()
    off, bl, ll = [0], [], []       # detections: the device's own predictions, moved a little
    for f in range(g.n_cams):
        b, _, fl = ctx.predict_boxes(cd[f], od, Kg, ROWS, COLS)
        vis = np.nonzero(fl == 1)[0]
        bl.append(b[vis] + rng.uniform(-2, 2, size=(len(vis), 4))); ll.append(labels[vis]); off.append(off[-1] + len(vis))
    off, boxes, labs = np.array(off, np.int32), np.concatenate(bl), np.concatenate(ll)
    assert len(boxes) > 0
    given = ctx.associate_boxes(cd, od, labels, Kg, ROWS, COLS, off, boxes, labs)
    resident = ctx.associate_boxes(None, None, labels, Kg, ROWS, COLS, off, boxes, labs)
    assert (given[0] >= 0).any()
    for a, b in zip(given, resident):
        assert a.tobytes() == b.tobytes()
    pg = ctx.predict_boxes(cd[0], od, Kg, ROWS, COLS)
    pres = ctx.predict_boxes(cd[0], None, Kg, ROWS, COLS)
    for a, b in zip(pg, pres):
        assert a.tobytes() == b.tobytes()
    rep_b = ctx.optimize_resident(p); cb, ob = ctx.download_states()
    assert rep_a == rep_b and np.array_equal(ca, cb) and np.array_equal(oa, ob)
    other = pkg.Context(0)          # a context that never associated
    try:
        other.upload_graph(g); other.upload_states(c, o)
        assert other.optimize_resident(p) == rep_b
    finally:
        other.close()


def test_bit_identical_runs(pkg, ctx):
    s = room(4)
    a, b = dev_of(pkg, ctx, s), dev_of(pkg, ctx, s)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    pa, pb = ctx.predict_boxes(s["cams"][3], s["objs"], K, ROWS, COLS), ctx.predict_boxes(s["cams"][3], s["objs"], K, ROWS, COLS)
    for x, y in zip(pa, pb):
        assert x.tobytes() == y.tobytes()
    g, _ = grid(TILE + 1)
    a, b = dev_of(pkg, ctx, g), dev_of(pkg, ctx, g)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_errors(pkg):
    cx = pkg.Context(0)
    s = room(0)
    args = [s["cams"], s["objs"], s["obj_labels"], K, ROWS, COLS, s["det_offsets"], s["det_boxes"], s["det_labels"]]

    def call(i, v, **over):
        a = list(args); a[i] = v
        return cx.associate_boxes(*a, pkg.abi.default_assoc_params(**over))
    try:
        for i in (0, 1):                                              # a NULL source without a resident graph
            with pytest.raises(pkg.EslError, match="esl_status 4"):
                call(i, None)
        with pytest.raises(pkg.EslError, match="esl_status 4"):
            cx.predict_boxes(s["cams"][0], None, K, ROWS, COLS)
        for k in ("min_iou", "occl_ratio", "min_box_px"):
            for v in (float("nan"), float("inf"), -0.1):
                with pytest.raises(pkg.EslError, match="esl_status 2"):
                    call(3, K, **{k: v})
                with pytest.raises(pkg.EslError, match="esl_status 2"):
                    cx.predict_boxes(s["cams"][0], s["objs"], K, ROWS, COLS, pkg.abi.default_assoc_params(**{k: v}))
        for i in (4, 5):                                              # rows, cols < 1
            with pytest.raises(pkg.EslError, match="esl_status 2"):
                call(i, 0)
        with pytest.raises(pkg.EslError, match="esl_status 2"):
            cx.predict_boxes(s["cams"][0], s["objs"], K, 0, COLS)
        off = s["det_offsets"].copy(); off[0] = 1
        with pytest.raises(pkg.EslError, match="esl_status 2"):
            call(6, off)
        off = s["det_offsets"].copy(); off[2] = off[1] - 1
        with pytest.raises(pkg.EslError, match="esl_status 2"):
            call(6, off)
        # the C-ABI itself: null pointers and negative counts
        L = pkg.lib.load()
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        Kc = (ctypes.c_double * 4)(*K); T = (ctypes.c_double * 7)(0, 0, 0, 0, 0, 0, 1); o1 = (ctypes.c_double * 10)(0, 0, 3, 0, 0, 0, 1, .4, .4, .4)
        off2 = (ctypes.c_int32 * 2)(0, 0); lab1 = (ctypes.c_int32 * 1)(0)
        bx, dz, fl = (ctypes.c_double * 4)(), (ctypes.c_double * 1)(), (ctypes.c_int32 * 1)()
        assert L.esl_predict_boxes(cx._h, None, o1, 1, Kc, ROWS, COLS, None, bx, dz, fl) == 2
        assert L.esl_predict_boxes(cx._h, T, o1, -1, Kc, ROWS, COLS, None, bx, dz, fl) == 2
        assert L.esl_predict_boxes(cx._h, T, o1, 1, None, ROWS, COLS, None, bx, dz, fl) == 2
        assert L.esl_predict_boxes(cx._h, T, o1, 1, Kc, ROWS, COLS, None, None, dz, fl) == 2
        assert L.esl_predict_boxes(cx._h, T, None, 1, Kc, ROWS, COLS, None, bx, dz, fl) == 4
        assert L.esl_predict_boxes(None, T, o1, 1, Kc, ROWS, COLS, None, bx, dz, fl) == 2
        assert L.esl_associate_boxes(cx._h, T, -1, o1, lab1, 1, Kc, ROWS, COLS, off2, None, None, None, None, None, None) == 2
        assert L.esl_associate_boxes(cx._h, T, 1, o1, lab1, 1, Kc, ROWS, COLS, None, None, None, None, None, None, None) == 2
        assert L.esl_associate_boxes(cx._h, T, 1, o1, None, 1, Kc, ROWS, COLS, off2, None, None, None, None, None, None) == 2
        off3 = (ctypes.c_int32 * 2)(0, 1)
        assert L.esl_associate_boxes(cx._h, T, 1, o1, lab1, 1, Kc, ROWS, COLS, off3, None, None, None, None, None, None) == 2
        # F and M against a resident graph
        g, c, o, _ = pkg.synth.make_graph(6, 5, 40, seed=1)
        cx.upload_graph(g); cx.upload_states(c, o)
        offg = np.zeros(g.n_cams + 2, np.int32)
        with pytest.raises(pkg.EslError, match="esl_status 2"):
            cx.associate_boxes(None, o, np.zeros(g.n_objs, np.int32), K, ROWS, COLS, offg, np.zeros((0, 4)), [])
        with pytest.raises(pkg.EslError, match="esl_status 2"):
            cx.associate_boxes(c, None, np.zeros(g.n_objs + 1, np.int32), K, ROWS, COLS, offg[:-1], np.zeros((0, 4)), [])
        assoc, _, st = cx.associate_boxes(None, None, np.zeros(g.n_objs, np.int32), K, ROWS, COLS, offg[:-1], np.zeros((0, 4)), [])
        assert len(assoc) == 0 and st.shape == (g.n_cams, 4)
    finally:
        cx.close()
