"""esl_map_overlaps / esl_map_merge on the device against their numpy statement (tests/map_merge_ref.py).

Comparison rule (tests/map_merge_scenes.py): counts, pair lists, n_*, groups, indices, merged rows (as bytes) and the rewritten list are
exact; iou and contain agree within TOL = 1e-12.  Every scene is first checked, on the reference alone, for the conditions that make the
exact part a fair demand (check_conditions); the reference of a scene is computed once and shared."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_merge_ref as mr          # noqa: E402
import map_merge_scenes as sc       # noqa: E402

pytestmark = pytest.mark.gpu


def frozen(over):
    return tuple(sorted(over.items()))


@functools.lru_cache(maxsize=None)
def clutter_overlaps(seed, over=()):
    s = sc.clutter_scene(seed)
    ov = mr.overlaps(s["objs"], s["labels"], **dict(over))
    sc.check_conditions(ov)
    return ov


@functools.lru_cache(maxsize=None)
def scene_merge(name, seed, mode, over=()):
    """mode: 'weights' (given, with the list), 'list' (weights from the list), 'none' (no list: every weight 1)"""
    s = sc.planted_scene(seed) if name == "planted" else sc.clutter_scene(seed)
    w = s["weights"] if mode == "weights" else None
    cam, obj = (None, None) if mode == "none" else (s["obs_cam"], s["obs_obj"])
    r = mr.merge(s["objs"], s["labels"], w, cam, obj, **dict(over))
    sc.check_conditions(r["overlaps"])
    return s, (w, cam, obj), r


def dev_overlaps(pkg, ctx, objs, labels, cap=None, **over):
    return ctx.map_overlaps(objs, labels, pkg.abi.default_merge_params(**over), cap)


def dev_merge(pkg, ctx, objs, labels, weights=None, obs_cam=None, obs_obj=None, **over):
    return ctx.map_merge(objs, labels, weights, obs_cam, obs_obj, pkg.abi.default_merge_params(**over))


def assert_overlaps(dev, ref, cap=None):
    k = ref["n_pairs"] if cap is None else min(cap, ref["n_pairs"])
    assert (dev["n_pairs"], dev["n_candidates"]) == (ref["n_pairs"], ref["n_candidates"])
    assert np.array_equal(dev["pairs"], ref["pairs"][:k]), (dev["pairs"], ref["pairs"][:k])
    assert np.array_equal(dev["counts"], ref["counts"][:k]), (dev["counts"], ref["counts"][:k])
    assert dev["iou"].shape == (k,) and dev["contain"].shape == (k,)
    if k:
        assert np.abs(dev["iou"] - ref["iou"][:k]).max() <= sc.TOL and np.abs(dev["contain"] - ref["contain"][:k]).max() <= sc.TOL


def assert_merge(dev, ref):
    assert dev["result"] == ref["result"], (dev["result"], ref["result"])
    assert np.array_equal(dev["group"], ref["group"]) and np.array_equal(dev["new_index"], ref["new_index"])
    assert dev["objs"].tobytes() == ref["objs"].tobytes()
    assert np.array_equal(dev["labels"], ref["labels"]) and np.array_equal(dev["weights"], ref["weights"])
    if ref["obs_obj"] is None:
        assert dev["obs_obj"] is None
    else:
        assert np.array_equal(dev["obs_obj"], ref["obs_obj"])


def check_overlaps(pkg, ctx, objs, labels, **over):
    ref = mr.overlaps(objs, labels, **over)
    sc.check_conditions(ref)
    dev = dev_overlaps(pkg, ctx, objs, labels, **over)
    assert_overlaps(dev, ref)
    return dev, ref


def check_merge(pkg, ctx, objs, labels, weights=None, obs_cam=None, obs_obj=None, **over):
    ref = mr.merge(objs, labels, weights, obs_cam, obs_obj, **over)
    sc.check_conditions(ref["overlaps"])
    dev = dev_merge(pkg, ctx, objs, labels, weights, obs_cam, obs_obj, **over)
    assert_merge(dev, ref)
    return dev, ref


def test_params_default_and_sizes(pkg):
    p = pkg.abi.EslMergeParams()
    pkg.lib.load().esl_merge_params_default(ctypes.byref(p))
    d = pkg.abi.default_merge_params()
    assert ctypes.sizeof(p) == 32 and ctypes.sizeof(pkg.abi.EslMergeResult) == 48
    for k, _ in pkg.abi.EslMergeParams._fields_:
        assert getattr(p, k) == getattr(d, k) == mr.DEFAULTS[k], k


# ---- esl_map_overlaps -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sc.CLUTTER_SEEDS)
def test_overlaps_clutter(pkg, ctx, seed):
    s, ref = sc.clutter_scene(seed), clutter_overlaps(seed)
    assert ref["n_pairs"] > 100 and ref["n_candidates"] > ref["n_pairs"] and ref["link"].any() and not ref["link"].all()
    assert_overlaps(dev_overlaps(pkg, ctx, s["objs"], s["labels"]), ref)


@pytest.mark.parametrize("lattice", sorted(sc.CLUTTER_SEED_BY_LATTICE))
def test_overlaps_other_lattices(pkg, ctx, lattice):
    """4: 32 points, less than a wavefront; 5: odd n, a partial last round; 32: 512 rounds"""
    seed = sc.CLUTTER_SEED_BY_LATTICE[lattice]
    s, ref = sc.clutter_scene(seed), clutter_overlaps(seed, frozen(dict(lattice=lattice)))
    assert ref["n_pairs"] > 100 and ref["counts"].max() <= mr.n_ball(lattice)
    assert_overlaps(dev_overlaps(pkg, ctx, s["objs"], s["labels"], lattice=lattice), ref)


def test_overlaps_cap(pkg, ctx):
    s, ref = sc.clutter_scene(0), clutter_overlaps(0)
    for cap in (0, 1, 17, ref["n_pairs"], ref["n_pairs"] + 5):
        assert_overlaps(dev_overlaps(pkg, ctx, s["objs"], s["labels"], cap=cap), ref, cap)


def test_shapes(pkg, ctx):
    z = np.zeros(0, np.int32)
    dev = dev_overlaps(pkg, ctx, np.zeros((0, 10)), z)
    assert dev["n_pairs"] == 0 and dev["n_candidates"] == 0 and dev["pairs"].shape == (0, 2)
    dm = dev_merge(pkg, ctx, np.zeros((0, 10)), z)
    assert dm["result"] == dict(status=0, n_valid=0, n_groups=0, n_merged_groups=0, largest_group=0, n_conflicts=0, n_candidates=0,
                                n_pairs=0, n_links=0) and dm["objs"].shape == (0, 10) and len(dm["group"]) == 0
    dm = dev_merge(pkg, ctx, np.zeros((0, 10)), z, None, [3, 4], [-1, -5])          # a list of skipped entries on an empty map
    assert list(dm["obs_obj"]) == [-1, -1]
    pair = sc.chain(2)
    check_merge(pkg, ctx, pair[:1], [7])
    dev, _ = check_merge(pkg, ctx, pair, [7, 7])
    assert list(dev["group"]) == [0, 0] and dev["result"]["n_groups"] == 1
    # all invalid: NaN, zero quaternion, zero half-axis, infinite centre
    bad = sc.chain(4, spacing=0.1)
    bad[0, 9] = np.nan; bad[1, 3:7] = 0; bad[2, 8] = 0; bad[3, 0] = np.inf
    dev, ref = check_merge(pkg, ctx, bad, np.zeros(4, np.int32))
    assert dev["result"]["n_valid"] == 0 and dev["result"]["n_groups"] == 4 and dev["result"]["n_candidates"] == 0
    assert dev["objs"].tobytes() == bad.tobytes()
    assert dev_overlaps(pkg, ctx, bad, np.zeros(4, np.int32))["n_candidates"] == 0
    # one NaN among valid ones, a negative half-axis, an unnormalised quaternion
    objs = sc.chain(4, spacing=0.1)
    objs[1, 4] = np.nan; objs[2, 7] = -1.0; objs[3, 3:7] *= 3.0
    dev, _ = check_merge(pkg, ctx, objs, np.zeros(4, np.int32))
    assert list(dev["group"]) == [0, 1, 0, 0] and dev["result"]["n_valid"] == 3
    ov, _ = check_overlaps(pkg, ctx, objs, np.zeros(4, np.int32))
    assert [tuple(p) for p in ov["pairs"]] == [(0, 2), (0, 3), (2, 3)]
    rot = np.stack([sc.ell([0, 0, 0], [0.6, 0.3, 0.2], q=np.array([0.1, -0.3, 0.2, 0.9]) * s) for s in (1 / np.linalg.norm([0.1, -0.3, 0.2, 0.9]), 5.0)])
    ov, _ = check_overlaps(pkg, ctx, rot, [0, 0])
    assert list(ov["counts"][0]) == [mr.n_ball(16)] * 2          # the same body: the scale of the quaternion does not matter


def test_pair_geometry(pkg, ctx):
    big = sc.ell([0.3, 0.1, -0.2], [0.9, 0.7, 0.8], yaw=0.4)
    nb = mr.n_ball(16)
    ov, _ = check_overlaps(pkg, ctx, np.stack([big, big]), [0, 0])
    assert list(ov["counts"][0]) == [nb, nb] and abs(ov["iou"][0] - 1) <= sc.TOL and ov["contain"][0] == 1.0
    small = sc.ell([0.35, 0.15, -0.1], [0.3, 0.2, 0.25], yaw=1.1)
    dev, ref = check_merge(pkg, ctx, np.stack([big, small]), [0, 0])
    ovr = ref["overlaps"]
    assert ovr["iou"][0] < 0.3 and ovr["contain"][0] >= 0.7 and ovr["counts"][0, 1] == nb          # by containment alone
    assert list(dev["group"]) == [0, 0] and dev["result"]["n_links"] == 1
    flat = np.stack([sc.ell([0, 0, 0], [0.9, 0.9, 0.1]), sc.ell([0, 0, 0.8], [0.9, 0.9, 0.1])])
    ov, _ = check_overlaps(pkg, ctx, flat, [0, 0])
    assert ov["n_candidates"] == 1 and ov["n_pairs"] == 0
    dev, _ = check_merge(pkg, ctx, flat, [0, 0])
    assert dev["result"]["n_candidates"] == 1 and dev["result"]["n_pairs"] == 0 and list(dev["group"]) == [0, 1]


def test_labels_and_containment_threshold(pkg, ctx):
    big = sc.ell([0.3, 0.1, -0.2], [0.9, 0.7, 0.8], yaw=0.4)
    small = sc.ell([0.35, 0.15, -0.1], [0.3, 0.2, 0.25], yaw=1.1)
    objs = np.stack([big, small])
    dev, _ = check_merge(pkg, ctx, objs, [0, 1])
    assert list(dev["group"]) == [0, 1] and dev["result"]["n_candidates"] == 0
    dev, _ = check_merge(pkg, ctx, objs, [0, 1], match_labels=0)
    assert list(dev["group"]) == [0, 0] and list(dev["labels"]) == [0]
    dev, _ = check_merge(pkg, ctx, objs, [0, 0], min_contain=2.0)          # containment switched off: the IoU alone is too small
    assert list(dev["group"]) == [0, 1] and dev["result"]["n_pairs"] == 1 and dev["result"]["n_links"] == 0
    s = sc.clutter_scene(2)
    a, _ = check_overlaps(pkg, ctx, s["objs"], s["labels"], match_labels=0)
    assert a["n_candidates"] > clutter_overlaps(2)["n_candidates"]


def test_chains(pkg, ctx):
    dev, ref = check_merge(pkg, ctx, sc.chain(3), np.zeros(3, np.int32))
    assert list(ref["overlaps"]["link"]) == [True, False, True]          # A ~ B, B ~ C, A and C overlap but do not link
    assert list(dev["group"]) == [0, 0, 0] and dev["result"]["n_links"] == 2
    long = sc.chain(33)
    dev, _ = check_merge(pkg, ctx, long, np.zeros(33, np.int32))
    assert dev["result"]["n_groups"] == 1 and dev["result"]["largest_group"] == 33
    order = np.random.default_rng(3).permutation(33)          # the chain's neighbours far apart in the index: more rounds
    dev, _ = check_merge(pkg, ctx, long[order], np.zeros(33, np.int32), np.arange(33)[::-1].copy())
    assert dev["result"]["n_groups"] == 1 and dev["objs"].tobytes() == long[order][0].tobytes()


# ---- esl_map_merge --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["weights", "list", "none"])
def test_merge_planted(pkg, ctx, mode):
    s, (w, cam, obj), ref = scene_merge("planted", 0, mode)
    dev = dev_merge(pkg, ctx, s["objs"], s["labels"], w, cam, obj)
    assert_merge(dev, ref)
    assert np.array_equal(dev["group"], s["group"]) and dev["result"]["n_merged_groups"] == sc.N_COPIES
    if mode != "none":
        assert dev["result"]["n_conflicts"] == 2 * sc.N_COPIES


@pytest.mark.parametrize("seed", sc.CLUTTER_SEEDS)
@pytest.mark.parametrize("mode", ["weights", "list", "none"])
def test_merge_clutter(pkg, ctx, seed, mode):
    s, (w, cam, obj), ref = scene_merge("clutter", seed, mode)
    assert ref["result"]["n_merged_groups"] > 0 and ref["result"]["largest_group"] > 2
    assert mode == "none" or ref["result"]["n_conflicts"] > 0
    assert_merge(dev_merge(pkg, ctx, s["objs"], s["labels"], w, cam, obj), ref)


def test_merge_without_labels_matching(pkg, ctx):
    s, (w, cam, obj), ref = scene_merge("planted", 0, "list", frozen(dict(match_labels=0)))
    dev = dev_merge(pkg, ctx, s["objs"], s["labels"], w, cam, obj, match_labels=0)
    assert_merge(dev, ref)
    assert np.array_equal(dev["group"], s["group"])


def test_rewritten_list_feeds_init_quadrics(pkg, ctx):
    """the -1 convention end to end: esl_init_quadrics accepts the rewritten list as it is"""
    s, (w, cam, obj), _ = scene_merge("planted", 0, "list")
    dev = dev_merge(pkg, ctx, s["objs"], s["labels"], w, cam, obj)
    assert (dev["obs_obj"] == -1).sum() > (obj < 0).sum()
    cams = np.tile([0, 0, 0, 0, 0, 0, 1.0], (sc.PLANTED_FRAMES, 1))
    boxes = np.tile([100.0, 120.0, 300.0, 260.0], (len(cam), 1))
    N = dev["result"]["n_groups"]
    e, _, _, stats = ctx.init_quadrics(cams, N, cam, dev["obs_obj"], boxes, [500.0, 500.0, 320.0, 240.0], min_observations=0)
    assert e.shape == (N, 10) and np.array_equal(stats[:, 1], np.bincount(dev["obs_obj"][dev["obs_obj"] >= 0], minlength=N))


def test_candidate_batch(pkg, ctx):
    """every pair of 300 ellipsoids is a candidate: 44,850, more than the overlap launch has wavefronts"""
    d = sc.dense_cluster()
    ref = mr.overlaps(d["objs"], d["labels"], lattice=8)
    sc.check_conditions(ref)
    assert ref["n_candidates"] == 300 * 299 // 2 > 2048 * 4
    assert_overlaps(dev_overlaps(pkg, ctx, d["objs"], d["labels"], lattice=8), ref)
    dev = dev_merge(pkg, ctx, d["objs"], d["labels"], lattice=8)
    assert dev["result"]["n_pairs"] == ref["n_pairs"] and dev["result"]["n_links"] == int(ref["link"].sum())
    assert dev["result"]["n_groups"] == 1 and dev["objs"].tobytes() == d["objs"][0].tobytes() and list(dev["weights"]) == [300]


def test_status_3(pkg, ctx):
    s, ref0 = sc.clutter_scene(0), clutter_overlaps(0)
    L = pkg.lib.load()
    other = pkg.Context(0)
    try:
        with pytest.raises(pkg.EslError):
            dev_merge(pkg, other, s["objs"], s["labels"], lattice=3)
        before = L.esl_last_error()
        for mode in ("list", "weights", "none"):
            w = s["weights"] if mode == "weights" else None
            cam, obj = (None, None) if mode == "none" else (s["obs_cam"], s["obs_obj"])
            dev = dev_merge(pkg, other, s["objs"], s["labels"], w, cam, obj, max_pairs=ref0["n_candidates"] - 1)          # ESL_OK: no exception
            ref = mr.merge(s["objs"], s["labels"], w, cam, obj, max_pairs=ref0["n_candidates"] - 1)
            assert_merge(dev, ref)
            assert dev["result"]["status"] == 3 and dev["result"]["n_candidates"] == ref0["n_candidates"]
            assert np.array_equal(dev["new_index"], np.arange(len(s["objs"]))) and dev["objs"].tobytes() == s["objs"].tobytes()
            if obj is not None:
                assert np.array_equal(dev["obs_obj"], np.where(obj < 0, -1, obj))
        assert L.esl_last_error() == before
        ov = dev_overlaps(pkg, other, s["objs"], s["labels"], max_pairs=ref0["n_candidates"] - 1)
        assert ov["n_pairs"] == -1 and ov["n_candidates"] == ref0["n_candidates"] and len(ov["pairs"]) == 0
        dev = dev_merge(pkg, other, s["objs"], s["labels"], max_pairs=ref0["n_candidates"])          # exactly at the limit: status 0
        assert dev["result"]["status"] == 0
    finally:
        other.close()


def test_bit_identical_runs(pkg, ctx):
    s, p = sc.clutter_scene(1), sc.planted_scene()

    def both():
        a = dev_merge(pkg, ctx, s["objs"], s["labels"], None, s["obs_cam"], s["obs_obj"])
        b = dev_overlaps(pkg, ctx, s["objs"], s["labels"])
        return a, b

    def same(x, y):
        assert x.keys() == y.keys()
        for k in x:
            if isinstance(x[k], np.ndarray):
                assert x[k].tobytes() == y[k].tobytes(), k
            else:
                assert x[k] == y[k], k
    a0, b0 = both()
    a1, b1 = both()
    same(a0, a1); same(b0, b1)
    dev_merge(pkg, ctx, p["objs"], p["labels"], p["weights"], p["obs_cam"], p["obs_obj"])          # another scene in between
    dev_overlaps(pkg, ctx, sc.dense_cluster()["objs"], sc.dense_cluster()["labels"], lattice=4)
    a2, b2 = both()
    same(a0, a2); same(b0, b2)


def test_resident_form_leaves_the_states_alone(pkg, ctx):
    g, c, o, _ = pkg.synth.make_graph(12, 30, 200, seed=3)
    rng = np.random.default_rng(1)
    o = np.array(o, dtype=np.float64).reshape(-1, 10).copy()
    o[7] = o[3]; o[7, :3] += 0.01          # a duplicate in the resident map
    labels = rng.integers(0, 2, g.n_objs).astype(np.int32); labels[7] = labels[3]
    ctx.upload_graph(g); ctx.upload_states(c, o)
    c0, o0 = ctx.download_states()
    given = dev_merge(pkg, ctx, o0, labels, None, g.bbox_cam, g.bbox_obj)
    resident = dev_merge(pkg, ctx, None, labels, None, g.bbox_cam, g.bbox_obj)
    assert given["result"]["n_merged_groups"] >= 1 and given["group"][7] == given["group"][3]
    for k in given:
        if isinstance(given[k], np.ndarray):
            assert given[k].tobytes() == resident[k].tobytes(), k
        else:
            assert given[k] == resident[k], k
    ov_g, ov_r = dev_overlaps(pkg, ctx, o0, labels), dev_overlaps(pkg, ctx, None, labels)
    assert ov_g["pairs"].tobytes() == ov_r["pairs"].tobytes() and ov_g["iou"].tobytes() == ov_r["iou"].tobytes() and ov_g["n_pairs"] >= 1
    c1, o1 = ctx.download_states()
    assert c0.tobytes() == c1.tobytes() and o0.tobytes() == o1.tobytes()
    with pytest.raises(pkg.EslError, match="esl_status 2"):          # M differs from the resident graph
        dev_merge(pkg, ctx, None, labels[:-1])
    with pytest.raises(pkg.EslError, match="esl_status 2"):
        dev_overlaps(pkg, ctx, None, labels[:-1])


def test_profiling_class_4(pkg):
    cx = pkg.Context(0)
    try:
        s = sc.clutter_scene(0)
        cx.profile_enable(2)
        dev_merge(pkg, cx, s["objs"], s["labels"], None, s["obs_cam"], s["obs_obj"])
        dev_overlaps(pkg, cx, s["objs"], s["labels"])
        prof = cx.profile_get()
        assert set(prof) == {"reduce"} and prof["reduce"]["count"] >= 4 and prof["reduce"]["total_ms"] > 0
    finally:
        cx.close()


def test_errors(pkg):
    cx = pkg.Context(0)
    s = sc.clutter_scene(0)
    M = len(s["objs"])
    try:
        for fn in (dev_merge, dev_overlaps):
            with pytest.raises(pkg.EslError, match="esl_status 4"):          # a NULL source without a resident graph
                fn(pkg, cx, None, s["labels"])
            for over in (dict(lattice=3), dict(lattice=33), dict(min_iou=0.0), dict(min_iou=1.5), dict(min_iou=float("nan")),
                         dict(min_iou=-0.1), dict(min_contain=0.0), dict(min_contain=float("inf")), dict(min_contain=float("nan")),
                         dict(max_pairs=-1)):
                with pytest.raises(pkg.EslError, match="esl_status 2"):
                    fn(pkg, cx, s["objs"], s["labels"], **over)
            with pytest.raises(pkg.EslError, match="esl_status 2"):          # M > 65536
                fn(pkg, cx, np.zeros((65537, 10)), np.zeros(65537, np.int32))
        w = s["weights"].copy(); w[5] = -1
        with pytest.raises(pkg.EslError, match="esl_status 2"):
            dev_merge(pkg, cx, s["objs"], s["labels"], w)
        w = np.full(M, 2 ** 31 // M + 1, np.int32)
        with pytest.raises(pkg.EslError, match="esl_status 2"):
            dev_merge(pkg, cx, s["objs"], s["labels"], w)
        obj = s["obs_obj"].copy(); obj[3] = M
        with pytest.raises(pkg.EslError, match="esl_status 2"):
            dev_merge(pkg, cx, s["objs"], s["labels"], None, s["obs_cam"], obj)
        cam = s["obs_cam"].copy(); cam[np.nonzero(s["obs_obj"] >= 0)[0][0]] = -1
        with pytest.raises(pkg.EslError, match="esl_status 2"):
            dev_merge(pkg, cx, s["objs"], s["labels"], None, cam, s["obs_obj"])
        cam = s["obs_cam"].copy(); cam[np.nonzero(s["obs_obj"] < 0)[0][0]] = -1          # on a skipped entry it is not looked at
        dev_merge(pkg, cx, s["objs"], s["labels"], None, cam, s["obs_obj"])
        # the C-ABI itself: null pointers and negative counts
        L = pkg.lib.load()
        ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
        o2 = (ctypes.c_double * 20)(*sc.chain(2).reshape(-1)); l2 = (ctypes.c_int32 * 2)(0, 0)
        g2, n2, ml, mw = [(ctypes.c_int32 * 2)() for _ in range(4)]
        mo = (ctypes.c_double * 20)(); res = pkg.abi.EslMergeResult()
        oc, oo, out = (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)()

        def merge(ctx=cx._h, objs=o2, lab=l2, w=None, M=2, cam=oc, obj=oo, n_obs=1, group=g2, new=n2, mobj=mo, mlab=ml, mwt=mw, oout=out, r=res):
            return L.esl_map_merge(ctx, objs, lab, w, M, cam, obj, ctypes.c_int64(n_obs), None, group, new, mobj, mlab, mwt, oout,
                                   ctypes.byref(r) if r is not None else None)
        assert merge() == 0 and res.n_groups == 1 and out[0] == 0
        assert merge(oout=None) == 0          # the list only weighs
        for bad in (dict(ctx=None), dict(lab=None), dict(M=-1), dict(cam=None), dict(obj=None), dict(n_obs=-1), dict(group=None),
                    dict(new=None), dict(mobj=None), dict(mlab=None), dict(mwt=None), dict(r=None), dict(n_obs=2 ** 31)):
            assert merge(**bad) == 2, bad
        assert merge(objs=None) == 4
        pr, cn = (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 2)()
        io, co = (ctypes.c_double * 1)(), (ctypes.c_double * 1)()
        npairs, ncand = ctypes.c_int64(0), ctypes.c_int64(0)

        def overlaps(ctx=cx._h, objs=o2, lab=l2, M=2, cap=1, pairs=pr, cnt=cn, iou=io, con=co, a=npairs, b=ncand):
            return L.esl_map_overlaps(ctx, objs, lab, M, None, ctypes.c_int64(cap), pairs, cnt, iou, con,
                                      ctypes.byref(a) if a is not None else None, ctypes.byref(b) if b is not None else None)
        assert overlaps() == 0 and npairs.value == 1 and ncand.value == 1 and list(pr) == [0, 1]
        assert overlaps(cap=0, pairs=None, cnt=None, iou=None, con=None) == 0 and npairs.value == 1
        for bad in (dict(ctx=None), dict(lab=None), dict(M=-1), dict(cap=-1), dict(pairs=None), dict(cnt=None), dict(iou=None),
                    dict(con=None), dict(a=None), dict(b=None)):
            assert overlaps(**bad) == 2, bad
        assert overlaps(objs=None) == 4
    finally:
        cx.close()
