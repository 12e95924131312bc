"""esl_dense_carve_frames on the device against its numpy statement (tests/dense_carve_ref.py).

The maps are built through esl_dense_add_frames from tests/dense_carve_scenes.py (the premises the scenes rely on are asserted on the
statement alone in tests/test_dense_carve_ref.py).  Every output is an integer and is compared with np.array_equal: both sides run
identical correctly rounded operations on identical integers.  No tolerance anywhere."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_carve_ref as dcr          # noqa: E402
import dense_carve_scenes as cs        # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTS = ("vox", "carved", "obs", "depth_kept", "mask", "own")
LATE, ALL = (3, 4, 5), (0, 1, 2, 3, 4, 5)
EXTRACT = ("key", "xyz", "count", "bgr", "inst", "votes")


def sub(a, i):
    return None if a is None else a[list(i)]


def dev_build(pkg, cx, sc, frames=None, depth=None):
    cx.dense_begin(pkg.abi.default_dense_params(**sc["params"]), sc["with_color"], sc["with_inst"])
    f = range(len(sc["cams"])) if frames is None else frames
    if len(sc["cams"]) and len(f):
        d = sc["depth"] if depth is None else depth
        cx.dense_add_frames(sc["cams"][list(f)], sc["K"], sc["rows"], sc["cols"], d[list(f)], sub(sc["bgr"], f), sub(sc["inst"], f))


def dev_carve(pkg, cx, sc, obs, own, want=OUTS, vox_cap=None, **kw):
    return cx.dense_carve_frames(sc["cams"][list(obs)], sc["depth"][list(obs)], sc["cams"][list(own)], sc["depth"][list(own)], sc["K"], sc["rows"],
                                 sc["cols"], sub(sc["bgr"], own), sub(sc["inst"], own), pkg.abi.default_dense_carve_params(**kw), want=want,
                                 vox_cap=vox_cap)


def ref_carve(sc, m, obs, own, vox_cap=None, **kw):
    return dcr.carve(m, sc["cams"][list(obs)], sc["depth"][list(obs)], sc["cams"][list(own)], sc["depth"][list(own)], sc["K"], sc["rows"],
                     sc["cols"], sub(sc["bgr"], own), sub(sc["inst"], own), vox_cap=vox_cap, **kw)


def assert_same(dev, ref, outs=OUTS):
    assert dev["result"] == ref["result"]
    for k in outs:
        assert dev[k].dtype == ref[k].dtype and dev[k].shape == ref[k].shape, (k, dev[k].dtype, dev[k].shape, ref[k].dtype, ref[k].shape)
        if not np.array_equal(dev[k], ref[k]):
            bad = np.argwhere(dev[k] != ref[k])[:5]
            raise AssertionError((k, bad.tolist(), dev[k][tuple(bad[0])], ref[k][tuple(bad[0])]))


def same_bytes(a, b, outs=OUTS):
    assert a["result"] == b["result"]
    for k in outs:
        assert a[k].tobytes() == b[k].tobytes(), k


def map_bytes(cx):
    e = cx.dense_extract()
    return e["n_voxels"], tuple(e[k].tobytes() for k in EXTRACT), cx.dense_info()


def chunk_size():
    """kDcvChunk of csrc/esl_dense_carve.hpp: the observer frames of one chunk of k_dcv_observe"""
    txt = open(os.path.join(ROOT, "object-oriented-slam_amd", "csrc", "esl_dense_carve.hpp")).read()
    return int(re.search(r"constexpr int kDcvChunk = (\d+);", txt).group(1))


# ---- the ghost scenes against the statement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cs.GHOSTS))
def test_ghost_scenes(pkg, ctx, name):
    sc = cs.ghost_scene(name)
    dev_build(pkg, ctx, sc)
    before, slots = map_bytes(ctx), ctx.dense_slots()
    ref = ref_carve(sc, cs.build(sc), LATE, ALL)
    dev = dev_carve(pkg, ctx, sc, LATE, ALL)
    assert_same(dev, ref)
    assert dev["result"]["n_carved"] > 50 and dev["result"]["removed"] == dcr.ZERO_REMOVED
    assert map_bytes(ctx) == before and ctx.dense_slots() == slots          # apply = 0 leaves extract's bytes and the slots alone
    same_bytes(dev_carve(pkg, ctx, sc, LATE, ALL), dev)          # a run repeated


@pytest.mark.parametrize("window", [0, 1, 2, 4])
def test_windows(pkg, ctx, window):
    sc = cs.ghost_scene("ghost_odd")
    dev_build(pkg, ctx, sc)
    assert_same(dev_carve(pkg, ctx, sc, ALL, ALL, window=window), ref_carve(sc, cs.build(sc), ALL, ALL, window=window))


@pytest.mark.parametrize("name", cs.EXACT)
def test_exact_scenes(pkg, ctx, name):
    e = cs.exact_scene(name)
    dev_build(pkg, ctx, e["map"])
    m = cs.build(e["map"])
    same = (tuple(e["K"]), e["rows"], e["cols"]) == (tuple(e["map"]["K"]), 1, 1)          # the owners share the observers' K and image size
    own = (e["map"]["cams"], e["map"]["depth"]) if same else (None, None)
    ref = dcr.carve(m, e["cams_obs"], e["depth_obs"], own[0], own[1], e["K"], e["rows"], e["cols"], **e["params"])
    dev = ctx.dense_carve_frames(e["cams_obs"], e["depth_obs"], own[0], own[1], e["K"], e["rows"], e["cols"],
                                 params=pkg.abi.default_dense_carve_params(**e["params"]))
    assert_same(dev, ref)
    # one observer per call: the classes themselves, held to the hand-made ones
    want = cs.exact_classes(name, m)
    for f in range(len(e["cams_obs"])):
        one = ctx.dense_carve_frames(e["cams_obs"][f:f + 1], e["depth_obs"][f:f + 1], None, None, e["K"], e["rows"], e["cols"],
                                     params=pkg.abi.default_dense_carve_params(**e["params"]), want=("vox", "obs"))
        cls = np.where(one["vox"].sum(axis=1) > 0, one["vox"].argmax(axis=1), -1)
        hand = np.where(want[f] <= dcr.NODATA, want[f], -1)
        assert np.array_equal(cls, hand), (name, f)
        assert one["obs"][0, 1] == (want[f] == dcr.DEPTH_OUT).sum() and one["obs"][0, 2] == (want[f] == dcr.OUTSIDE).sum()


# ---- independence of batching and order ---------------------------------------------------------------------------------------------------
def test_batching_and_order(pkg, ctx):
    sc = cs.ghost_scene("ghost")
    dev_build(pkg, ctx, sc)
    whole = dev_carve(pkg, ctx, sc, ALL, ALL)
    assert_same(whole, ref_carve(sc, cs.build(sc), ALL, ALL))
    # F_obs calls of one frame: the counts add, the verdict follows from the summed counts
    parts = [dev_carve(pkg, ctx, sc, (f,), ALL, want=("vox", "obs")) for f in ALL]
    vox = sum(p["vox"] for p in parts)
    assert np.array_equal(vox, whole["vox"]) and np.array_equal(np.concatenate([p["obs"] for p in parts]), whole["obs"])
    assert np.array_equal(dcr.verdict(vox, dcr.DEFAULTS).astype(np.uint8), whole["carved"])
    # any observer order: the voxels' outputs are the same bytes, the frames' rows permuted
    perm = (4, 0, 5, 2, 1, 3)
    po = dev_carve(pkg, ctx, sc, perm, ALL)
    same_bytes(po, whole, ("vox", "carved", "depth_kept", "mask", "own"))
    assert np.array_equal(po["obs"], whole["obs"][list(perm)])
    # any owner order: the owners' outputs permuted
    pw = dev_carve(pkg, ctx, sc, ALL, perm)
    same_bytes(pw, whole, ("vox", "carved", "obs"))
    for k in ("depth_kept", "mask", "own"):
        assert np.array_equal(pw[k], whole[k][list(perm)]), k


def test_chunk_boundary(pkg, ctx):
    ch = chunk_size()
    sc = cs.ghost_scene("ghost_odd")
    dev_build(pkg, ctx, sc)
    m = cs.build(sc)
    for F in (ch - 1, ch, ch + 1):
        obs = [(3, 4, 5, 0, 4, 1, 5)[i % 7] for i in range(F)]
        assert_same(dev_carve(pkg, ctx, sc, obs, ALL), ref_carve(sc, m, obs, ALL))


# ---- apply --------------------------------------------------------------------------------------------------------------------------------
def test_apply_is_the_map_of_the_kept_images(pkg, ctx):
    sc = cs.ghost_scene("ghost_labelled")
    ground = (0.0, 0.0, 1.0, -float(cs.das.LO[2]))
    OP = pkg.abi.default_dense_obj_params(min_component=10)
    PP = pkg.abi.default_dense_plane_params(min_inliers=200, up=(0.0, 0.0, 1.0))

    def views(cx):
        ob, pl = cx.dense_objects(2, ground, OP), cx.dense_planes(PP)
        return (map_bytes(cx), ob["result"], ob["objs"].tobytes(), ob["stats"].tobytes(), ob["voxel_comp"].tobytes(), pl["result"],
                pl["planes"].tobytes(), pl["stats"].tobytes(), pl["voxel_plane"].tobytes(), pl["ground"].tobytes())
    dev_build(pkg, ctx, sc)
    m = cs.build(sc)
    n0 = ctx.dense_info()["n_voxels"]
    ref = ref_carve(sc, m, LATE, ALL, apply=1)
    dev = dev_carve(pkg, ctx, sc, LATE, ALL, apply=1)
    assert_same(dev, ref)
    res = dev["result"]
    assert res["status"] == 0 and res["n_carved"] > 50 and res["removed"]["n_missing"] == 0 and res["removed"]["n_emptied"] == res["n_carved"]
    assert res["removed"]["n_used"] == res["samples_carved"] and ctx.dense_info()["n_voxels"] == n0 - res["n_carved"]
    assert ctx.dense_slots()["dead_voxels"] == res["n_carved"] and ctx.dense_slots() == m.slots()
    carved_map = views(ctx)
    assert ctx.dense_objects(2, ground, OP)["stats"].size and carved_map[0][0] == m.extract()["n_voxels"]
    # a second carve finds nothing; an owner moves with its kept image and the map stays consistent; a purge drops the dead slots
    again = dev_carve(pkg, ctx, sc, LATE, ALL, apply=1)
    assert again["result"]["n_carved"] == 0 and again["result"]["samples_carved"] == 0 and again["result"]["status"] == 0
    kept = dev["depth_kept"]
    new = sc["cams"][0:1].copy(); new[0, 0] += 0.125
    mv = ctx.dense_move_frames(sc["cams"][0:1], new, sc["K"], sc["rows"], sc["cols"], kept[0:1], sc["bgr"][0:1], sc["inst"][0:1])
    assert mv["removed"]["status"] == 0 and mv["removed"]["n_missing"] == 0 and mv["added"]["status"] == 0 and ctx.dense_info()["status"] == 0
    back = ctx.dense_move_frames(new, sc["cams"][0:1], sc["K"], sc["rows"], sc["cols"], kept[0:1], sc["bgr"][0:1], sc["inst"][0:1])
    assert back["added"]["status"] == 0 and views(ctx) == carved_map
    b, a = ctx.dense_purge()
    assert b["dead_voxels"] >= res["n_carved"] and a["dead_voxels"] == 0 and views(ctx) == carved_map
    final = dev_carve(pkg, ctx, sc, LATE, ALL, apply=1)
    assert final["result"]["n_carved"] == 0 and final["result"]["status"] == 0
    # the map built from scratch from the kept images: the same bytes in extract (xyz included), objects, planes and info
    dev_build(pkg, ctx, sc, depth=kept)
    assert views(ctx) == carved_map


def test_half_the_owners(pkg, ctx):
    sc = cs.ghost_scene("ghost_stride2")
    dev_build(pkg, ctx, sc)
    m = cs.build(sc)
    dev = dev_carve(pkg, ctx, sc, LATE, (0, 2, 4), apply=1)
    assert_same(dev, ref_carve(sc, m, LATE, (0, 2, 4), apply=1))
    assert 0 < dev["result"]["removed"]["n_emptied"] < dev["result"]["n_carved"] and ctx.dense_slots() == m.slots()
    e, r = ctx.dense_extract(), m.extract()
    assert e["n_voxels"] == r["n_voxels"] and all(e[k].tobytes() == r[k].tobytes() for k in EXTRACT)


# ---- edge inputs ---------------------------------------------------------------------------------------------------------------------------
def test_edge_inputs(pkg, ctx):
    sc = cs.ghost_scene("ghost")
    dev_build(pkg, ctx, sc)
    m = cs.build(sc)
    full = dev_carve(pkg, ctx, sc, LATE, ALL)
    before = map_bytes(ctx)
    for cap in (0, 100, full["result"]["n_voxels"] + 5):          # vox_cap below and above n_voxels
        d = dev_carve(pkg, ctx, sc, LATE, ALL, vox_cap=cap)
        assert_same(d, ref_carve(sc, m, LATE, ALL, vox_cap=cap))
        assert len(d["vox"]) == len(d["carved"]) == min(cap, full["result"]["n_voxels"])
    for k in OUTS:          # one output at a time, then none
        d = dev_carve(pkg, ctx, sc, LATE, ALL, want=(k,))
        assert sorted(d) == sorted([k, "result"]) and d[k].tobytes() == full[k].tobytes() and d["result"] == full["result"]
    assert dev_carve(pkg, ctx, sc, LATE, ALL, want=()) == dict(result=full["result"])
    none = dev_carve(pkg, ctx, sc, (), ALL)          # F_obs = 0: nothing is seen, nothing carved
    assert_same(none, ref_carve(sc, m, (), ALL))
    assert none["result"]["n_tested"] == 0 and none["result"]["n_carved"] == 0 and none["obs"].shape == (0, 8) and (none["mask"] == 0).all()
    assert_same(dev_carve(pkg, ctx, sc, LATE, ()), ref_carve(sc, m, LATE, ()))          # F_own = 0
    assert_same(dev_carve(pkg, ctx, sc, (), (), apply=1), ref_carve(sc, m, (), (), apply=1))
    blind = dict(sc, depth=np.zeros_like(sc["depth"]))          # an all-zero observer image: every observation no data
    d = ctx.dense_carve_frames(sc["cams"][3:], blind["depth"][3:], sc["cams"], sc["depth"], sc["K"], sc["rows"], sc["cols"])
    assert (d["vox"][:, :3] == 0).all() and (d["obs"][:, 3:6] == 0).all() and (d["obs"][:, 6] == d["obs"][:, 0]).all() and d["obs"][:, 0].sum() > 0
    assert d["result"]["n_carved"] == 0 and d["result"]["n_tested"] == 0 and d["depth_kept"].tobytes() == sc["depth"].tobytes()
    assert map_bytes(ctx) == before
    # a warm call of the same shape allocates nothing
    warm = ctx.dense_allocs()
    same_bytes(dev_carve(pkg, ctx, sc, LATE, ALL), full)
    assert ctx.dense_allocs() == warm
    # the empty map
    dev_build(pkg, ctx, sc, frames=())
    d = dev_carve(pkg, ctx, sc, LATE, ALL)
    assert_same(d, ref_carve(sc, cs.build(sc, frames=[]), LATE, ALL))
    assert d["result"]["n_voxels"] == 0 and (d["own"][:, 1] == 0).all() and (d["own"][:, 3] == d["own"][:, 0]).all()


def raw_call(pkg, cx, a):
    """esl_dense_carve_frames through ctypes alone; a: dict of the arguments (arrays or None) -> (rc, result dict)"""
    L = pkg.lib.load()
    T = dict(cams_obs=ctypes.c_double, depth_obs=ctypes.c_uint16, cams_own=ctypes.c_double, depth_own=ctypes.c_uint16, bgr_own=ctypes.c_uint8,
             inst_own=ctypes.c_int32, K=ctypes.c_double, vox=ctypes.c_int32, carved=ctypes.c_uint8, obs=ctypes.c_int32,
             depth_kept=ctypes.c_uint16, mask=ctypes.c_uint8, own=ctypes.c_int32)
    DT = dict(cams_obs=np.float64, depth_obs=np.uint16, cams_own=np.float64, depth_own=np.uint16, bgr_own=np.uint8, inst_own=np.int32, K=np.float64)
    keep = {k: np.ascontiguousarray(a[k], dtype=DT[k]) for k in DT if a.get(k) is not None}

    def ptr(k):
        v = keep.get(k, a.get(k))
        return None if v is None else v.ctypes.data_as(ctypes.POINTER(T[k]))
    res = pkg.abi.EslDenseCarveResult()
    ctypes.memset(ctypes.byref(res), 7, ctypes.sizeof(res))
    rc = L.esl_dense_carve_frames(cx._h if cx is not None else None, ptr("cams_obs"), a["F_obs"], ptr("depth_obs"), ptr("cams_own"), a["F_own"],
                                  ptr("depth_own"), ptr("bgr_own"), ptr("inst_own"), ptr("K"), a["rows"], a["cols"],
                                  None if a.get("p") is None else ctypes.byref(a["p"]), a.get("vox_cap", 0), ptr("vox"), ptr("carved"), ptr("obs"),
                                  ptr("depth_kept"), ptr("mask"), ptr("own"), ctypes.byref(res) if a.get("out", True) else None)
    return rc, res.as_dict()


def test_status_3_writes_nothing(pkg, ctx):
    sc = cs.full_scene()
    dev_build(pkg, ctx, sc)
    assert ctx.dense_info()["status"] == 3
    e = cs.exact_scene("tol")
    bufs = dict(vox=np.full((9, 4), 77, np.int32), carved=np.full(9, 7, np.uint8), obs=np.full((5, 8), 77, np.int32),
                depth_kept=np.full((2, 1, 1), 77, np.uint16), mask=np.full((2, 1, 1), 7, np.uint8), own=np.full((2, 4), 77, np.int32))
    rc, res = raw_call(pkg, ctx, dict(bufs, cams_obs=e["cams_obs"], F_obs=5, depth_obs=e["depth_obs"], cams_own=sc["cams"][:2], F_own=2,
                                      depth_own=sc["depth"][:2], K=e["K"], rows=1, cols=1, vox_cap=9))
    want = dcr.carve(cs.build(sc), e["cams_obs"], e["depth_obs"], sc["cams"][:2], sc["depth"][:2], e["K"], 1, 1)["result"]
    assert rc == 0 and res == want and res["status"] == 3 and res["n_voxels"] == -1
    assert all((bufs[k] == 77).all() for k in ("vox", "obs", "depth_kept", "own")) and (bufs["carved"] == 7).all() and (bufs["mask"] == 7).all()


# ---- the resident cameras and the errors ---------------------------------------------------------------------------------------------------
def test_resident_cameras_and_errors(pkg):
    g, c, o, _ = pkg.synth.make_graph(5, 8, 40, seed=3)
    sc = cs.ghost_scene("ghost_labelled")
    cx = pkg.Context(0)
    P = pkg.abi.default_dense_carve_params
    who = "esl_dense_carve_frames"
    try:
        with pytest.raises(pkg.EslError, match=f"esl_status 4: {who}: no esl_dense_begin before"):
            dev_carve(pkg, cx, sc, LATE, ALL)
        dev_build(pkg, cx, sc)
        before, slots = map_bytes(cx), cx.dense_slots()
        L = pkg.lib.load()
        base = dict(cams_obs=sc["cams"][3:], F_obs=3, depth_obs=sc["depth"][3:], cams_own=sc["cams"], F_own=6, depth_own=sc["depth"],
                    bgr_own=sc["bgr"], inst_own=sc["inst"], K=sc["K"], rows=sc["rows"], cols=sc["cols"])

        def refused(status, what, ctx_=cx, **kw):
            rc, _ = raw_call(pkg, ctx_, dict(base, **kw))
            msg = L.esl_last_error().decode()
            assert rc == status and msg.startswith(who + ": ") and what in msg, (rc, msg)
        refused(4, "NULL cams needs a resident graph with states", cams_obs=None)
        cx.upload_graph(g); cx.upload_states(c, o)
        c0, _ = cx.download_states()
        F = len(c0)
        depth = np.stack([sc["depth"][3 + f % 3] for f in range(F)])
        given = cx.dense_carve_frames(c0, depth, sc["cams"], sc["depth"], sc["K"], sc["rows"], sc["cols"])
        res = cx.dense_carve_frames(None, depth, sc["cams"], sc["depth"], sc["K"], sc["rows"], sc["cols"])          # the resident states
        same_bytes(res, given)
        assert_same(given, dcr.carve(cs.build(sc), c0, depth, sc["cams"], sc["depth"], sc["K"], sc["rows"], sc["cols"]))
        refused(2, "F differs from the resident graph's n_cams", cams_obs=None, F_obs=F - 1)
        refused(2, "null ctx", ctx_=None)
        refused(2, "null out", out=False)
        refused(2, "negative F_obs", F_obs=-1); refused(2, "negative F_own", F_own=-1)
        refused(2, "null K", K=None)
        refused(2, "rows", rows=0); refused(2, "cols", cols=16385)
        refused(2, "fx", K=(0.0, 60.0, 1.0, 1.0)); refused(2, "fy", K=(60.0, np.inf, 1.0, 1.0))
        refused(2, "negative vox_cap", vox_cap=-1)
        refused(2, "depth_scale", p=P(depth_scale=0.0)); refused(2, "depth_min", p=P(depth_min=-1.0)); refused(2, "depth_max", p=P(depth_max=np.nan))
        refused(2, "depth_tol", p=P(depth_tol=np.nan)); refused(2, "depth_min > depth_max", p=P(depth_min=2.0, depth_max=1.0))
        refused(2, "depth_max > 4095", p=P(depth_max=4096.0))
        refused(2, "window", p=P(window=-1)); refused(2, "window", p=P(window=5))
        refused(2, "min_through", p=P(min_through=0)); refused(2, "through_per_agree", p=P(through_per_agree=-1))
        refused(2, "apply", p=P(apply=2))
        refused(2, "F_obs > 65535", F_obs=65536)
        refused(2, "null depth_obs", depth_obs=None); refused(2, "null cams_own", cams_own=None); refused(2, "null depth_own", depth_own=None)
        refused(4, "null bgr_own", bgr_own=None, p=P(apply=1)); refused(4, "null inst_own", inst_own=None, p=P(apply=1))
        bad = sc["cams"].copy(); bad[4, 3:] = 0
        refused(2, "a pose", cams_obs=bad[3:]); refused(2, "a pose", cams_own=bad)
        refused(2, "2^31", F_obs=0, F_own=8, cams_own=np.tile(sc["cams"][:1], (8, 1)), rows=16384, cols=16384, p=P(apply=1))
        # every refused call left the map alone; bgr / inst are not read without apply; the last valid values pass
        assert map_bytes(cx) == before and cx.dense_slots() == slots
        ok = cx.dense_carve_frames(sc["cams"][3:], sc["depth"][3:], sc["cams"], sc["depth"], sc["K"], sc["rows"], sc["cols"],
                                   params=P(window=4, depth_max=4095.0, through_per_agree=0, min_through=1))
        assert_same(ok, ref_carve(dict(sc, bgr=None, inst=None), cs.build(sc), LATE, ALL, window=4, depth_max=4095.0, through_per_agree=0, min_through=1))
        cx.dense_end()
        with pytest.raises(pkg.EslError, match=f"esl_status 4: {who}: no esl_dense_begin before"):
            dev_carve(pkg, cx, sc, LATE, ALL)
    finally:
        cx.close()


# ---- the refusal ladder: every argument wrong at once, repaired one rung at a time, in the entry's order ----------------------------------------
def test_refusal_ladder(pkg):
    """esl_dense_carve_frames with every argument wrong at once: the status and the whole text of the first refusal, that argument
    repaired, the next refusal, through the entry's sequence.  No map until "no esl_dense_begin before" has come out, then a map of
    one 4 x 4 frame; no kernel of the entry runs until the last call."""
    who = "esl_dense_carve_frames"
    P = pkg.abi.default_dense_carve_params
    L = pkg.lib.load()
    good = np.array([[0, 0, 0, 0, 0, 0, 1.0]] * 8)
    bad = good.copy(); bad[5, 3:] = 0
    depth, bgr, inst = np.full((1, 4, 4), 5000, np.uint16), np.full((1, 4, 4, 3), 9, np.uint8), np.zeros((1, 4, 4), np.int32)
    K = (60.0, 60.0, 1.5, 1.5)
    a = dict(cx=None, out=False, cams_obs=None, F_obs=-1, depth_obs=None, cams_own=None, F_own=-1, depth_own=None, bgr_own=None, inst_own=None,
             K=None, rows=0, cols=16385, vox_cap=-1)          # every argument wrong
    p = dict(depth_scale=0.0, depth_min=-1.0, depth_max=np.nan, depth_tol=np.nan, window=5, min_through=0, through_per_agree=-1, apply=2)
    ladder = [          # (status, text, the repair of an argument or (in a tuple) of a parameter); 16384 x 16384 x 8 owners hold 2^31 samples
        (2, "null ctx", "ctx"),
        (2, "null out", dict(out=True)),
        (2, "negative F_obs", dict(F_obs=65536)),
        (2, "negative F_own", dict(F_own=8)),
        (2, "null K", dict(K=(0.0, np.inf, 1.5, 1.5))),
        (2, "rows < 1 or > 16384", dict(rows=16384)),
        (2, "cols < 1 or > 16384", dict(cols=16384)),
        (2, "fx not finite or <= 0", dict(K=(60.0, np.inf, 1.5, 1.5))),
        (2, "fy not finite or <= 0", dict(K=K)),
        (2, "negative vox_cap", dict(vox_cap=0)),
        (2, "depth_scale not finite or <= 0", (dict(depth_scale=5000.0),)),
        (2, "depth_min not finite or negative", (dict(depth_min=5000.0),)),
        (2, "depth_max not finite or negative", (dict(depth_max=4096.0),)),
        (2, "depth_tol not finite or negative", (dict(depth_tol=0.05),)),
        (2, "depth_min > depth_max", (dict(depth_min=0.1),)),
        (2, "depth_max > 4095", (dict(depth_max=4095.0),)),
        (2, "window outside 0 .. 4", (dict(window=4),)),
        (2, "min_through < 1", (dict(min_through=1),)),
        (2, "negative through_per_agree", (dict(through_per_agree=0),)),
        (2, "apply not 0 or 1", (dict(apply=1),)),
        (2, "F_obs > 65535", dict(F_obs=1)),
        (2, "null depth_obs", dict(depth_obs=depth)),
        (2, "null cams_own", dict(cams_own=bad)),
        (2, "null depth_own", dict(depth_own=depth)),
        (4, "no esl_dense_begin before", "map"),
        (4, "null bgr_own on a map begun with colour", dict(bgr_own=bgr)),
        (4, "null inst_own on a map begun with labels", dict(inst_own=inst)),
        (4, "NULL cams needs a resident graph with states", dict(cams_obs=bad[5:6])),
        (2, "a pose with a non-finite number or a quaternion of norm 0", dict(cams_obs=good[:1])),
        (2, "a pose with a non-finite number or a quaternion of norm 0", dict(cams_own=good)),
        (2, "more samples than a map holds: 2^31", dict(rows=4, cols=4, F_own=1)),
    ]
    cx = pkg.Context(0)
    try:
        for status, text, repair in ladder:
            rc, _ = raw_call(pkg, a["cx"], dict(a, p=P(**p)))
            assert (rc, L.esl_last_error().decode()) == (status, f"{who}: {text}")
            if repair == "ctx":
                a["cx"] = cx
            elif repair == "map":
                cx.dense_begin()
                cx.dense_add_frames(good[:1], K, 4, 4, depth, bgr, inst)
                before = cx.dense_info()
                assert before["n_samples"] == 16 and before["status"] == 0
            elif isinstance(repair, tuple):
                p.update(repair[0])
            else:
                a.update(repair)
        assert cx.dense_info() == before          # every refused call left the map alone
        rc, res = raw_call(pkg, a["cx"], dict(a, p=P(**p)))
        # the one observer agrees with what the one owner added: nothing is carved, the removal of step C6 takes no sample
        assert rc == 0 and res["status"] == 0 and res["n_voxels"] > 0 and res["n_carved"] == 0 and cx.dense_info() == before
    finally:
        cx.close()
