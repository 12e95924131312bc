"""esl_dense_render on the device against its numpy statement (tests/dense_render_ref.py).

The maps are placed exactly through esl_dense_add_frames (tests/dense_render_scenes.py; the premises the scenes rely on are asserted on
the statement alone in tests/test_dense_render_ref.py).  Every integer output is compared with np.array_equal and depth with
equal_nan=True and otherwise exactly: both sides run identical correctly rounded operations on identical integers."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_render_ref as drr         # noqa: E402
import dense_render_scenes as rs       # noqa: E402

pytestmark = pytest.mark.gpu

OUTS = ("depth", "voxel", "bgr", "inst", "frame", "vox")


def dev_build(pkg, cx, name):
    s = rs.scene(name)
    cx.dense_begin(pkg.abi.default_dense_params(**s["params"]), True, True)
    fr = s["frames"]
    if fr is not None:
        cx.dense_add_frames(fr["cams"], fr["K"], fr["rows"], fr["cols"], fr["depth"], fr["bgr"], fr["inst"])
        for f in s.get("remove") or []:
            cx.dense_remove_frames(fr["cams"][f:f + 1], fr["K"], fr["rows"], fr["cols"], fr["depth"][f:f + 1], fr["bgr"][f:f + 1], fr["inst"][f:f + 1])


def ref_of(name, vox_cap=None, **kw):
    c = rs.case(name)
    return drr.render(rs.extract(c["map"]), rs.leaf_of(c["map"]), c["cams"], c["K"], c["rows"], c["cols"], c["depth_meas"], vox_cap=vox_cap,
                      **dict(c["params"], **kw))


def dev_of(pkg, cx, name, vox_cap=None, want=OUTS, frames=None, **kw):
    c = rs.case(name)
    f = slice(None) if frames is None else frames
    meas = None if c["depth_meas"] is None else c["depth_meas"][f]
    return cx.dense_render(c["cams"][f], c["K"], c["rows"], c["cols"], meas, pkg.abi.default_dense_render_params(**dict(c["params"], **kw)),
                           want=want, vox_cap=vox_cap)


def assert_same(dev, ref, outs=OUTS):
    assert dev["result"] == ref["result"]
    for k in outs:
        assert dev[k].dtype == ref[k].dtype and dev[k].shape == ref[k].shape, (k, dev[k].dtype, dev[k].shape, ref[k].shape)
        if not np.array_equal(dev[k], ref[k], equal_nan=(k == "depth")):
            bad = np.argwhere(~((dev[k] == ref[k]) | ((dev[k] != dev[k]) & (ref[k] != ref[k]))))[:5]
            raise AssertionError((k, bad.tolist(), dev[k][tuple(bad[0])], ref[k][tuple(bad[0])]))


def same_bytes(a, b, outs=OUTS):
    for k in outs:
        assert a[k].tobytes() == b[k].tobytes(), k


def check(pkg, cx, name, build=True, **kw):
    if build:
        dev_build(pkg, cx, rs.case(name)["map"])
    dev = dev_of(pkg, cx, name, **kw)
    assert_same(dev, ref_of(name, **kw))
    return dev


# ---- known answers, footprints and culls --------------------------------------------------------------------------------------------------
def test_known_answers(pkg, ctx):
    dev_build(pkg, ctx, "probe")
    d = check(pkg, ctx, "axis", build=False)
    assert (d["voxel"][0] == 4).sum() == 25 and d["depth"][0, 24, 32] == 1.0 and (d["voxel"][0] == 5).sum() == 0          # the nearer of one ray
    assert (d["voxel"][1] == 4).sum() == 9 and d["depth"][1, 24, 32] == 2.0
    assert sorted(set(np.nonzero(d["voxel"][0] == 8)[1].tolist())) == [62, 63] and sorted(set(np.nonzero(d["voxel"][0] == 2)[0].tolist())) == [0, 1, 2]
    for name in ("half_pixel", "radius0", "radius1", "radius8", "footprint0", "footprint15", "depth_max", "depth_min_exact", "nonfinite"):
        check(pkg, ctx, name, build=False)
    d = check(pkg, ctx, "half_pixel", build=False, footprint=0.0)
    assert np.argwhere(d["voxel"][0] == 4).tolist() == [[24, 32]]          # u + 0.5 an exact integer: the upper pixel


def test_zq_tie(pkg, ctx):
    d = check(pkg, ctx, "tie")
    assert (d["voxel"][0, 22:27, 33:35] == 0).all() and (d["depth"][0, 22:27, 33:35] == 1.0 + 2.0 ** -25).all() and d["depth"][0, 24, 35] == 1.0


def test_tolerance_boundary(pkg, ctx):
    d = check(pkg, ctx, "tol")
    assert d["frame"][:, 4:].tolist() == [[25, 0, 0, 0], [0, 0, 25, 0], [25, 0, 0, 0], [0, 25, 0, 0], [0, 0, 0, 25]]


def test_min_count(pkg, ctx):
    d = check(pkg, ctx, "min_count2")
    assert d["result"]["n_small"] == 2
    check(pkg, ctx, "min_count2", build=False, min_count=3)


# ---- the room ------------------------------------------------------------------------------------------------------------------------------
def test_room_chunks_and_splits(pkg, ctx):
    dev_build(pkg, ctx, "room")
    a0 = ctx.dense_allocs()
    d = check(pkg, ctx, "room", build=False)
    assert ((d["voxel"] >= 0).sum(axis=(1, 2)) > 48 * 64 // 2).all()
    s = check(pkg, ctx, "room_shift", build=False)
    assert (s["frame"][1, 4:] > 0).all() and (s["frame"][:, 4:].sum(axis=1) == s["frame"][:, 3]).all()
    assert s["vox"].sum(axis=0).tolist() == s["frame"][:, 3:7].sum(axis=0).tolist()
    warm = ctx.dense_allocs()
    assert warm[0] > a0[0]
    again = dev_of(pkg, ctx, "room_shift")          # a warm call of the same shape: the same bytes, no allocation
    assert ctx.dense_allocs() == warm and again["result"] == s["result"]
    same_bytes(again, s)
    # one frame per chunk against the default: the same bytes
    one = check(pkg, ctx, "room_shift", build=False, zbuf_bytes=8 * 48 * 64)
    assert one["result"]["n_chunks"] == 3 and s["result"]["n_chunks"] == 1
    same_bytes(one, s)
    # F calls of one frame: the same images, the per-voxel counts add up
    parts = [dev_of(pkg, ctx, "room_shift", frames=slice(f, f + 1)) for f in range(3)]
    for k in ("depth", "voxel", "bgr", "inst", "frame"):
        assert np.concatenate([p[k] for p in parts]).tobytes() == s[k].tobytes(), k
    assert np.array_equal(sum(p["vox"] for p in parts), s["vox"])
    # without a measured depth the comparison counts are zero, the images the same
    n = check(pkg, ctx, "room", build=False, vox_cap=100)
    assert len(n["vox"]) == 100
    c = rs.case("room")
    bare = ctx.dense_render(c["cams"], c["K"], c["rows"], c["cols"], None)
    assert (bare["frame"][:, 4:] == 0).all() and (bare["vox"][:, 1:] == 0).all() and bare["voxel"].tobytes() == d["voxel"].tobytes()
    assert np.array_equal(bare["frame"][:, :4], d["frame"][:, :4]) and np.array_equal(bare["vox"][:, 0], d["vox"][:, 0])
    # the call left the map alone, and its indices are dense_extract's
    e = ctx.dense_extract()
    ext = rs.extract("room")
    assert e["n_voxels"] == ext["n_voxels"] and e["xyz"].tobytes() == ext["xyz"].tobytes() and np.array_equal(e["inst"], ext["inst"])


def test_after_remove_frames(pkg, ctx):
    d = check(pkg, ctx, "removed")
    e = ctx.dense_extract()
    assert e["n_voxels"] == d["result"]["n_voxels"] < rs.extract("room")["n_voxels"]
    has = d["voxel"] >= 0
    assert np.array_equal(d["inst"][has], e["inst"][d["voxel"][has]]) and np.array_equal(d["bgr"][has], e["bgr"][d["voxel"][has]])


def test_overdraw_twice(pkg, ctx):
    a = check(pkg, ctx, "overdraw")
    b = dev_of(pkg, ctx, "overdraw")
    assert a["result"] == b["result"] and (a["frame"][:, 3] <= 40).all()
    same_bytes(a, b)


# ---- list lengths, caps, single outputs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rs.LIST_LENGTHS)
def test_list_lengths(pkg, ctx, n):
    check(pkg, ctx, f"grid{n}")


def test_caps_and_single_outputs(pkg, ctx):
    full = check(pkg, ctx, "grid65")
    for cap in (0, 10, 65, 100):
        d = check(pkg, ctx, "grid65", build=False, vox_cap=cap)
        assert len(d["vox"]) == min(cap, 65)
    for k in OUTS:
        d = dev_of(pkg, ctx, "grid65", want=(k,))
        assert sorted(d) == sorted([k, "result"]) and d[k].tobytes() == full[k].tobytes() and d["result"] == full["result"]
    d = dev_of(pkg, ctx, "grid65", want=())
    assert d == dict(result=full["result"])
    c = rs.case("grid65")
    none = ctx.dense_render(np.zeros((0, 7)), c["K"], c["rows"], c["cols"])          # F = 0
    assert none["result"] == dict(status=0, n_voxels=65, n_small=0, n_chunks=0) and none["depth"].shape == (0, 48, 64) and none["vox"].tolist() == [[0] * 4] * 65


# ---- an invalid map -----------------------------------------------------------------------------------------------------------------------
def raw_call(pkg, cx, cams, F, K, rows, cols, meas=None, p=None, bufs=None, vox_cap=0, out=True):
    """esl_dense_render through ctypes alone; bufs: dict of preallocated arrays -> (rc, result)"""
    L = pkg.lib.load()
    dp, ip, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
    bufs = bufs or {}

    def ptr(k, t):
        return bufs[k].ctypes.data_as(t) if k in bufs else None
    cams = None if cams is None else np.ascontiguousarray(cams, dtype=np.float64)
    Kc = None if K is None else np.ascontiguousarray(K, dtype=np.float64)
    res = pkg.abi.EslDenseRenderResult(7, 7, 7, 7)
    rc = L.esl_dense_render(cx._h if cx is not None else None, None if cams is None else cams.ctypes.data_as(dp), F,
                            None if Kc is None else Kc.ctypes.data_as(dp), rows, cols,
                            None if meas is None else meas.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                            None if p is None else ctypes.byref(p), ptr("depth", dp), ptr("voxel", ip), ptr("bgr", bp), ptr("inst", ip),
                            ptr("frame", ip), vox_cap, ptr("vox", ip), ctypes.byref(res) if out else None)
    return rc, res.as_dict()


def test_status_3_writes_nothing(pkg, ctx):
    dev_build(pkg, ctx, "full")
    assert ctx.dense_info()["status"] == 3
    c = rs.case("axis")
    bufs = dict(depth=np.full((2, 48, 64), 7.5), voxel=np.full((2, 48, 64), 77, np.int32), bgr=np.full((2, 48, 64, 3), 7, np.uint8),
                inst=np.full((2, 48, 64), 77, np.int32), frame=np.full((2, 8), 77, np.int32), vox=np.full((9, 4), 77, np.int32))
    rc, res = raw_call(pkg, ctx, c["cams"], 2, c["K"], 48, 64, bufs=bufs, vox_cap=9)
    assert rc == 0 and res == dict(status=3, n_voxels=-1, n_small=0, n_chunks=0)
    assert (bufs["depth"] == 7.5).all() and (bufs["bgr"] == 7).all() and all((bufs[k] == 77).all() for k in ("voxel", "inst", "frame", "vox"))
    assert ref_of("axis")["result"]["status"] == 0 and drr.render(rs.extract("full"), rs.LEAF, c["cams"], c["K"], 48, 64)["result"] == res


# ---- the resident cameras and the errors ---------------------------------------------------------------------------------------------------
def test_resident_cameras_and_errors(pkg):
    g, c, o, _ = pkg.synth.make_graph(5, 8, 40, seed=3)
    s = rs.scene("room")
    fr = s["frames"]
    cx = pkg.Context(0)
    P = pkg.abi.default_dense_render_params
    try:
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_render: no esl_dense_begin before"):
            cx.dense_render(fr["cams"], fr["K"], 48, 64, want=("depth",))
        dev_build(pkg, cx, "room")
        L = pkg.lib.load()

        def refused(status, what, **kw):
            a = dict(cams=fr["cams"], F=3, K=fr["K"], rows=48, cols=64)
            a.update(kw)
            rc, _ = raw_call(pkg, cx, a["cams"], a["F"], a["K"], a["rows"], a["cols"], p=a.get("p"), vox_cap=a.get("vox_cap", 0), out=a.get("out", True))
            msg = L.esl_last_error().decode()
            assert rc == status and msg.startswith("esl_dense_render: ") and what in msg, (rc, msg)
        refused(4, "NULL cams needs a resident graph with states", cams=None)
        cx.upload_graph(g); cx.upload_states(c, o)
        c0, _ = cx.download_states()
        F = len(c0)
        assert F == g.n_cams
        given = cx.dense_render(c0, fr["K"], 48, 64)
        res = cx.dense_render(None, fr["K"], 48, 64)          # the resident camera states: the same bytes as the same poses given
        assert res["result"] == given["result"] and given["result"]["n_voxels"] == rs.extract("room")["n_voxels"]
        same_bytes(res, given)
        refused(2, "F differs from the resident graph's n_cams", cams=None, F=F - 1)
        refused(2, "null out", out=False)
        refused(2, "negative F", F=-1)
        refused(2, "null K", K=None)
        refused(2, "rows", rows=0); refused(2, "cols", cols=16385)
        refused(2, "fx", K=(0.0, 60.0, 1.0, 1.0)); refused(2, "fy", K=(60.0, np.inf, 1.0, 1.0))
        refused(2, "negative vox_cap", vox_cap=-1); refused(2, "null vox_out", vox_cap=4)
        refused(2, "depth_scale", p=P(depth_scale=0.0)); refused(2, "depth_min", p=P(depth_min=-1.0)); refused(2, "depth_tol", p=P(depth_tol=np.nan))
        refused(2, "depth_min > depth_max", p=P(depth_min=2.0, depth_max=1.0)); refused(2, "depth_max > 4095", p=P(depth_max=4096.0))
        refused(2, "footprint", p=P(footprint=-0.5)); refused(2, "footprint", p=P(footprint=np.inf))
        refused(2, "max_radius", p=P(max_radius=-1)); refused(2, "max_radius", p=P(max_radius=65))
        refused(2, "min_count", p=P(min_count=0))
        refused(2, "zbuf_bytes", p=P(zbuf_bytes=8 * 48 * 64 - 1))
        bad = fr["cams"].copy(); bad[2, 3:] = 0
        refused(2, "a pose", cams=bad)
        assert raw_call(pkg, None, fr["cams"], 3, fr["K"], 48, 64)[0] == 2
        # max_radius 64, depth_max 4095 and zbuf_bytes = 8 rows cols are the last valid values; every refused call left the map alone
        ok = cx.dense_render(fr["cams"], fr["K"], 48, 64, params=P(max_radius=64, depth_max=4095.0, zbuf_bytes=8 * 48 * 64))
        assert_same(ok, drr.render(rs.extract("room"), rs.ROOM_LEAF, fr["cams"], fr["K"], 48, 64, max_radius=64, depth_max=4095.0, zbuf_bytes=8 * 48 * 64))
        cx.dense_end()
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_render: no esl_dense_begin before"):
            cx.dense_render(fr["cams"], fr["K"], 48, 64, want=("frame",))
    finally:
        cx.close()


# ---- the refusal ladder: every argument wrong at once, repaired one rung at a time, in the entry's order ----------------------------------------
def test_refusal_ladder(pkg):
    """esl_dense_render with every argument wrong at once: the status and the whole text of the first refusal, that argument repaired,
    the next refusal, through the entry's sequence.  No map until "no esl_dense_begin before" has come out, then a map of one 4 x 4
    frame; no kernel of the entry runs until the last call."""
    who = "esl_dense_render"
    P = pkg.abi.default_dense_render_params
    L = pkg.lib.load()
    good = np.array([[0, 0, 0, 0, 0, 0, 1.0]])
    K = (60.0, 60.0, 1.5, 1.5)
    vox = np.full((4, 4), 77, np.int32)
    a = dict(cx=None, out=False, cams=None, F=-1, K=None, rows=0, cols=16385, vox_cap=-1, bufs={})          # every argument wrong
    p = dict(depth_scale=0.0, depth_min=-1.0, depth_max=np.nan, depth_tol=np.nan, footprint=-0.5, max_radius=65, min_count=0, zbuf_bytes=127)
    ladder = [          # (status, text, the repair of an argument or (in a tuple) of a parameter)
        (2, "null ctx", "ctx"),
        (2, "null out", dict(out=True)),
        (2, "negative F", dict(F=1)),
        (2, "null K", dict(K=(0.0, np.inf, 1.5, 1.5))),
        (2, "rows < 1 or > 16384", dict(rows=4)),
        (2, "cols < 1 or > 16384", dict(cols=4)),
        (2, "fx not finite or <= 0", dict(K=(60.0, np.inf, 1.5, 1.5))),
        (2, "fy not finite or <= 0", dict(K=K)),
        (2, "negative vox_cap", dict(vox_cap=4)),
        (2, "null vox_out with vox_cap > 0", dict(bufs=dict(vox=vox))),
        (2, "depth_scale not finite or <= 0", (dict(depth_scale=5000.0),)),
        (2, "depth_min not finite or negative", (dict(depth_min=5000.0),)),
        (2, "depth_max not finite or negative", (dict(depth_max=4096.0),)),
        (2, "depth_tol not finite or negative", (dict(depth_tol=0.05),)),
        (2, "depth_min > depth_max", (dict(depth_min=0.1),)),
        (2, "depth_max > 4095", (dict(depth_max=4095.0),)),
        (2, "footprint not finite or negative", (dict(footprint=1.0),)),
        (2, "max_radius outside 0 .. 64", (dict(max_radius=64),)),
        (2, "min_count < 1", (dict(min_count=1),)),
        (2, "zbuf_bytes < 8 rows cols", (dict(zbuf_bytes=128),)),
        (4, "no esl_dense_begin before", "map"),
        (4, "NULL cams needs a resident graph with states", dict(cams=np.zeros((1, 7)))),
        (2, "a pose with a non-finite number or a quaternion of norm 0", dict(cams=good)),
    ]
    cx = pkg.Context(0)

    def call():
        return raw_call(pkg, a["cx"], a["cams"], a["F"], a["K"], a["rows"], a["cols"], p=P(**p), bufs=a["bufs"], vox_cap=a["vox_cap"], out=a["out"])
    try:
        for status, text, repair in ladder:
            rc, _ = call()
            assert (rc, L.esl_last_error().decode()) == (status, f"{who}: {text}")
            if repair == "ctx":
                a["cx"] = cx
            elif repair == "map":
                cx.dense_begin()
                cx.dense_add_frames(good, K, 4, 4, np.full((1, 4, 4), 5000, np.uint16), np.full((1, 4, 4, 3), 9, np.uint8), np.zeros((1, 4, 4), np.int32))
                before = cx.dense_info()
                assert before["n_samples"] == 16 and before["status"] == 0
            elif isinstance(repair, tuple):
                p.update(repair[0])
            else:
                a.update(repair)
        assert (vox == 77).all() and cx.dense_info() == before          # every refused call wrote nothing
        rc, res = call()
        assert rc == 0 and res["status"] == 0 and res["n_voxels"] == cx.dense_extract(want=("key",))["n_voxels"] > 0 and res["n_chunks"] == 1
        assert (vox != 77).all()
    finally:
        cx.close()
