"""esl_dense_remove_frames / _move_frames / _purge / _slots_get on the device: against the numpy statement (tests/dense_update_ref.py)
and against device maps built from scratch from the surviving samples.

The contract under test (include/esl.h, "the dense map", steps 8-11): while the status stays 0, any interleaving of add, remove, move
and purge calls leaves the bytes that esl_dense_begin and one esl_dense_add_frames of the multiset difference leave, in every output
of esl_dense_extract, esl_dense_objects and esl_dense_planes and in esl_dense_info.  Every comparison is exact.  The scenes and the
conditions under which they test something are those of tests/dense_update_scenes.py, asserted on the statement alone."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_planes_scenes as dps     # noqa: E402
import dense_scenes as sc             # noqa: E402
import dense_update_ref as ur         # noqa: E402
import dense_update_scenes as us      # noqa: E402

pytestmark = pytest.mark.gpu

OUTS = ("key", "xyz", "count", "bgr", "inst", "votes")
MAXV = us.MAXV
ALL = list(range(us.N_CAMS))
KEPT, REMOVED, MOVED = us.kept(), list(us.REMOVED), list(us.MOVED)
STAY = [f for f in ALL if f not in MOVED]          # the frames the move leaves where they are
ZERO_ADD = dict(n_sampled=0, n_zero=0, n_depth_out=0, n_key_out=0, n_used=0)
ZERO_REMOVE = dict(ZERO_ADD, n_missing=0, n_emptied=0)
ROOM_GROUND = (0.0, -1.0, 0.0, 0.6)          # as tests/test_gpu_dense_objects.py: the floor 0.6 m below the cameras
FLOOR = (0.0, 0.0, 1.0, 0.0)
POS_SHIFT = (10.0, 10.0, 10.0)          # as tests/test_gpu_dense.py: the whole room inside the voxel [0, 50)^3 of leaf 50


def begin(pkg, cx, with_color=True, with_inst=True, **over):
    over.setdefault("max_voxels", MAXV)
    cx.dense_begin(pkg.abi.default_dense_params(**over), with_color, with_inst)


def add(cx, s, idx, cams="cams"):
    return cx.dense_add_frames(*us.frames_of(s, idx, cams))


def rem(cx, s, idx, cams="cams"):
    return cx.dense_remove_frames(*us.frames_of(s, idx, cams))


def move(cx, s, old, new):
    return cx.dense_move_frames(s[old], None if new is None else s[new], s["K"], s["rows"], s["cols"], s["depth"], s["bgr"], s["inst"])


def snap(cx):
    return dict(cx.dense_extract(), info=cx.dense_info())


def scratch(pkg, cx, s, idx, cams="cams", with_color=True, with_inst=True, **over):
    """a device map from scratch: one add of the frames idx"""
    begin(pkg, cx, with_color, with_inst, **over)
    add(cx, s, idx, cams)
    return snap(cx)


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def of_ref(m):
    return dict(m.extract(), info=m.info())


# ---- 1. add(all), remove(A) = the statement = a device map of B alone ----------------------------------------------------------------------
@pytest.mark.parametrize("leaf,stride,with_color,with_inst", [
    (0.01, 1, True, True), (0.01, 3, True, True), (0.05, 1, True, True), (0.05, 3, True, True),
    (0.05, 1, False, True), (0.05, 1, True, False), (0.05, 1, False, False), (0.01, 3, False, False)])
def test_remove_equals_statement_and_from_scratch(pkg, ctx, leaf, stride, with_color, with_inst):
    s = us.room()
    us.removal_conditions(leaf, stride); us.room_maps(leaf, stride)          # the conditions of exact equality, and of a removal that bites
    m, radd = us.build(s, ALL, with_color=with_color, with_inst=with_inst, leaf=leaf, stride=stride)
    rrem = m.remove_frames(*us.frames_of(s, REMOVED))
    begin(pkg, ctx, with_color, with_inst, leaf=leaf, stride=stride)
    assert add(ctx, s, ALL) == radd
    res = rem(ctx, s, REMOVED)
    assert res == rrem and res["status"] == 0 and res["n_emptied"] > 0 and res["n_missing"] == 0
    dev = snap(ctx)
    same(dev, of_ref(m))
    assert ctx.dense_slots() == m.slots()
    same(dev, scratch(pkg, ctx, s, KEPT, with_color=with_color, with_inst=with_inst, leaf=leaf, stride=stride))


# ---- 2. the run boundaries of the combined removal ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 65), (1, 129), (65, 1), (1, 1)])
@pytest.mark.parametrize("stride", [1, 3, 64])
def test_run_boundaries(pkg, ctx, rows, cols, stride):
    K = (60.0, 60.0, (cols - 1) / 2 + 0.25, (rows - 1) / 2 + 0.3)
    s = sc.room_scene(0, rows=rows, cols=cols, Kx=K)
    m, radd = us.build(s, [0, 1], leaf=0.05, stride=stride)
    sc.check_conditions(m, two_frames=False)
    rrem = m.remove_frames(*us.frames_of(s, [0]))
    begin(pkg, ctx, leaf=0.05, stride=stride)
    assert add(ctx, s, [0, 1]) == radd and rem(ctx, s, [0]) == rrem and rrem["status"] == 0
    dev = snap(ctx)
    same(dev, of_ref(m))
    same(dev, scratch(pkg, ctx, s, [1], leaf=0.05, stride=stride))


# ---- 3. one voxel ---------------------------------------------------------------------------------------------------------------------------
def test_one_voxel(pkg, ctx):
    s = sc.room_scene(0, shift=POS_SHIFT)
    over = dict(leaf=50.0, depth_max=20.0)
    one = scratch(pkg, ctx, s, [0], **over)
    begin(pkg, ctx, **over)
    add(ctx, s, [0, 0])          # the same frame twice
    two = snap(ctx)
    assert two["n_voxels"] == 1 and two["count"][0] == 2 * one["count"][0] > 4000
    r = rem(ctx, s, [0])
    assert r["n_used"] == one["count"][0] and r["n_emptied"] == 0 and r["n_missing"] == 0 and r["status"] == 0
    same(snap(ctx), one)          # the counts and the sums halve exactly
    r = rem(ctx, s, [0])
    assert r["n_used"] == one["count"][0] and r["n_emptied"] == 1 and r["status"] == 0
    info = ctx.dense_info()
    assert info["n_voxels"] == 0 and info["n_pairs"] == 0 and info["n_samples"] == 0 and info["status"] == 0
    sl = ctx.dense_slots()
    assert sl["voxel_slots"] == 1 and sl["dead_voxels"] == 1 and sl["pair_slots"] == sl["dead_pairs"] == one["info"]["n_pairs"]
    ext = ctx.dense_extract()
    assert ext["n_voxels"] == 0 and all(len(ext[k]) == 0 for k in OUTS)
    buf = np.full((4, 3), 77, np.int32); n = ctypes.c_int64(5)
    L = pkg.lib.load()
    assert L.esl_dense_extract(ctx._h, 4, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None, None, None, None, None, ctypes.byref(n)) == 0
    assert n.value == 0 and (buf == 77).all()
    ob = ctx.dense_objects(3, FLOOR)
    assert ob["result"]["status"] == 0 and ob["result"]["n_voxels"] == 0 and ob["result"]["n_components"] == 0 and (ob["stats"][:, 0] == 1).all()
    pl = ctx.dense_planes()
    assert pl["result"]["status"] == 0 and pl["result"]["n_voxels"] == 0 and pl["result"]["n_planes"] == 0
    add(ctx, s, [0])          # the dead slot is revived
    same(snap(ctx), one)
    assert ctx.dense_slots()["dead_voxels"] == 0 and ctx.dense_slots()["voxel_slots"] == 1


# ---- 4. plain and combined removal ------------------------------------------------------------------------------------------------------------
def test_plain_and_combined_removal_agree(pkg, ctx):
    """ESL_DENSE_COMBINE picks the form of both kernels at esl_dense_begin: integer sums, the same bits"""
    old = os.environ.get("ESL_DENSE_COMBINE")
    s, one = us.room(), sc.room_scene(0, shift=POS_SHIFT)
    res = {}
    try:
        for form in ("0", "1"):
            os.environ["ESL_DENSE_COMBINE"] = form
            res[form] = []
            for leaf in (0.01, 0.2):
                begin(pkg, ctx, leaf=leaf)
                add(ctx, s, ALL)
                res[form].append((rem(ctx, s, REMOVED), snap(ctx), ctx.dense_slots()))
            begin(pkg, ctx, leaf=50.0, depth_max=20.0)
            add(ctx, one, [0, 1, 2])
            res[form].append((rem(ctx, one, [1]), snap(ctx), ctx.dense_slots()))
    finally:
        if old is None:
            os.environ.pop("ESL_DENSE_COMBINE", None)
        else:
            os.environ["ESL_DENSE_COMBINE"] = old
    for (ra, a, sa), (rb, b, sb) in zip(res["0"], res["1"]):
        assert ra == rb and ra["status"] == 0 and sa == sb
        same(a, b)
    same(res["0"][0][1], of_ref(us.room_maps(0.01, 1)["kept"]))


# ---- 5. interleavings -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("purge", [False, True])
def test_interleavings_equal_one_from_scratch_map(pkg, ctx, purge):
    s = us.with_moved(us.room())
    leaf = 0.05
    want = of_ref(us.room_maps(leaf, 1)["moved"])
    same(scratch(pkg, ctx, s, ALL, "cams_moved", leaf=leaf), want)

    def mid():
        if purge:
            before, after = ctx.dense_purge()
            assert after["dead_voxels"] == 0 and after["dead_pairs"] == 0 and after["voxel_slots"] == before["voxel_slots"] - before["dead_voxels"]

    def order_a():          # frame by frame at the first poses, then one move of the whole set
        for f in ALL:
            add(ctx, s, [f])
        mid()
        r = move(ctx, s, "cams", "cams_moved")
        assert r["n_frames_moved"] == len(MOVED) and r["n_frames_same"] == us.N_CAMS - len(MOVED) and r["added"]["status"] == 0

    def order_b():          # the moved frames first, removed and added again one by one among the others
        add(ctx, s, MOVED)
        add(ctx, s, [STAY[0]])
        rem(ctx, s, [MOVED[0]])
        mid()
        add(ctx, s, [MOVED[0]], "cams_moved")
        add(ctx, s, STAY[1:])
        rem(ctx, s, MOVED[1:])
        add(ctx, s, MOVED[1:], "cams_moved")

    def order_c():          # everything at the second poses, the staying frames moved back; a frame removed and added again on the way
        add(ctx, s, ALL, "cams2")
        rem(ctx, s, [MOVED[0]], "cams2")
        r = move(ctx, dict(s, old=s["cams2"][STAY], new=s["cams"][STAY], depth=s["depth"][STAY], bgr=s["bgr"][STAY], inst=s["inst"][STAY]),
                 "old", "new")
        assert r["n_frames_moved"] == len(STAY)
        mid()
        add(ctx, s, [MOVED[0]], "cams2")

    runs = []
    for order in (order_a, order_b, order_c, order_a):          # the last: a repeat run
        begin(pkg, ctx, leaf=leaf)
        order()
        runs.append(snap(ctx))
        same(runs[-1], want)
        # a move to the same poses changes nothing
        r = move(ctx, s, "cams_moved", "cams_moved")
        assert r == dict(removed=dict(ZERO_REMOVE, status=0), added=dict(ZERO_ADD, status=0), n_frames_moved=0, n_frames_same=us.N_CAMS)
        same(snap(ctx), want)
    same(runs[0], runs[3])


# ---- 6. move ------------------------------------------------------------------------------------------------------------------------------------
def test_move_equals_statement_remove_add_and_from_scratch(pkg, ctx):
    s = us.with_moved(us.room())
    leaf = 0.01
    cond = us.move_conditions(leaf, 1)
    m, _ = us.build(s, ALL, leaf=leaf)
    rres = m.move_frames(s["cams"], s["cams_moved"], s["K"], s["rows"], s["cols"], s["depth"], s["bgr"], s["inst"])
    begin(pkg, ctx, leaf=leaf)
    add(ctx, s, ALL)
    res = move(ctx, s, "cams", "cams_moved")
    assert res == rres and res["removed"]["n_emptied"] == cond["revived"] + cond["dead"] and res["added"]["status"] == 0
    moved = snap(ctx)
    same(moved, of_ref(m))
    assert ctx.dense_slots() == m.slots() and ctx.dense_slots()["dead_voxels"] == cond["dead"]
    begin(pkg, ctx, leaf=leaf)
    add(ctx, s, ALL)
    assert rem(ctx, s, MOVED) == rres["removed"] and add(ctx, s, MOVED, "cams_moved") == rres["added"]
    same(snap(ctx), moved)
    same(scratch(pkg, ctx, s, ALL, "cams_moved", leaf=leaf), moved)


def test_move_to_the_resident_cameras(pkg):
    g, c, o, _ = pkg.synth.make_graph(12, 30, 200, seed=3)
    rng = np.random.default_rng(5)
    cx = pkg.Context(0)
    try:
        cx.upload_graph(g); cx.upload_states(c, o)
        c0, o0 = cx.download_states()
        F = len(c0)
        s = dict(cams=c0, cams2=us.second_poses(c0, 3), K=(40.0, 40.0, 7.6, 5.3), rows=12, cols=16,
                 depth=rng.integers(2600, 20000, (F, 12, 16)).astype(np.uint16), bgr=rng.integers(0, 256, (F, 12, 16, 3), dtype=np.uint8),
                 inst=rng.integers(-1, 4, (F, 12, 16)).astype(np.int32))
        s["cams2"][3] = c0[3]          # one frame stays
        for name in ("cams", "cams2"):
            sc.check_conditions(us.build(s, range(F), name, leaf=0.05)[0], two_frames=False)
        want = scratch(pkg, cx, s, range(F), leaf=0.05)
        begin(pkg, cx, leaf=0.05)
        add(cx, s, range(F), "cams2")
        r = move(cx, s, "cams2", None)
        assert r["n_frames_moved"] == F - 1 and r["n_frames_same"] == 1 and r["removed"]["status"] == 0
        same(snap(cx), want)
        # ... and removal with the resident cameras
        r = cx.dense_remove_frames(None, s["K"], 12, 16, s["depth"], s["bgr"], s["inst"])
        assert r["status"] == 0 and r["n_used"] == want["info"]["n_samples"] and cx.dense_info()["n_voxels"] == 0
        c1, o1 = cx.download_states()
        assert c0.tobytes() == c1.tobytes() and o0.tobytes() == o1.tobytes()
    finally:
        cx.close()


# ---- 7. downstream: objects and planes see live voxels only ---------------------------------------------------------------------------------------
def downstream(pkg, cx):
    ob = cx.dense_objects(13, ROOM_GROUND, pkg.abi.default_dense_obj_params(min_component=20))
    pl = cx.dense_planes(pkg.abi.default_dense_plane_params(**dps.ROOM), hyp=True)
    return dict(obj_result=ob["result"], objs=ob["objs"], obj_stats=ob["stats"], comp=ob["comp"], voxel_comp=ob["voxel_comp"],
                pl_result=pl["result"], planes=pl["planes"], centroid=pl["centroid"], pl_stats=pl["stats"], samples=pl["samples"],
                ground=pl["ground"], voxel_plane=pl["voxel_plane"], hyp=pl["hyp"])


def test_objects_and_planes_after_removal_and_move(pkg, ctx):
    s = us.with_moved(us.room())
    leaf = 0.05
    us.removal_conditions(leaf, 1); us.move_conditions(leaf, 1)
    scratch(pkg, ctx, s, KEPT, leaf=leaf)
    want_kept = downstream(pkg, ctx)
    scratch(pkg, ctx, s, ALL, "cams_moved", leaf=leaf)
    want_moved = downstream(pkg, ctx)
    assert want_kept["obj_result"]["n_components"] > 0 and want_kept["pl_result"]["n_planes"] > 0
    begin(pkg, ctx, leaf=leaf)
    add(ctx, s, ALL)
    downstream(pkg, ctx)          # the readers' own buffers now hold the full map's lists
    rem(ctx, s, REMOVED)
    same(downstream(pkg, ctx), want_kept)
    add(ctx, s, REMOVED)
    move(ctx, s, "cams", "cams_moved")
    same(downstream(pkg, ctx), want_moved)
    ctx.dense_purge()
    same(downstream(pkg, ctx), want_moved)


def test_removing_the_bridge_splits_the_component(pkg, ctx):
    assert us.bridge_conditions() == dict(full=1, kept=2)
    b = us.bridge()
    s, n = b["frames"], b["n_blob"]
    P = pkg.abi.default_dense_obj_params(reach=us.BRIDGE_REACH, min_component=1)
    scratch(pkg, ctx, s, range(n), leaf=us.BRIDGE_LEAF)
    want = ctx.dense_objects(1, FLOOR, P)
    assert want["result"]["n_components"] == 2
    begin(pkg, ctx, leaf=us.BRIDGE_LEAF)
    add(ctx, s, range(n + 1))
    assert ctx.dense_objects(1, FLOOR, P)["result"]["n_components"] == 1          # and the neighbour index of every slot is written
    r = rem(ctx, s, [n])
    assert r["n_emptied"] == 1 and r["status"] == 0
    got = ctx.dense_objects(1, FLOOR, P)
    assert got["result"]["n_components"] == 2
    same(got, want)


# ---- 8. capacity ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("purge", [False, True])
def test_capacity_counts_claimed_slots(pkg, ctx, purge):
    """The map with MOVED at their second poses fits max_voxels exactly; taking them back to the first poses claims new slots."""
    s = us.with_moved(us.room())
    mp = us.room_maps(0.05, 1)
    V = mp["moved"].info()["n_voxels"]
    assert mp["full"].info()["n_voxels"] <= V
    m, radd = us.build(s, ALL, "cams_moved", leaf=0.05, max_voxels=V)
    begin(pkg, ctx, leaf=0.05, max_voxels=V)
    assert add(ctx, s, ALL, "cams_moved") == radd and radd["status"] == 0
    assert rem(ctx, s, MOVED, "cams_moved") == m.remove_frames(*us.frames_of(s, MOVED, "cams_moved"))
    assert ctx.dense_slots() == m.slots() and m.slots()["voxel_slots"] == V and m.slots()["dead_voxels"] > 0
    if purge:
        assert ctx.dense_purge() == m.purge()
        assert ctx.dense_slots() == m.slots() and m.slots()["dead_voxels"] == 0 and m.slots()["dead_pairs"] == 0
    ra = m.add_frames(*us.frames_of(s, MOVED))
    assert add(ctx, s, MOVED) == ra
    assert ctx.dense_info() == m.info()
    if purge:
        assert ra["status"] == 0
        assert ctx.dense_slots() == m.slots()
        same(snap(ctx), of_ref(mp["full"]))
    else:
        assert ra["status"] == 3 and ctx.dense_info()["n_voxels"] == -1 and ctx.dense_extract()["n_voxels"] == -1
        assert ctx.dense_slots() == dict(voxel_slots=-1, dead_voxels=-1, pair_slots=-1, dead_pairs=-1)
        assert rem(ctx, s, MOVED) == dict(ZERO_REMOVE, status=3)          # a map at status 3 stays at 3
        assert ctx.dense_purge()[1]["voxel_slots"] == -1 and ctx.dense_info()["status"] == 3


# ---- 9. status 4 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["never_added", "twice", "other_colour"])
def test_status_4(pkg, ctx, route):
    s = us.room()
    m = ur.DenseUpdateMap(leaf=0.05, max_voxels=MAXV)
    begin(pkg, ctx, leaf=0.05)
    if route == "never_added":
        first, gone = KEPT, us.frames_of(s, REMOVED)
    elif route == "twice":
        first, gone = ALL, us.frames_of(s, REMOVED)
    else:
        first, gone = REMOVED, us.frames_of(dict(s, bgr=s["bgr"] ^ 1), REMOVED)
    assert add(ctx, s, first) == m.add_frames(*us.frames_of(s, first))
    if route == "twice":
        assert ctx.dense_remove_frames(*gone) == m.remove_frames(*gone)
        assert ctx.dense_info()["status"] == 0
    r = ctx.dense_remove_frames(*gone)
    assert r == m.remove_frames(*gone)
    assert r["status"] == 4 and (r["n_missing"] > 0) == (route == "never_added")
    info = ctx.dense_info()
    assert info == m.info() and info["status"] == 4 and info["n_voxels"] == -1 and info["n_pairs"] == -1
    # the map is invalid until the next esl_dense_begin
    ext = ctx.dense_extract()
    assert ext["n_voxels"] == -1 and all(len(ext[k]) == 0 for k in OUTS)
    ob = ctx.dense_objects(3, FLOOR)
    assert ob["result"]["status"] == 4 and ob["result"]["n_voxels"] == -1
    pl = ctx.dense_planes()
    assert pl["result"]["status"] == 4 and pl["result"]["n_voxels"] == -1
    assert add(ctx, s, ALL) == dict(ZERO_ADD, status=4)
    assert rem(ctx, s, ALL) == dict(ZERO_REMOVE, status=4)
    mv = move(ctx, s, "cams", "cams2")
    assert mv == dict(removed=dict(ZERO_REMOVE, status=4), added=dict(ZERO_ADD, status=4), n_frames_moved=0, n_frames_same=0)
    none = dict(voxel_slots=-1, dead_voxels=-1, pair_slots=-1, dead_pairs=-1)
    assert ctx.dense_slots() == none and ctx.dense_purge() == (none, none) and ctx.dense_info() == info
    same(scratch(pkg, ctx, s, KEPT, leaf=0.05), of_ref(us.room_maps(0.05, 1)["kept"]))          # esl_dense_begin clears it


# ---- 10. errors, F = 0, buffers, profiling, sizes ---------------------------------------------------------------------------------------------------
def raw(pkg, cx, name, s, ctx_h=True, **over):
    """the C-ABI itself, every argument free; raises like the binding.  Arrays are passed flat, without a shape check."""
    L = pkg.lib.load()
    a = dict(cams=s["cams"], cams_old=s["cams"], F=len(s["cams"]), K=s["K"], rows=s["rows"], cols=s["cols"], depth=s["depth"], bgr=s["bgr"],
             inst=s["inst"], out=True)
    a.update(over)
    keep = []

    def arr(x, dt, t):
        if x is None:
            return None
        x = np.ascontiguousarray(x, dtype=dt); keep.append(x)
        return x.ctypes.data_as(ctypes.POINTER(t))
    res = pkg.abi.EslDenseMoveResult() if name == "esl_dense_move_frames" else pkg.abi.EslDenseRemoveResult()
    poses = [arr(a["cams_old"], np.float64, ctypes.c_double)] if name == "esl_dense_move_frames" else []
    poses.append(arr(a["cams"], np.float64, ctypes.c_double))
    rc = getattr(L, name)(cx._h if ctx_h else None, *poses, a["F"], arr(a["K"], np.float64, ctypes.c_double), a["rows"], a["cols"],
                          arr(a["depth"], np.uint16, ctypes.c_uint16), arr(a["bgr"], np.uint8, ctypes.c_uint8),
                          arr(a["inst"], np.int32, ctypes.c_int32), ctypes.byref(res) if a["out"] else None)
    if rc != 0:
        raise pkg.EslError(f"{name} failed with esl_status {rc}: {L.esl_last_error().decode()}")
    return res.as_dict()


@pytest.mark.parametrize("name", ["esl_dense_remove_frames", "esl_dense_move_frames"])
def test_errors(pkg, name):
    s = us.room()
    cx = pkg.Context(0)
    L = pkg.lib.load()
    nan, inf = float("nan"), float("inf")
    try:
        with pytest.raises(pkg.EslError, match=f"esl_status 4: {name}: no esl_dense_begin"):
            raw(pkg, cx, name, s)
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_slots_get"):
            cx.dense_slots()
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_purge"):
            cx.dense_purge()
        begin(pkg, cx, leaf=0.05)
        add(cx, s, ALL)
        before = snap(cx)
        cases = [
            (dict(ctx_h=False), "ctx"), (dict(F=-1), "F"), (dict(K=None), "K"), (dict(depth=None), "depth"),
            (dict(rows=0), "rows"), (dict(rows=16385), "rows"), (dict(rows=-3), "rows"), (dict(cols=0), "cols"), (dict(cols=16385), "cols"),
            (dict(K=(0.0, 60, 4, 4)), "fx"), (dict(K=(nan, 60, 4, 4)), "fx"), (dict(K=(inf, 60, 4, 4)), "fx"), (dict(K=(-60.0, 60, 4, 4)), "fx"),
            (dict(K=(60, 0.0, 4, 4)), "fy"), (dict(K=(60, nan, 4, 4)), "fy"), (dict(K=(60, -1.0, 4, 4)), "fy"),
        ]
        for k, v in ((1, nan), (4, inf), (0, -inf)):          # an invalid pose in frame 2 of 4
            cams = s["cams"].copy(); cams[1, k] = v
            cases.append((dict(cams=cams), "pose"))
            if name == "esl_dense_move_frames":
                cases.append((dict(cams_old=cams, cams=s["cams2"]), "pose"))
        cams = s["cams"].copy(); cams[1, 3:] = 0.0
        cases.append((dict(cams=cams), "pose"))
        cams = s["cams"].copy(); cams[1, 3:] = 1e200          # the norm overflows
        cases.append((dict(cams=cams), "pose"))
        if name == "esl_dense_move_frames":
            cases.append((dict(cams_old=None), "cams_old"))
        for over, word in cases:
            with pytest.raises(pkg.EslError, match=f"esl_status 2: {name}: .*" + word):
                raw(pkg, cx, name, s, **over)
        with pytest.raises(pkg.EslError, match=f"esl_status 4: {name}: .*bgr"):
            raw(pkg, cx, name, s, bgr=None)
        with pytest.raises(pkg.EslError, match=f"esl_status 4: {name}: .*inst"):
            raw(pkg, cx, name, s, inst=None)
        with pytest.raises(pkg.EslError, match=f"esl_status 4: {name}: NULL cams needs a resident graph with states"):
            raw(pkg, cx, name, s, cams=None)
        # the 2^31 bound: frames claimed to be 16384 x 16384, eight of them (nothing of them is read before the refusal)
        big = dict(cams=np.tile(s["cams2"][:1], (8, 1)), cams_old=np.tile(s["cams"][:1], (8, 1)), F=8, rows=16384, cols=16384)
        with pytest.raises(pkg.EslError, match=f"esl_status 2: {name}: .*2\\^31"):
            raw(pkg, cx, name, s, **big)
        assert L.esl_dense_slots_get(cx._h, None) == 2 and L.esl_dense_slots_get(None, ctypes.byref(pkg.abi.EslDenseSlots())) == 2
        assert L.esl_dense_purge(None, None, None) == 2
        # every refused call left the map as it was
        same(snap(cx), before)
        # valid all the same: F = 0, a NULL result, a purge with NULL results
        zero = raw(pkg, cx, name, s, cams=None, cams_old=None, F=0, depth=None, bgr=None, inst=None)
        assert (zero["removed"] if "removed" in zero else zero)["n_sampled"] == 0
        assert raw(pkg, cx, name, s, cams=np.zeros((0, 7)), cams_old=np.zeros((0, 7)), F=0) == zero
        same(snap(cx), before)
        assert L.esl_dense_purge(cx._h, None, None) == 0
        same(snap(cx), before)
        raw(pkg, cx, name, s, cams=s["cams2"] if name == "esl_dense_move_frames" else s["cams"], out=False)
        want = us.room_maps(0.05, 1)["second"].info() if name == "esl_dense_move_frames" else dict(before["info"], n_samples=0, n_voxels=0, n_pairs=0)
        assert cx.dense_info() == want
        assert L.esl_dense_purge(cx._h, None, None) == 0 and cx.dense_slots()["dead_voxels"] == 0
        # the binding's own checks
        with pytest.raises(ValueError):
            cx.dense_remove_frames(s["cams"], s["K"], s["rows"], s["cols"] + 1, s["depth"], s["bgr"], s["inst"])
        with pytest.raises(ValueError):
            cx.dense_move_frames(None, s["cams"], s["K"], s["rows"], s["cols"], s["depth"], s["bgr"], s["inst"])
        with pytest.raises(ValueError):
            cx.dense_move_frames(s["cams"][:2], s["cams"], s["K"], s["rows"], s["cols"], s["depth"], s["bgr"], s["inst"])
    finally:
        cx.close()


def test_struct_sizes(pkg):
    assert ctypes.sizeof(pkg.abi.EslDenseRemoveResult) == 64 and ctypes.sizeof(pkg.abi.EslDenseMoveResult) == 120
    assert ctypes.sizeof(pkg.abi.EslDenseSlots) == 32
    assert pkg.abi.EslDenseMoveResult.added.offset == 64 and pkg.abi.EslDenseMoveResult.n_frames_moved.offset == 112


def update_round(pkg, cx, s):
    begin(pkg, cx, leaf=0.01)
    add(cx, s, ALL)
    rem(cx, s, REMOVED)
    add(cx, s, REMOVED)
    move(cx, s, "cams", "cams_moved")
    slots = cx.dense_purge()
    return snap(cx), slots


def test_grow_only_buffers(pkg):
    s = us.with_moved(us.room())
    cx = pkg.Context(0)
    try:
        a0, s0 = update_round(pkg, cx, s)
        allocs = cx.dense_allocs()
        assert allocs[0] > 0 and s0[0]["dead_voxels"] > 0 and s0[1]["dead_voxels"] == 0
        a1, s1 = update_round(pkg, cx, s)          # warm: the same shapes again
        assert cx.dense_allocs() == allocs and s0 == s1
        same(a0, a1)
        same(a1, of_ref(us.room_maps(0.01, 1)["moved"]))
        for owner in cx.SCRATCH_OWNERS:
            assert cx.scratch_allocs(owner) == (0, 0), owner
    finally:
        cx.close()


def test_profiling_class_4(pkg):
    s = us.with_moved(us.room())
    cx = pkg.Context(0)
    try:
        begin(pkg, cx, leaf=0.05)
        add(cx, s, ALL)
        cx.profile_enable(2)
        count = 0
        for call in (lambda: rem(cx, s, REMOVED), lambda: add(cx, s, REMOVED), lambda: move(cx, s, "cams", "cams_moved"), cx.dense_purge):
            call()
            prof = cx.profile_get()
            assert set(prof) == {"reduce"} and prof["reduce"]["count"] > count and prof["reduce"]["total_ms"] > 0
            count = prof["reduce"]["count"]
    finally:
        cx.close()
