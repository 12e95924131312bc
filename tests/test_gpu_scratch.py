"""The grow-only device scratch of the map-side calls (csrc/esl_scratch.hpp) through esl_debug_scratch_allocs: a warm call allocates
nothing, a smaller call after a larger one reads nothing the larger one left behind, a call grows exactly the slots it needs, every
owner keeps a set of its own, and the four callers of the resident-source check word it alike.

Every comparison is bit for bit between two runs of the device (the same call warm and cold, or on a used and on a fresh context);
what the calls compute is held to their references in their own test files.  esl_render_map's grow-only case is
tests/test_gpu_render.py::test_repeats_and_grow_only_buffers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc2d_scenes as a2          # noqa: E402
import init_batch_ref as ib          # noqa: E402
import init_robust_ref as ir         # noqa: E402
import map_merge_scenes as ms        # noqa: E402
import reloc_scenes as rs            # noqa: E402
import render_scenes as rn           # noqa: E402

pytestmark = pytest.mark.gpu

OWNERS = ("reloc", "assoc", "merge", "render", "init_batch", "init_robust")


def flat(x):
    """every array and number of a call's result, in a fixed order, as bytes"""
    if isinstance(x, dict):
        return [b for k in sorted(x) for b in flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [b for v in x for b in flat(v)]
    return [] if x is None else [np.asarray(x).tobytes()]


# ---- the calls: scene -> result, one function per owner -------------------------------------------------------------------------------
def reloc_call(pkg, cx, s):
    cx.reloc_set_map(s["map"], s["map_labels"], s["ground_world"])
    return cx.relocalize(s["det"], s["det_labels"], s["ground_cam"], pkg.abi.default_reloc_params(min_inliers=2))


def assoc_call(pkg, cx, s):
    return (cx.associate_boxes(s["cams"], s["objs"], s["obj_labels"], s["K"], s["rows"], s["cols"], s["det_offsets"], s["det_boxes"],
                               s["det_labels"]),
            cx.predict_boxes(s["cams"][0], s["objs"], s["K"], s["rows"], s["cols"]))


def merge_call(pkg, cx, s):
    return cx.map_overlaps(s["objs"], s["labels"]), cx.map_merge(s["objs"], s["labels"], None, s["obs_cam"], s["obs_obj"])


def init_batch_call(pkg, cx, s):
    return cx.init_quadrics(s["cams"], s["N"], s["obs_cam"], s["obs_obj"], s["obs_boxes"], s["K"])


def init_robust_call(pkg, cx, s):
    return cx.init_quadrics_robust(s["cams"], s["N"], s["obs_cam"], s["obs_obj"], s["obs_boxes"], s["K"], faithful=0, want_hyp=True)


# ---- the scenes: a larger one, a smaller one, and a strictly smaller cut of the smaller one -----------------------------------------------
def reloc_scenes():
    return rs.room_scene(1, [8, 8], [0, 1, 2, 8, 9]), rs.room_scene(3, [3, 3], [0, 1, 3]), rs.room_scene(3, [1, 1], [0, 1])


def assoc_scenes():
    big, small = a2.room_scene(0), a2.room_scene(1, M=12, F=3)
    n = int(small["det_offsets"][1])          # frame 0 alone, eight of the twelve objects
    tiny = dict(small, cams=small["cams"][:1], objs=small["objs"][:8], obj_labels=small["obj_labels"][:8],
                det_offsets=small["det_offsets"][:2], det_boxes=small["det_boxes"][:n], det_labels=small["det_labels"][:n])
    return big, small, tiny


def merge_scenes():
    big, small = ms.clutter_scene(0), ms.clutter_scene(1, M=15)
    keep = small["obs_obj"] < 8
    tiny = dict(objs=small["objs"][:8], labels=small["labels"][:8], obs_cam=small["obs_cam"][keep], obs_obj=small["obs_obj"][keep])
    return big, small, tiny


def init_cut(s, N, F):
    """the first N objects and F cameras of an esl_init_quadrics list: fewer objects, frames and observations"""
    keep = (s["obs_obj"] < N) & (s["obs_cam"] < F)
    return dict(cams=s["cams"][:F], N=N, obs_cam=s["obs_cam"][keep], obs_obj=s["obs_obj"][keep], obs_boxes=s["obs_boxes"][keep], K=s["K"])


def init_batch_scenes():
    s = ib.scene("A0")
    return s, init_cut(s, 6, 60), init_cut(s, 3, 30)


def init_robust_scenes():
    s = ir.planted_scene("A0")
    return s, init_cut(s, 6, 60), init_cut(s, 3, 30)


GROW_ONLY = {"reloc": (reloc_call, reloc_scenes), "assoc": (assoc_call, assoc_scenes), "merge": (merge_call, merge_scenes),
             "init_batch": (init_batch_call, init_batch_scenes), "init_robust": (init_robust_call, init_robust_scenes)}


# ---- tests -------------------------------------------------------------------------------------------------------------------------------------------
def test_fresh_context_and_unknown_owner(pkg):
    cx = pkg.Context(0)
    try:
        for k, owner in enumerate(OWNERS):
            assert cx.scratch_allocs(owner) == (0, 0) and cx.scratch_allocs(k) == (0, 0), owner
        assert cx.render_allocs() == (0, 0)
        for bad in (-1, len(OWNERS), 99):
            with pytest.raises(pkg.EslError, match="esl_status 2"):
                cx.scratch_allocs(bad)
        L = pkg.lib.load()
        n = C.c_int64(7)
        assert L.esl_debug_scratch_allocs(cx._h, 0, None, C.byref(n)) == 2 and L.esl_debug_scratch_allocs(cx._h, 0, C.byref(n), None) == 2
        assert L.esl_debug_scratch_allocs(None, 0, C.byref(n), C.byref(n)) == 2
    finally:
        cx.close()


@pytest.mark.parametrize("owner", list(GROW_ONLY))
def test_grow_only(pkg, owner):
    call, scenes = GROW_ONLY[owner]
    big, small, tiny = scenes()
    cx, fresh = pkg.Context(0), pkg.Context(0)
    try:
        a0, b0 = flat(call(pkg, cx, big)), flat(call(pkg, cx, small))
        counters = cx.scratch_allocs(owner)
        print(owner, "allocations %d, bytes held %d" % counters)
        assert counters[0] > 0 and counters[1] > 0
        a1, b1 = flat(call(pkg, cx, big)), flat(call(pkg, cx, small))          # warm: the same shapes again, the smaller after the larger
        assert cx.scratch_allocs(owner) == counters          # nothing allocated
        assert a1 == a0 and b1 == b0
        call(pkg, cx, big)
        t = flat(call(pkg, cx, tiny))          # strictly smaller, after the larger one
        assert cx.scratch_allocs(owner) == counters
        assert t == flat(call(pkg, fresh, tiny))          # it reads nothing the larger one left behind
        assert 0 < fresh.scratch_allocs(owner)[1] < counters[1]
        for other in OWNERS:          # the robust call's refit is an esl_init_quadrics call: the one owner that uses another
            if other != owner and (owner, other) != ("init_robust", "init_batch"):
                assert cx.scratch_allocs(other) == (0, 0), other
    finally:
        cx.close(); fresh.close()


def test_render_grows_exactly_the_measured_depth_and_the_comparison(pkg):
    s = rn.room_scene(0)
    F, M, npix = len(s["cams"]), len(s["objs"]), s["rows"] * s["cols"]
    raw = np.full((F, s["rows"], s["cols"]), 10000, np.uint16)
    cx = pkg.Context(0)
    try:
        first = cx.render_map(s["cams"], s["objs"], s["K"], s["rows"], s["cols"])
        n0, b0 = cx.scratch_allocs("render")
        assert cx.render_allocs() == (n0, b0) and n0 > 0
        second = cx.render_map(s["cams"], s["objs"], s["K"], s["rows"], s["cols"], raw)
        n1, b1 = cx.scratch_allocs("render")
        # two slots more, and the bytes of exactly these two: uint16 per pixel, four int32 per (frame, object); the rest kept their capacity
        assert n1 == n0 + 2 and b1 == b0 + F * npix * 2 + F * M * 4 * 4
        assert set(second) == set(first) | {"cmp"} and all(second[k].tobytes() == first[k].tobytes() for k in first)
    finally:
        cx.close()


def test_init_quadrics_grows_exactly_the_stats(pkg):
    s = ib.scene("A0")
    N, n_obs = s["N"], len(s["obs_cam"])
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    Kc = (C.c_double * 4)(*s["K"])
    oc, oo, ob = (np.ascontiguousarray(s[k]) for k in ("obs_cam", "obs_obj", "obs_boxes"))
    cams = np.ascontiguousarray(s["cams"])

    def call(cx, stats):
        ell = np.zeros((N, 10))
        rc = pkg.lib.load().esl_init_quadrics(cx._h, cams.ctypes.data_as(dp), C.c_int32(len(cams)), C.c_int32(N), oc.ctypes.data_as(ip),
                                              oo.ctypes.data_as(ip), ob.ctypes.data_as(dp), C.c_int64(n_obs), Kc, C.c_int32(480), C.c_int32(640),
                                              C.c_int32(1), C.c_int32(0), ell.ctypes.data_as(dp), dp(), dp(),
                                              stats.ctypes.data_as(ip) if stats is not None else ip())
        pkg.lib._check(rc, "esl_init_quadrics")
        return ell
    cx = pkg.Context(0)
    try:
        e0 = call(cx, None)
        n0, b0 = cx.scratch_allocs("init_batch")
        stats = np.full((N, 4), -1, np.int32)
        e1 = call(cx, stats)
        n1, b1 = cx.scratch_allocs("init_batch")
        assert n0 > 0 and n1 == n0 + 1 and b1 == b0 + N * 4 * 4          # four int32 per object
        assert e1.tobytes() == e0.tobytes() and (stats[:, 1] > 0).all()
    finally:
        cx.close()


def test_owners_are_separate(pkg):
    s = a2.room_scene(1, M=12, F=3)
    cx = pkg.Context(0)
    try:
        assoc_call(pkg, cx, s)
        assert cx.scratch_allocs("assoc")[0] > 0
        assert cx.scratch_allocs("render") == (0, 0) and cx.render_allocs() == (0, 0)
    finally:
        cx.close()


def raw_render(pkg, cx, cams, F, objs, M):
    """esl_render_map's flags alone, F and M free of the arrays"""
    dp = C.POINTER(C.c_double)
    flags = np.zeros(max(F * M, 1), np.int32)
    rc = pkg.lib.load().esl_render_map(cx._h, None if cams is None else np.ascontiguousarray(cams).ctypes.data_as(dp), F,
                                       None if objs is None else np.ascontiguousarray(objs).ctypes.data_as(dp), M,
                                       (C.c_double * 4)(*rn.K), 8, 8, None, None, None, None, None, None,
                                       flags.ctypes.data_as(C.POINTER(C.c_int32)))
    pkg.lib._check(rc, "esl_render_map")


def test_resident_source_check(pkg):
    """the four callers: a NULL source without a resident graph is ESL_ERR_STATE, a count that differs from the resident graph's is
    ESL_ERR_INVALID, in one wording"""
    g, c, o, _ = pkg.synth.make_graph(6, 5, 40, seed=1)
    F, M = g.n_cams, g.n_objs
    gw = [0, 0, 1, 0]
    off = np.zeros(F + 1, np.int32)
    none = np.zeros((0, 4))

    def lab(n):
        return np.zeros(n, np.int32)
    cx = pkg.Context(0)
    try:
        null_objs = {
            "esl_reloc_set_map": lambda m: cx.reloc_set_map(None, lab(m), gw),
            "esl_associate_boxes": lambda m: cx.associate_boxes(c, None, lab(m), a2.K, a2.ROWS, a2.COLS, off, none, []),
            "esl_map_overlaps": lambda m: cx.map_overlaps(None, lab(m)),
            "esl_map_merge": lambda m: cx.map_merge(None, lab(m)),
            "esl_render_map": lambda m: raw_render(pkg, cx, c, F, None, m),
        }
        null_cams = {
            "esl_associate_boxes": lambda f: cx.associate_boxes(None, o, lab(M), a2.K, a2.ROWS, a2.COLS, np.zeros(f + 1, np.int32), none, []),
            "esl_render_map": lambda f: raw_render(pkg, cx, None, f, o, M),
        }
        for who, fn in null_objs.items():
            with pytest.raises(pkg.EslError, match="esl_status 4: %s: NULL objs needs a resident graph with states" % who):
                fn(M)
        for who, fn in null_cams.items():
            with pytest.raises(pkg.EslError, match="esl_status 4: %s: NULL cams needs a resident graph with states" % who):
                fn(F)
        cx.upload_graph(g); cx.upload_states(c, o)
        for who, fn in null_objs.items():
            with pytest.raises(pkg.EslError, match="esl_status 2: %s: M differs from the resident graph's n_objs" % who):
                fn(M + 1)
            fn(M)
        for who, fn in null_cams.items():
            with pytest.raises(pkg.EslError, match="esl_status 2: %s: F differs from the resident graph's n_cams" % who):
                fn(F + 1)
            fn(F)
    finally:
        cx.close()
