"""esl_init_quadrics on the device: against the C oracle and the numpy statement (tests/init_batch_ref.py), against the single-object
call, its exact invariances, statuses, the tile boundaries, errors and bystanders.

Tolerances are those of test_gpu_init_quadric_matches_oracle (init_batch_ref.assert_values); the plane error is held to 1e-9
relative, the figure tests/test_adapter_link.py holds the single call to.  The conditions under which these are fair demands are
asserted on the CPU in tests/test_init_batch_ref.py for every scene and list used here; references are computed once and shared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_batch_ref as ib     # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, STATE = 2, 4   # ESL_ERR_INVALID, ESL_ERR_STATE


def dev(ctx, s, cams="given", **kw):
    return ctx.init_quadrics(s["cams"] if isinstance(cams, str) else cams, s["N"], s["obs_cam"], s["obs_obj"], s["obs_boxes"], s["K"], **kw)


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def rows_of(out, sel):
    return tuple(x[sel] for x in out)


def assert_against_reference(out, ref, what):
    ell, Q, err, st = out
    rell, rQ, rerr, rst = ref
    assert np.array_equal(st[:, :3], rst), (what, st, rst)
    for o in range(len(st)):
        if st[o, 0] in (1, 2):
            assert not ell[o].any() and not Q[o].any() and err[o] == 0, (what, o)
            continue
        ib.assert_values(ell[o], Q[o], rell[o], rQ[o], st[o, 0] == 0, (what, o))
        if st[o, 0] == 3:
            assert Q[o].any() and not ell[o].any() and err[o] == 0, (what, o)


@pytest.mark.parametrize("faithful", [0, 1])
@pytest.mark.parametrize("name", list(ib.SCENES))
def test_matches_oracle(ctx, name, faithful):
    out = dev(ctx, ib.scene(name), faithful=faithful)
    ref = ib.scene_reference(name, faithful)
    assert_against_reference(out, ref, (name, faithful))
    assert (out[3][:, 3] == 0).all()
    if name == "B":
        assert out[3][12, 0] == 3 and out[1][12].any() and not out[0][12].any()
        assert (np.delete(out[3][:, 0], 12) == 0).all()


@pytest.mark.parametrize("faithful", [0, 1])
@pytest.mark.parametrize("name", list(ib.SCENES))
def test_matches_single_call(po, ctx, name, faithful):
    s = ib.scene(name)
    ell, Q, err, st = dev(ctx, s, faithful=faithful)
    equal_bits = []
    for o, sel in enumerate(ib.group(s["obs_obj"], s["N"])):
        Tcw, boxes = s["cams"][s["obs_cam"][sel]], s["obs_boxes"][sel]
        Twc = np.array([po.se3_inv(T) for T in Tcw])
        e1, Q1, ok1 = ctx.init_quadric(Twc, boxes, s["K"], faithful=faithful)
        assert ok1 == (st[o, 0] == 0), (name, o)
        ib.assert_values(ell[o], Q[o], e1, Q1, ok1, (name, o))
        if ok1:
            single = ctx.init_plane_error(Twc, boxes, s["K"], ell[o])
            numpy_ = ib.plane_error(ib.plane_rows(Tcw, boxes, s["K"]), ell[o])
            print(name, faithful, o, "plane error %.17g, single call %.17g, numpy %.17g" % (err[o], single, numpy_))
            assert abs(err[o] - single) <= 1e-9 * abs(single), (name, o)
            assert abs(err[o] - numpy_) <= 1e-9 * abs(numpy_), (name, o)
            equal_bits.append(err[o] == single and ell[o].tobytes() == e1.tobytes())
    print(name, faithful, "objects with the single call's bits:", sum(equal_bits), "of", len(equal_bits))


def interleave(s, seed):
    """the same list dealt out in another interleaving of the objects, each object's own order kept"""
    rng = np.random.default_rng(seed)
    base = ib.group(s["obs_obj"], s["N"])
    owner = rng.permutation(s["obs_obj"][s["obs_obj"] >= 0])
    nxt = {o: iter(sel) for o, sel in enumerate(base)}
    perm = np.array([next(nxt[o]) for o in owner])
    return dict(s, obs_cam=s["obs_cam"][perm], obs_obj=s["obs_obj"][perm], obs_boxes=s["obs_boxes"][perm])


@pytest.mark.parametrize("name", ["A1", "B"])
def test_exact_invariances(pkg, ctx, name):
    s = ib.scene(name)
    N = s["N"]
    full = dev(ctx, s, faithful=1)
    assert same_bytes(full, dev(ctx, s, faithful=1)), "the same call twice"
    s2 = interleave(s, 3)
    assert not np.array_equal(s2["obs_obj"], s["obs_obj"])
    assert same_bytes(full, dev(ctx, s2, faithful=1)), "shuffled across objects"
    p = np.random.default_rng(4).permutation(N).astype(np.int32)
    ren = dev(ctx, dict(s, obs_obj=p[s["obs_obj"]]), faithful=1)
    assert same_bytes(full, rows_of(ren, p)), "objects renumbered"
    for o in sorted(set(range(0, N, 5)) | {N // 2}):   # N // 2 = 12 in scene B: the rejected object too
        alone = dev(ctx, dict(s, obs_obj=np.where(s["obs_obj"] == o, o, -1).astype(np.int32)), faithful=1)
        assert same_bytes(rows_of(full, [o]), rows_of(alone, [o])), ("alone in the batch", o)
        others = np.delete(np.arange(N), o)
        assert (alone[3][others, 0] == 2).all() and not alone[3][others, 1:].any() and not alone[0][others].any()
    own = pkg.Context(0)
    try:
        own.upload_graph(s["graph"])
        own.upload_states(s["cams"], s["objs"])
        assert same_bytes(full, dev(own, s, cams=None, faithful=1)), "resident camera states"
        assert same_bytes(full, dev(own, s, faithful=1)), "another context"
    finally:
        own.close()


def test_statuses_of_short_objects(ctx):
    s = ib.scene("A0")
    sel = ib.group(s["obs_obj"], s["N"])
    keep = np.concatenate([sel[2], sel[5][:2]])
    obj = np.concatenate([np.zeros(len(sel[2]), np.int32), np.full(2, 2, np.int32)])
    t = dict(s, N=3, obs_cam=s["obs_cam"][keep], obs_obj=obj, obs_boxes=s["obs_boxes"][keep])
    ell, Q, err, st = dev(ctx, t)
    assert st[:, :3].tolist() == [[0, len(sel[2]), 4 * len(sel[2])], [2, 0, 0], [2, 2, 8]]
    assert ell[0].any() and not ell[1:].any() and not Q[1:].any() and not err[1:].any()
    ell3, Q3, err3, st3 = dev(ctx, t, min_observations=3)
    assert st3[:, :3].tolist() == [[0, len(sel[2]), 4 * len(sel[2])], [1, 0, 0], [1, 2, 0]]
    assert same_bytes((ell, Q, err), (ell3, Q3, err3))


@pytest.mark.parametrize("name", ["A0", "A1"])
def test_min_observations_15(ctx, name):
    s = ib.scene(name)
    full = dev(ctx, s)
    gated = dev(ctx, s, min_observations=15)
    short = full[3][:, 1] < 15
    assert np.array_equal(gated[3][:, 0] == 1, short)
    assert same_bytes(rows_of(full, ~short), rows_of(gated, ~short))
    assert not gated[0][short].any() and not gated[1][short].any() and not gated[2][short].any() and not gated[3][short, 2].any()
    assert np.array_equal(gated[3][:, 1], full[3][:, 1])
    if name == "A1":
        assert short.any() and not short.all()


def test_box_edits_inside_a_batch(ctx):
    s = ib.scene("A0")
    cases = ib.box_edit_cases()
    N, F = s["N"], len(s["cams"])
    cams = np.concatenate([s["cams"]] + [c[0] for c in cases])
    at = F + np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])])
    t = dict(s, N=N + len(cases), cams=cams,
             obs_cam=np.concatenate([s["obs_cam"]] + [np.arange(at[i], at[i + 1], dtype=np.int32) for i in range(len(cases))]),
             obs_obj=np.concatenate([s["obs_obj"]] + [np.full(len(c[0]), N + i, np.int32) for i, c in enumerate(cases)]),
             obs_boxes=np.concatenate([s["obs_boxes"]] + [c[1] for c in cases]))
    out = dev(ctx, interleave(t, 9))
    assert out[3][N:, 2].tolist() == [c[2] for c in cases] == [8, 12, 11, 8, 8]
    assert out[3][N:, 0].tolist() == [0 if c[3] else 2 for c in cases] == [2, 0, 0, 2, 2]
    assert same_bytes(rows_of(out, slice(0, N)), dev(ctx, s)), "the normal objects beside them"
    assert_against_reference(out, ib.reference(t["cams"], t["N"], t["obs_cam"], t["obs_obj"], t["obs_boxes"], t["K"]), "box edits")


@pytest.mark.parametrize("faithful", [0, 1])
@pytest.mark.parametrize("i", range(len(ib.BOUNDARY)))
def test_tile_boundary(ctx, i, faithful):
    one, refs, spilled = ib.boundary_case(i)
    n = ib.BOUNDARY[i][3]
    out = dev(ctx, one, faithful=faithful)
    assert out[3].tolist() == [[0, n, 4 * n, spilled]], (ib.BOUNDARY[i], out[3])
    assert_against_reference(out, refs[faithful], ib.BOUNDARY[i])
    numpy_ = ib.plane_error(ib.plane_rows(one["cams"][one["obs_cam"]], one["obs_boxes"], one["K"]), out[0][0])
    assert abs(out[2][0] - numpy_) <= 1e-9 * abs(numpy_)


def raw(pkg, h, s, **over):
    """the C call with single arguments replaced; returns (rc, ellipsoids, stats)"""
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    N = over.get("N", s["N"])
    a = dict(cams=np.ascontiguousarray(s["cams"]), F=len(s["cams"]), N=N, obs_cam=np.ascontiguousarray(s["obs_cam"], np.int32),
             obs_obj=np.ascontiguousarray(s["obs_obj"], np.int32), obs_boxes=np.ascontiguousarray(s["obs_boxes"]), n_obs=len(s["obs_obj"]),
             K=np.array(s["K"]), rows=480, cols=640, faithful=1, min_observations=0, ell=np.full((max(N, 1), 10), 7.0),
             stats=np.full((max(N, 1), 4), 7, np.int32))
    a.update(over)

    def p(x, t):
        return t() if x is None or x.size == 0 else x.ctypes.data_as(t)
    rc = pkg.lib.load().esl_init_quadrics(h, p(a["cams"], dp), C.c_int32(a["F"]), C.c_int32(a["N"]), p(a["obs_cam"], ip), p(a["obs_obj"], ip),
                                          p(a["obs_boxes"], dp), C.c_int64(a["n_obs"]), p(a["K"], dp), C.c_int32(a["rows"]), C.c_int32(a["cols"]),
                                          C.c_int32(a["faithful"]), C.c_int32(a["min_observations"]), p(a["ell"], dp), None, None, p(a["stats"], ip))
    return rc, a["ell"], a["stats"]


def test_errors_and_empty_inputs(pkg, ctx):
    s = ib.scene("A0")
    h, F, N = ctx._h, len(s["cams"]), s["N"]
    assert raw(pkg, h, s)[0] == 0
    for over in (dict(K=None), dict(N=-1), dict(F=-1), dict(n_obs=-1), dict(min_observations=-1), dict(obs_cam=None), dict(obs_obj=None),
                 dict(obs_boxes=None), dict(ell=None), dict(rows=0), dict(cols=0)):
        assert raw(pkg, h, s, **over)[0] == INVALID, over
    assert raw(pkg, None, s)[0] == INVALID
    for k, v in (("obs_cam", F), ("obs_cam", -1), ("obs_obj", N)):
        bad = s[k].copy(); bad[17] = v
        assert raw(pkg, h, dict(s, **{k: bad}))[0] == INVALID, (k, v)
    skipped = s["obs_obj"].copy(); skipped[17] = -1
    bad = s["obs_cam"].copy(); bad[17] = F + 5
    assert raw(pkg, h, dict(s, obs_obj=skipped, obs_cam=bad))[0] == 0     # a skipped entry's frame is not looked at
    # N = 0: with an empty list, and with every entry skipped
    empty = dict(s, obs_cam=s["obs_cam"][:0], obs_obj=s["obs_obj"][:0], obs_boxes=s["obs_boxes"][:0])
    assert raw(pkg, h, empty, N=0)[0] == 0
    assert raw(pkg, h, dict(s, obs_obj=np.full_like(s["obs_obj"], -1)), N=0)[0] == 0
    assert raw(pkg, h, s, N=0)[0] == INVALID                              # obs_obj >= N
    # n_obs = 0 with N > 0
    rc, ell, st = raw(pkg, h, empty, N=3)
    assert rc == 0 and not ell.any() and st.tolist() == [[2, 0, 0, 0]] * 3
    rc, ell, st = raw(pkg, h, empty, N=3, min_observations=1)
    assert rc == 0 and not ell.any() and st.tolist() == [[1, 0, 0, 0]] * 3


def test_resident_cameras_errors_and_bystanders(pkg):
    s = ib.scene("A0")
    own = pkg.Context(0)
    try:
        assert raw(pkg, own._h, s, cams=None)[0] == STATE                 # no resident graph
        own.upload_graph(s["graph"])
        assert raw(pkg, own._h, s, cams=None)[0] == STATE                 # no states
        own.upload_states(s["cams"], s["objs"])
        before = own.download_states()
        assert raw(pkg, own._h, s, cams=None, F=len(s["cams"]) - 1)[0] == INVALID
        assert raw(pkg, own._h, s, cams=None)[0] == 0
        assert raw(pkg, own._h, s)[0] == 0
        after = own.download_states()
        assert same_bytes(before, after)
    finally:
        own.close()
