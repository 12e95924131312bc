"""Fixed ellipsoid vertices: the numpy reference (tests/fixed_ref.py) against the unmodified oracle/np_oracle.py, its known answer
(localisation against the true map), and the public surface of the feature (symbols, wrappers, constant).  No GPU needed."""
import inspect

import numpy as np

from oracle import np_oracle as npo
from tests import fixed_ref as fr


def cam_err(a, b):
    e = 0.0
    for x, y in zip(a, b):
        e = max(e, np.linalg.norm(npo.se3_log(npo.T_inv(npo.T_from7(x)) @ npo.T_from7(y))))
    return e


def test_no_flags_equals_np_oracle(pkg):
    g, c, o, _ = pkg.synth.make_graph(10, 4, 60, seed=5, slam=True)
    P = npo.NpGraph(g, c, o); P.drop_nan(); P.finalize()
    Hp, bp = P.build(1e-6)
    for flags in (None, np.zeros(g.n_objs, np.uint8)):
        G = fr.FixedNpGraph(g, c, o, flags); G.drop_nan(); G.finalize()
        assert G.n == P.n and G.idx_c == P.idx_c and G.idx_o == P.idx_o and not G.inactive_edges
        H, b = G.build(1e-6)
        assert np.array_equal(H, Hp) and np.array_equal(b, bp)
        assert G.chi2() == P.chi2()


def test_flags_delete_rows_and_columns(pkg):
    g, c, o, _ = pkg.synth.make_graph(12, 6, 120, seed=5, slam=True)
    fixed = sorted(np.argsort(-np.bincount(g.bbox_obj, minlength=g.n_objs))[:2].tolist())   # the two ellipsoids with the most boxes
    flags = np.zeros(g.n_objs, np.uint8); flags[fixed] = 1
    P = npo.NpGraph(g, c, o); P.drop_nan(); P.finalize()
    Hp, bp = P.build(1e-6)
    G = fr.FixedNpGraph(g, c, o, flags); G.drop_nan(); G.finalize()
    H, b = G.build(1e-6)
    # a SLAM graph of synth.make_graph has one fixed camera (0): the inactive edges are the fixed ellipsoids' gravity priors and
    # their observations from camera 0; both only ever touched the deleted rows
    assert G.inactive_edges
    assert all(e[0] == "grav" or (e[0] in ("bbox", "e3d") and e[1] == 0) for e in G.inactive_edges)
    assert sum(e[0] == "grav" for e in G.inactive_edges) == 2
    assert all(flags[e[2]] for e in G.inactive_edges)
    keep = np.ones(P.n, bool)
    for ob in fixed:
        keep[P.idx_o[ob]:P.idx_o[ob] + 9] = False
    assert G.n == keep.sum() == P.n - 18
    assert G.idx_c == P.idx_c
    assert np.array_equal(H, Hp[np.ix_(keep, keep)]) and np.array_equal(b, bp[keep])
    # chi2 drops by exactly the inactive edges' share
    share = 0.0
    for e in G.inactive_edges:
        r = G.residual(e)
        share += r @ (e[4] * r)
    assert share > 0
    assert abs(G.chi2() - (P.chi2() - share)) <= 1e-12 * P.chi2()   # (the same terms, summed in another order)
    # an anchored edge (fixed ellipsoid, free camera) has the camera block alone
    anch = [e for e in G.edges if e[0] != "odom" and flags[e[2]]]
    assert anch and all(e[1] > 0 for e in anch)
    js = G.jacobians(anch[0], 1e-6)
    assert len(js) == 1 and js[0][0] == G.idx_c[anch[0][1]] and js[0][1].shape[1] == 6
    # fixed ellipsoids do not move
    before = [(T.copy(), s.copy()) for (T, s) in G.objs]
    G.apply(np.full(G.n, 1e-3))
    for ob in range(g.n_objs):
        same = np.array_equal(before[ob][0], G.objs[ob][0]) and np.array_equal(before[ob][1], G.objs[ob][1])
        assert same == bool(flags[ob])


def known_answer_graph(pkg, odometry=True):
    """cameras of a 12-frame loop perturbed by 2 cm / 0.5 degrees, the map (8 ellipsoids) exact and fixed, exact boxes"""
    g, c, o, truth = pkg.synth.make_graph(12, 8, 400, seed=3, slam=True, frac_3d=0.0)
    bb, _, _ = pkg.synth.project_bboxes(truth["cams"], truth["objs"], g.K, g.bbox_cam, g.bbox_obj)
    kw = dict(odom_i=g.odom_i, odom_j=g.odom_j, odom_meas=g.odom_meas) if odometry else {}
    g2 = pkg.Graph(g.K, g.n_cams, g.n_objs, g.cam_fixed, g.bbox_cam, g.bbox_obj, bb, g.bbox_weight, grav_obj=g.grav_obj,
                   grav_normal=g.grav_normal, grav_weight=g.grav_weight, **kw)
    return g2, c, truth["objs"].copy(), truth


def test_known_answer_localisation(pkg):
    g, c, o, truth = known_answer_graph(pkg)
    ones = np.ones(g.n_objs, np.uint8)
    e0 = cam_err(c, truth["cams"])
    co, oo, rep = fr.optimize(g, c, o, obj_fixed=ones, delta=1e-6)
    e1 = cam_err(co, truth["cams"])
    print("localisation, 12 cameras: worst camera error %.3g -> %.3g in %d iterations, trials %s, chi2 %.3g" % (
        e0, e1, rep["iterations"], [t[2] for t in rep["trace"]], rep["chi2_final"]))
    assert e0 > 1e-2      # the start is off by centimetres
    assert e1 < 1e-4      # measured: 5.7e-6
    np.testing.assert_allclose(oo, o, rtol=0, atol=1e-15)   # the map did not move (the 10-vector round trip renormalises the quaternion)


def test_known_answer_without_odometry(pkg):
    """no odometry: every camera stands alone; camera 11, which sees no box, is not part of the system and stays where it was"""
    g, c, o, truth = known_answer_graph(pkg, odometry=False)
    assert 11 not in set(g.bbox_cam.tolist())
    ones = np.ones(g.n_objs, np.uint8)
    co, _, rep = fr.optimize(g, c, o, obj_fixed=ones, delta=1e-6)
    e11 = cam_err(co[11:12], truth["cams"][11:12])
    rest = cam_err(co[:11], truth["cams"][:11])
    print("localisation without odometry: camera 11 error %.3g, the others %.3g" % (e11, rest))
    assert cam_err(co[11:12], c[11:12]) < 1e-15 and e11 > 1e-2   # measured: 0.0297
    assert rest < 1e-4


def test_public_surface(pkg):
    L = pkg.lib.load()
    for s in ("esl_graph_upload_fixed", "esl_optimize_fixed", "esl_graph_obj_fixed"):
        assert hasattr(L, s), s
    assert "obj_fixed" in inspect.signature(pkg.Context.upload_graph).parameters
    assert "obj_fixed" in inspect.signature(pkg.Context.optimize).parameters
    assert inspect.signature(pkg.Context.upload_graph).parameters["obj_fixed"].default is None
    assert inspect.signature(pkg.Context.optimize).parameters["obj_fixed"].default is None
    assert hasattr(pkg.Context, "graph_obj_fixed")
    assert pkg.abi.SOLVER_CAMERA_CHAIN == 3
    assert L.esl_abi_version() == 5
