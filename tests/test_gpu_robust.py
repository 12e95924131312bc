"""Robust kernels on the device (esl_lm_set_robust / esl_edge_chi2): the weighted linearisation against the C oracle of the
reweighted graph, whole LM runs against tests/robust_ref.py, 'off is off' and the per-edge query."""
import copy

import numpy as np
import pytest

from tests import robust_ref as rr

pytestmark = pytest.mark.gpu


def unpack9(p):
    H = np.zeros((9, 9))
    k = 0
    for a in range(9):
        for c in range(a, 9):
            H[a, c] = H[c, a] = p[k]
            k += 1
    return H


def widths(g, c, o, classes):
    """delta per class = sqrt(median raw chi2): both branches of every kernel are taken"""
    return {k: float(np.sqrt(np.median(rr.edge_chi2(g, c, o, k)[0]))) for k in classes}


def reweighted(g, c, o, robust):
    """the graph with each edge's information scaled by rho1(e) of its raw chi2 at (c, o), and sum rho0"""
    g2 = copy.copy(g)
    tot = 0.0
    for cls, attr in (("bbox", "bbox_weight"), ("e3d", "e3d_weight")):
        e, w = rr.edge_chi2(g, c, o, cls, robust)
        k = robust.get(cls)
        tot += sum(rr.robustify(k[0], k[1], x)[0] if k else x for x in e)
        setattr(g2, attr, getattr(g, attr) * w)
    if len(g.odom_i):
        e, w = rr.edge_chi2(g, c, o, "odom", robust)
        k = robust.get("odom")
        tot += sum(rr.robustify(k[0], k[1], x)[0] if k else x for x in e)
        info = np.ones((len(g.odom_i), 6)) if g.odom_info is None else g.odom_info.reshape(-1, 6)
        g2.odom_info = np.ascontiguousarray(info * w[:, None])
    tot += sum(rr.edge_chi2(g, c, o, "grav")[0])
    return g2, tot


KIND_SETS = [("huber", "cauchy", "tukey"), ("pseudo_huber", "tukey", "huber"), ("cauchy", "huber", "pseudo_huber"), ("tukey", "pseudo_huber", "cauchy")]


@pytest.mark.parametrize("kinds", KIND_SETS)
@pytest.mark.parametrize("jac,tol", [(0, 5e-6), (1, 5e-6)])   # the oracle differentiates numerically (as test_gpu_slam.py)
@pytest.mark.parametrize("slam", [False, True])
def test_robust_linearisation_matches_reweighted_oracle(pkg, po, ctx, slam, jac, tol, kinds):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=slam)
    dl = widths(g, c, o, ["bbox", "e3d"] + (["odom"] if slam else []))
    robust = {cls: (k, dl[cls]) for cls, k in zip(("bbox", "e3d", "odom"), kinds) if cls in dl}
    g2, chi_ref = reweighted(g, c, o, robust)
    H, b, fidx, _ = po.build_system(g2, c, o, delta=1e-6)
    ctx.upload_graph(g); ctx.upload_states(c, o)
    ctx.set_robust(**robust)
    try:
        ctx.lm_begin(pkg.default_lm_params(jacobian_mode=jac, numeric_delta=1e-6))
        part = ctx.lm_linearize()
        assert part.chi2 == pytest.approx(chi_ref, rel=1e-9)
        assert part.max_diag == pytest.approx(np.abs(np.diag(H)).max(), rel=1e-5)
        Hoo = ctx.lm_download(0, g.n_objs * 45).reshape(g.n_objs, 45)
        bo = ctx.lm_download(1, g.n_objs * 9).reshape(g.n_objs, 9)
        for ob in range(g.n_objs):
            i = fidx[g.n_cams + ob]
            Href = H[i:i + 9, i:i + 9]
            np.testing.assert_allclose(unpack9(Hoo[ob]), Href, atol=tol * np.abs(Href).max())
            np.testing.assert_allclose(bo[ob], b[i:i + 9], atol=tol * max(np.abs(b[i:i + 9]).max(), 1.0))
        if slam:
            nf = int((~g.cam_fixed.astype(bool)).sum())
            Hcc = ctx.lm_download(3, nf * 36).reshape(nf, 6, 6)
            bc = ctx.lm_download(4, nf * 6).reshape(nf, 6)
            free = [i for i in range(g.n_cams) if not g.cam_fixed[i]]
            for s, ci in enumerate(free):
                i = fidx[ci]
                np.testing.assert_allclose(Hcc[s], H[i:i + 6, i:i + 6], atol=tol * np.abs(H[i:i + 6, i:i + 6]).max())
                np.testing.assert_allclose(bc[s], b[i:i + 6], atol=tol * max(np.abs(b[i:i + 6]).max(), 1.0))
            # the W blocks carry the weight into the camera side: the reduced camera system equals the reweighted oracle's
            lam = 1e-5 * part.max_diag
            _, n, lda = ctx.lm_reduced_system(lam)
            from tests.test_gpu_slam import lower_to_full
            S, _ = lower_to_full(ctx.lm_download(6, lda * n), n, lda)
            Hl = H + lam * np.eye(len(b))
            S_ref = Hl[:n, :n] - Hl[:n, n:] @ np.linalg.solve(Hl[n:, n:], Hl[:n, n:].T)
            np.testing.assert_allclose(S, S_ref, atol=tol * np.abs(S_ref).max())
    finally:
        ctx.set_robust()


@pytest.mark.parametrize("kind", ["huber", "pseudo_huber", "cauchy", "tukey"])
@pytest.mark.parametrize("slam", [False, True])
def test_robust_gravity_linearisation_matches_reference(pkg, ctx, slam, kind):
    """the merged gravity prior (count * rho(grav_w r^2), weight count * grav_w * rho1): H, b and chi2 against robust_ref's
    per-edge build, at the start state and after a damped step (the trial chi2 / step kernels)"""
    g, c, o, _ = pkg.synth.make_graph(10, 4, 50, seed=6, slam=slam)
    g = pkg.Graph(g.K, g.n_cams, g.n_objs, g.cam_fixed, g.bbox_cam, g.bbox_obj, g.bbox_meas, g.bbox_weight, g.e3d_cam, g.e3d_obj,
                  g.e3d_meas, g.e3d_weight, np.concatenate([g.grav_obj, g.grav_obj[:2]]), g.grav_normal, g.grav_weight,
                  odom_i=g.odom_i, odom_j=g.odom_j, odom_meas=g.odom_meas)   # two ellipsoids with 2 gravity edges each
    # delta^2 halfway between two neighbouring distinct gravity chi2 values: both branches taken, no edge on the branch point itself
    # (a median falls ON an edge here -- objects 0, 1 carry two equal gravity edges -- and Tukey's rho1 ~ (1 - e / delta^2)^2 is then
    # 0 on one side and 1e-32 on the other)
    eg = np.unique(rr.edge_chi2(g, c, o, "grav")[0])
    robust = {"grav": (kind, float(np.sqrt(0.5 * (eg[len(eg) // 2 - 1] + eg[len(eg) // 2]))))}
    G = rr.RobustNpGraph(g, c, o, robust)
    G.drop_nan(); G.finalize()
    H, b = G.build(1e-6)
    ctx.upload_graph(g); ctx.upload_states(c, o)
    ctx.set_robust(**robust)
    try:
        ctx.lm_begin(pkg.default_lm_params(jacobian_mode=1))
        part = ctx.lm_linearize()
        assert part.chi2 == pytest.approx(G.chi2(), rel=1e-9)
        Hoo = ctx.lm_download(0, g.n_objs * 45).reshape(g.n_objs, 45)
        bo = ctx.lm_download(1, g.n_objs * 9).reshape(g.n_objs, 9)
        for ob in range(g.n_objs):
            i = G.idx_o[ob]
            Href = H[i:i + 9, i:i + 9]
            np.testing.assert_allclose(unpack9(Hoo[ob]), Href, atol=5e-6 * np.abs(Href).max())
            np.testing.assert_allclose(bo[ob], b[i:i + 9], atol=5e-6 * max(np.abs(b[i:i + 9]).max(), 1.0))
        tr = ctx.lm_try_step(1e-3 * part.max_diag)
        co = ctx.lm_download(8, g.n_cams * 7).reshape(-1, 7) if slam else c
        ob_ = ctx.lm_download(7, g.n_objs * 10).reshape(-1, 10)
        assert tr.chi2 == pytest.approx(rr.RobustNpGraph(g, co, ob_, robust).chi2(), rel=1e-9)
        ctx.lm_commit(False)
    finally:
        ctx.set_robust()


def run_gpu(pkg, ctx, g, c, o, p, robust):
    ctx.upload_graph(g); ctx.upload_states(c, o)
    ctx.set_robust(**robust)
    try:
        rep = ctx.optimize_resident(p)
        cams, objs = ctx.download_states()
    finally:
        ctx.set_robust()
    return cams, objs, rep


@pytest.mark.parametrize("case", ["huber_cauchy", "tukey_small"])
# chi2 traces to 1e-7 relative, not 1e-9: the reference differentiates in numpy, the device in its own order (measured gap up to
# 4e-8); the project's other LM-vs-oracle tests hold 1e-5 .. 1e-6.  Iterations and trials per iteration must be equal.
@pytest.mark.parametrize("slam,solver", [(False, 0), (True, 1), (True, 2)])
def test_robust_lm_matches_reference(pkg, ctx, slam, solver, case):
    g, c, o, _ = pkg.synth.make_graph(12, 3, 60, seed=2, slam=slam)
    if case == "huber_cauchy":
        dl = widths(g, c, o, ["bbox", "e3d", "grav"])
        robust = {"bbox": ("huber", dl["bbox"]), "e3d": ("cauchy", dl["e3d"]), "grav": ("pseudo_huber", dl["grav"])}
        if slam:
            robust["odom"] = ("huber", 1e-3)
    else:
        # Tukey with a width below every box edge of ellipsoid 0: that ellipsoid's boxes all carry weight 0 (rho1 = 0)
        e, _ = rr.edge_chi2(g, c, o, "bbox")
        d2 = 0.5 * float(e[g.bbox_obj == 0].min())
        assert d2 < np.median(e)
        robust = {"bbox": ("tukey", float(np.sqrt(d2)))}
        _, w = rr.edge_chi2(g, c, o, "bbox", robust)
        assert np.all(w[g.bbox_obj == 0] == 0)
    p = pkg.default_lm_params(jacobian_mode=0, numeric_delta=1e-6, linear_solver=solver)
    cr, orf, rref = rr.optimize(g, c, o, robust=robust, delta=1e-6)
    cg, og, rg = run_gpu(pkg, ctx, g, c, o, p, robust)
    assert rg["iterations"] == rref["iterations"]
    assert rg["trace_trials"] == [t[2] for t in rref["trace"]]
    # numpy central differences against the device's: the traces agree to ~4e-8 relative (measured), well inside 1e-7
    np.testing.assert_allclose(rg["trace_chi2"], [t[0] for t in rref["trace"]], rtol=1e-7)
    assert np.all(np.isfinite(og)) and np.all(np.isfinite(cg))
    np.testing.assert_allclose(og, orf, rtol=1e-4, atol=1e-6)
    if slam:
        np.testing.assert_allclose(cg, cr, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("slam", [False, True])
def test_robust_off_is_off(pkg, ctx, slam):
    g, c, o, _ = pkg.synth.make_graph(120, 24, 2400, seed=7, slam=slam)
    p = pkg.default_lm_params(jacobian_mode=1, max_iters=4)
    runs = []
    for mode in ("never", "none", "reset"):
        cx = pkg.Context(0)
        try:
            if mode == "none":
                cx.set_robust(bbox=("none", 1.0), e3d=("none", 1.0), grav=("none", 1.0), odom=("none", 1.0))
            elif mode == "reset":
                cx.set_robust(bbox=("huber", 1.0))
                cx.set_robust()
            runs.append(cx.optimize(g, c, o, p))
        finally:
            cx.close()
    for r in runs[1:]:
        assert r[2]["trace_chi2"] == runs[0][2]["trace_chi2"] and r[2]["trace_trials"] == runs[0][2]["trace_trials"]
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])


def shuffled(pkg, g, seed):
    """the same graph with its bbox, 3-D, gravity and odometry edges in a random caller order (the upload sorts by ellipsoid)"""
    rng = np.random.default_rng(seed)
    pb, pe, pg, po_ = (rng.permutation(n) for n in (len(g.bbox_cam), len(g.e3d_cam), len(g.grav_obj), len(g.odom_i)))
    kw = {}
    if len(g.odom_i):
        kw = dict(odom_i=g.odom_i[po_], odom_j=g.odom_j[po_], odom_meas=g.odom_meas.reshape(-1, 7)[po_])
    return pkg.Graph(g.K, g.n_cams, g.n_objs, g.cam_fixed, g.bbox_cam[pb], g.bbox_obj[pb], g.bbox_meas.reshape(-1, 4)[pb], g.bbox_weight[pb],
                     g.e3d_cam[pe], g.e3d_obj[pe], g.e3d_meas.reshape(-1, 10)[pe], g.e3d_weight[pe], g.grav_obj[pg], g.grav_normal,
                     g.grav_weight, **kw)


@pytest.mark.parametrize("slam", [False, True])
def test_edge_chi2_in_caller_order(pkg, ctx, slam):
    g0, c, o, _ = pkg.synth.make_graph(12, 3, 60, seed=2, slam=slam)
    g = shuffled(pkg, g0, 4)
    assert np.any(np.diff(g.bbox_obj) < 0) and np.any(np.diff(g.e3d_obj) < 0)   # the upload's sort is not the identity
    robust = {"bbox": ("huber", 2.0), "e3d": ("cauchy", 1.0), "grav": ("tukey", 1.0), "odom": ("pseudo_huber", 1.0)}
    cg, og, _ = run_gpu(pkg, ctx, g, c, o, pkg.default_lm_params(jacobian_mode=1, max_iters=3), robust)
    ctx.set_robust(**robust)
    try:
        for cls in ("bbox", "e3d", "grav", "odom"):
            e, w = ctx.edge_chi2(cls)
            er, wr = rr.edge_chi2(g, cg, og, cls, robust)
            assert len(e) == len(er) == ({"bbox": len(g.bbox_cam), "e3d": len(g.e3d_cam), "grav": len(g.grav_obj), "odom": len(g.odom_i)}[cls])
            np.testing.assert_allclose(e, er, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(w, wr, rtol=1e-9)
            assert np.any(w != 1.0) or cls == "odom"
    finally:
        ctx.set_robust()
    with pytest.raises(pkg.EslError):   # count must equal the class's edge count
        L = pkg.lib
        n = np.zeros(3)
        L._check(L.load().esl_edge_chi2(ctx._h, 0, n.ctypes.data_as(L._dp), n.ctypes.data_as(L._dp), L.C.c_int64(3)), "esl_edge_chi2")


def test_edge_chi2_nan_dropped_box_has_weight_zero(pkg, ctx):
    """Optimizer.cpp:234-243: a box whose chi2 is NaN at the start state is dropped; the query reports it with weight 0"""
    from oracle import np_oracle as npo
    g, c, o, _ = pkg.synth.make_graph(40, 6, 300, seed=7)
    c = c.copy(); Rt = o[0, :3]
    T = npo.T_from7(c[3]); T[:3, 3] = -T[:3, :3] @ (Rt + 0.01); c[3] = npo.T_to7(T)   # camera 3 inside ellipsoid 0: NaN
    k = 17   # caller position of the NaN edge
    bc, bo = np.insert(g.bbox_cam, k, 3), np.insert(g.bbox_obj, k, 0)
    bm = np.insert(g.bbox_meas.reshape(-1, 4), k, [100, 100, 200, 200], axis=0)
    bw = np.insert(g.bbox_weight, k, 0.8)
    extra = shuffled(pkg, pkg.Graph(g.K, g.n_cams, g.n_objs, None, bc, bo, bm, bw, g.e3d_cam, g.e3d_obj, g.e3d_meas, g.e3d_weight,
                                    g.grav_obj, g.grav_normal, g.grav_weight), 1)
    for robust in ({}, {"bbox": ("huber", 1.0)}):
        _, og, rep = run_gpu(pkg, ctx, extra, c, o, pkg.default_lm_params(jacobian_mode=1), robust)
        assert rep["n_bbox_dropped"] >= 1
        ctx.set_robust(**robust)
        try:
            e, w = ctx.edge_chi2("bbox")
        finally:
            ctx.set_robust()
        er, wr = rr.edge_chi2(extra, c, og, "bbox", robust)
        bad = np.isnan(er)
        assert bad.sum() == rep["n_bbox_dropped"]
        assert np.all(w[bad] == 0) and np.all(np.isnan(e[bad]))
        np.testing.assert_allclose(e[~bad], er[~bad], rtol=1e-9)
        np.testing.assert_allclose(w[~bad], wr[~bad], rtol=1e-9)


def test_edge_chi2_after_append_equals_rebuilt(pkg, ctx):
    """caller order across esl_graph_append (the first append re-lays the compact upload out): the upload's edges, then each
    frame's, element by element against a context that uploaded the whole graph in that order"""
    from tests.test_gpu_streaming import slam_graph_upto
    F, N = 16, 6
    g, c, o, _ = pkg.synth.make_graph(F, N, 14 * F, seed=9, slam=True)
    p = pkg.default_lm_params(jacobian_mode=1, max_iters=2)
    robust = {"bbox": ("huber", 1.0), "e3d": ("cauchy", 1.0), "odom": ("cauchy", 1.0)}
    f0 = 4
    g_up = slam_graph_upto(pkg, g, f0)
    ctx.upload_graph(g_up); ctx.upload_states(c[:f0 + 1], o)
    ctx.set_robust(**robust)
    ref = pkg.Context(0)
    ref.set_robust(**robust)
    order = {"bbox": [np.nonzero(g.bbox_cam <= f0)[0]], "e3d": [np.nonzero(g.e3d_cam <= f0)[0]], "odom": [np.nonzero(g.odom_j <= f0)[0]]}
    assert len(order["bbox"][0]) == len(g_up.bbox_cam) and np.array_equal(g.bbox_cam[order["bbox"][0]], g_up.bbox_cam)
    try:
        for f in range(f0 + 1, f0 + 4):
            mb, me, mo = g.bbox_cam == f, g.e3d_cam == f, g.odom_j == f
            ctx.append_graph(new_cams=c[f:f + 1], new_cam_fixed=[0],
                             bbox=(g.bbox_cam[mb], g.bbox_obj[mb], g.bbox_meas.reshape(-1, 4)[mb], g.bbox_weight[mb]),
                             e3d=(g.e3d_cam[me], g.e3d_obj[me], g.e3d_meas.reshape(-1, 10)[me], g.e3d_weight[me]),
                             odom=(g.odom_i[mo], g.odom_j[mo], g.odom_meas.reshape(-1, 7)[mo]))
            order["bbox"].append(np.nonzero(mb)[0]); order["e3d"].append(np.nonzero(me)[0]); order["odom"].append(np.nonzero(mo)[0])
            ctx.optimize_resident(p)
            cams, objs = ctx.download_states()
            # the rebuilt graph in the appended context's caller order: the upload's edges, then every frame's
            ib, ie, io = (np.concatenate(order[k]) for k in ("bbox", "e3d", "odom"))
            gr = pkg.Graph(g.K, f + 1, N, g.cam_fixed[:f + 1], g.bbox_cam[ib], g.bbox_obj[ib], g.bbox_meas.reshape(-1, 4)[ib],
                           g.bbox_weight[ib], g.e3d_cam[ie], g.e3d_obj[ie], g.e3d_meas.reshape(-1, 10)[ie], g.e3d_weight[ie],
                           g.grav_obj, g.grav_normal, g.grav_weight, odom_i=g.odom_i[io], odom_j=g.odom_j[io],
                           odom_meas=g.odom_meas.reshape(-1, 7)[io])
            ref.upload_graph(gr); ref.upload_states(cams, objs)
            for cls in ("bbox", "e3d", "odom"):
                a, b = ctx.edge_chi2(cls), ref.edge_chi2(cls)
                np.testing.assert_array_equal(a[0], b[0])   # element by element: the same edge at the same caller index
                np.testing.assert_array_equal(a[1], b[1])
                er, wr = rr.edge_chi2(gr, cams, objs, cls, robust)
                np.testing.assert_allclose(a[0], er, rtol=1e-9, atol=1e-12)
                np.testing.assert_allclose(a[1], wr, rtol=1e-9)
    finally:
        ref.close()
        ctx.set_robust()


def test_huber_rejects_displaced_boxes(pkg, ctx):
    """what the feature is for: 10 % of the boxes displaced by 60-120 px (bbox edges the only position information, 2 px noise).
    Huber (delta = 10 px) must halve the median ellipsoid-centre error and its weights must single out the displaced boxes."""
    g, c, o, truth = pkg.synth.make_graph(60, 12, 1200, seed=21, frac_3d=0.0)
    rng = np.random.default_rng(5)
    nb = len(g.bbox_cam)
    bad = rng.choice(nb, size=nb // 10, replace=False)
    bm = g.bbox_meas.reshape(-1, 4).copy()
    shift = rng.uniform(60, 120, size=(len(bad), 2)) * rng.choice([-1, 1], size=(len(bad), 2))
    bm[bad] += np.concatenate([shift, shift], 1)
    g.bbox_meas = np.ascontiguousarray(bm)
    p = pkg.default_lm_params(jacobian_mode=1)
    robust = {"bbox": ("huber", 10.0)}
    _, o_plain, _ = run_gpu(pkg, ctx, g, c, o, p, {})
    _, o_rob, _ = run_gpu(pkg, ctx, g, c, o, p, robust)
    ctx.set_robust(**robust)
    try:
        _, w = ctx.edge_chi2("bbox")
    finally:
        ctx.set_robust()
    err = lambda objs: float(np.median(np.linalg.norm(objs[:, :3] - truth["objs"][:, :3], axis=1)))
    flagged = w < 1
    clean = np.ones(nb, bool); clean[bad] = False
    # measured: median centre error 0.118 m without the kernel, 0.0115 m with it; 100 % of the displaced boxes flagged, 0 % of the clean
    assert err(o_rob) <= 0.5 * err(o_plain), (err(o_rob), err(o_plain))
    assert flagged[bad].mean() >= 0.9, flagged[bad].mean()
    assert flagged[clean].mean() <= 0.05, flagged[clean].mean()


def _robust_pkg(pkg, robust):
    """pkg whose Context carries the robust setting from creation on (the sharded helper creates its own contexts)"""
    class P:
        lib = pkg.lib

        @staticmethod
        def Context(dev=0):
            cx = pkg.Context(dev)
            cx.set_robust(**robust)
            return cx
    return P


def test_mapping_two_shards_robust_match_single_context(pkg, ctx):
    from tests.test_gpu_sharded import run_sharded
    g, c, o, _ = pkg.synth.make_graph(40, 10, 400, seed=11)
    robust = {"bbox": ("huber", 2.0), "odom": ("huber", 1.0)}
    p = pkg.default_lm_params(jacobian_mode=1)
    _, ro, ref = run_gpu(pkg, ctx, g, c, o, p, robust)
    _, ro_plain, _ = run_gpu(pkg, ctx, g, c, o, p, {})
    assert np.abs(ro - ro_plain).max() > 1e-6   # the kernel changes the answer
    reps, cams, objs, ar = run_sharded(_robust_pkg(pkg, robust), g, c, o, p)
    for rep in reps:
        assert rep["iterations"] == ref["iterations"] and rep["trace_trials"] == ref["trace_trials"]
        np.testing.assert_allclose(rep["trace_chi2"], ref["trace_chi2"], rtol=1e-12)
    assert reps[0]["trace_chi2"] == reps[1]["trace_chi2"]
    np.testing.assert_allclose(objs, ro, rtol=1e-11, atol=1e-13)


def test_slam_two_shards_robust_match_single_context(pkg, ctx):
    from tests.test_gpu_sharded import run_sharded
    g, c, o, _ = pkg.synth.make_graph(30, 8, 300, seed=5, slam=True)
    robust = {"bbox": ("huber", 2.0), "odom": ("huber", 1e-3)}
    p = pkg.default_lm_params(jacobian_mode=1)
    rc, ro, ref = run_gpu(pkg, ctx, g, c, o, p, robust)
    reps, cams, objs, ar = run_sharded(_robust_pkg(pkg, robust), g, c, o, p)
    for rep in reps:
        assert rep["chi2_initial"] == pytest.approx(ref["chi2_initial"], rel=1e-12)
        np.testing.assert_allclose(rep["trace_chi2"][:2], ref["trace_chi2"][:2], rtol=1e-7)   # as test_gpu_sharded.py's SLAM test
        assert rep["chi2_final"] == pytest.approx(ref["chi2_final"], rel=1e-4)
    assert reps[0]["trace_chi2"] == reps[1]["trace_chi2"]
    np.testing.assert_array_equal(cams[0], cams[1])
    np.testing.assert_allclose(objs, ro, rtol=1e-4, atol=1e-6)
