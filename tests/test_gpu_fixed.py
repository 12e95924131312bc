"""Fixed ellipsoid vertices on the device (esl_graph_upload_fixed / esl_optimize_fixed, ESL_SOLVER_CAMERA_CHAIN) against the numpy
reference tests/fixed_ref.py.  Every tolerance is one the suite already uses for the same kind of comparison (quoted where used)."""
import numpy as np
import pytest

from tests import fixed_ref as fr
from tests.test_gpu_slam import cam_err, obj_rel
from tests.test_gpu_robust import unpack9
from tests.test_fixed_ref import known_answer_graph

pytestmark = pytest.mark.gpu

STATUS_INVALID, STATUS_STATE = 2, 4


def every_other(g):
    f = np.zeros(g.n_objs, np.uint8)
    f[::2] = 1
    return f


def run_resident(cx, g, c, o, p, obj_fixed=None, flagged_call=True):
    if flagged_call:
        cx.upload_graph(g, obj_fixed=obj_fixed)
    else:
        cx.upload_graph(g)
    cx.upload_states(c, o)
    rep = cx.optimize_resident(p)
    cc, oo = cx.download_states()
    return cc, oo, rep


def assert_fixed_untouched(o_in, o_out, flags):
    fx = np.asarray(flags) != 0
    assert np.array_equal(np.asarray(o_out)[fx], np.asarray(o_in, dtype=np.float64).reshape(-1, 10)[fx])


def assert_matches_ref(rg, cg, og, ref, flags):
    """the LM-run tolerances of test_slam_lm_matches_faithful_dense_oracle (tests/test_gpu_slam.py:94-100)"""
    co, oo, ro = ref
    tr = ro["trace"]
    n = min(len(rg["trace_chi2"]), len(tr))
    assert rg["trace_trials"][:n] == [t[2] for t in tr][:n]
    np.testing.assert_allclose(rg["trace_chi2"][:n], [t[0] for t in tr][:n], rtol=5e-7)
    assert cam_err(cg, co) < 5e-6
    free = np.asarray(flags) == 0
    np.testing.assert_allclose(og[free, :3], oo[free, :3], atol=2e-6)
    np.testing.assert_allclose(og[free, 7:], oo[free, 7:], rtol=1e-6)


# ---- 1. off means off -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jac", [0, 1])
@pytest.mark.parametrize("slam", [False, True])
def test_off_means_off(pkg, ctx, slam, jac):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=slam)
    p = pkg.default_lm_params(jacobian_mode=jac, numeric_delta=1e-6)
    base = run_resident(ctx, g, c, o, p, flagged_call=False)
    for flags in (None, np.zeros(g.n_objs, np.uint8)):
        cc, oo, rep = run_resident(ctx, g, c, o, p, obj_fixed=flags)
        assert np.array_equal(cc, base[0]) and np.array_equal(oo, base[1])
        assert rep == base[2]
        assert not ctx.graph_obj_fixed().any()
    cc, oo, rep = ctx.optimize(g, c, o, p, obj_fixed=np.zeros(g.n_objs, np.uint8))
    assert np.array_equal(cc, base[0]) and np.array_equal(oo, base[1]) and rep == base[2]


# ---- 3. mapping mode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jac", [0, 1])
def test_mapping_subset_fixed_equals_graph_without_their_edges(pkg, ctx, jac):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3)
    flags = every_other(g)
    p = pkg.default_lm_params(jacobian_mode=jac, numeric_delta=1e-6)
    cc, oo, rep = run_resident(ctx, g, c, o, p, obj_fixed=flags)
    assert np.array_equal(ctx.graph_obj_fixed(), flags)
    assert_fixed_untouched(o, oo, flags)
    c2, o2, rep2 = run_resident(ctx, fr.without_edges_of(g, flags), c, o, p, flagged_call=False)
    # the reordering tolerances of test_sparse_interior_rows_on_awkward_structures (tests/test_gpu_slam.py:484-487)
    assert rep["trace_trials"] == rep2["trace_trials"]
    np.testing.assert_allclose(rep["trace_chi2"], rep2["trace_chi2"], rtol=1e-10)
    free = flags == 0
    assert obj_rel(oo[free], o2[free]) < 1e-8
    assert rep["n_bbox_valid"] == rep2["n_bbox_valid"] and rep["n_bbox_dropped"] == rep2["n_bbox_dropped"]
    assert np.array_equal(cc, c)


def test_mapping_all_fixed_has_nothing_to_optimise(pkg, ctx):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3)
    ones = np.ones(g.n_objs, np.uint8)
    cc, oo, rep = ctx.optimize(g, c, o, pkg.default_lm_params(), obj_fixed=ones)
    assert rep["stop_reason"] == 3 and rep["iterations"] == 0
    assert np.array_equal(cc, c) and np.array_equal(oo, o)


# ---- 4. SLAM mode: linearisation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jac,delta,tol", [(0, 1e-6, 5e-6), (1, 1e-6, 5e-6)])   # the forms of test_slam_linearisation_matches_oracle
def test_slam_linearisation_with_subset_fixed(pkg, ctx, jac, delta, tol):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=True)
    flags = every_other(g)
    G = fr.FixedNpGraph(g, c, o, flags); G.drop_nan(); G.finalize()
    H, b = G.build(1e-6)
    chi = G.chi2()
    ctx.upload_graph(g, obj_fixed=flags); ctx.upload_states(c, o)
    nv, nd = ctx.lm_begin(pkg.default_lm_params(jacobian_mode=jac, numeric_delta=delta))
    assert nv == sum(e[0] == "bbox" for e in G.edges) and nd == 0
    part = ctx.lm_linearize()
    assert part.chi2 == pytest.approx(chi, rel=1e-9)
    free = [i for i in range(g.n_cams) if not g.cam_fixed[i]]
    nf = len(free)
    Hcc = ctx.lm_download(3, nf * 36).reshape(nf, 6, 6)
    bc = ctx.lm_download(4, nf * 6).reshape(nf, 6)
    for s, ci in enumerate(free):
        i = G.idx_c[ci]
        assert i == 6 * s
        np.testing.assert_allclose(Hcc[s], H[i:i + 6, i:i + 6], atol=tol * np.abs(H[i:i + 6, i:i + 6]).max())
        np.testing.assert_allclose(bc[s], b[i:i + 6], atol=tol * max(np.abs(b[i:i + 6]).max(), 1.0))
    Hoo = ctx.lm_download(0, g.n_objs * 45).reshape(g.n_objs, 45)
    bo = ctx.lm_download(1, g.n_objs * 9).reshape(g.n_objs, 9)
    for ob in range(g.n_objs):
        if flags[ob]:
            assert not Hoo[ob].any() and not bo[ob].any()   # exactly zero
            continue
        i = G.idx_o[ob]
        Href = H[i:i + 9, i:i + 9]
        np.testing.assert_allclose(unpack9(Hoo[ob]), Href, atol=tol * np.abs(Href).max())
        np.testing.assert_allclose(bo[ob], b[i:i + 9], atol=tol * max(np.abs(b[i:i + 9]).max(), 1.0))
    assert part.max_diag == pytest.approx(np.abs(np.diag(H)).max(), rel=1e-5)
    with pytest.raises(pkg.EslError, match="esl_status %d" % STATUS_STATE):
        ctx.lm_download(9, (len(g.bbox_cam) + len(g.e3d_cam)) * 54)
    # a trial step on the step API: the fixed ellipsoids' x_o is zero, their trial states are the states
    tr = ctx.lm_try_step(1e-5 * part.max_diag)
    assert tr.solve_ok == 1
    xo = ctx.lm_download(2, g.n_objs * 9).reshape(g.n_objs, 9)
    ot = ctx.lm_download(7, g.n_objs * 10).reshape(g.n_objs, 10)
    assert not xo[flags != 0].any()
    assert_fixed_untouched(o, ot, flags)
    ctx.lm_commit(False)


# ---- 5. SLAM mode: LM run with a subset fixed -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slam_subset_ref(pkg):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=True)
    flags = every_other(g)
    return g, c, o, flags, fr.optimize(g, c, o, obj_fixed=flags, delta=1e-6)


@pytest.mark.parametrize("solver", [0, 1, 2])
@pytest.mark.parametrize("jac", [0, 1])
def test_slam_lm_with_subset_fixed_matches_reference(pkg, ctx, slam_subset_ref, jac, solver):
    g, c, o, flags, ref = slam_subset_ref
    cg, og, rg = ctx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=jac, numeric_delta=1e-6, linear_solver=solver), obj_fixed=flags)
    assert ctx.lm_solver_used() in ((1, 2) if solver == 0 else (solver,))   # free cameras see free ellipsoids: never the chain
    assert_fixed_untouched(o, og, flags)
    assert np.array_equal(cg[0], c[0])
    assert_matches_ref(rg, cg, og, ref, flags)


# ---- 6. localisation: all ellipsoids fixed --------------------------------------------------------------------------------
def test_localisation_matches_reference(pkg, ctx):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=True)
    ones = np.ones(g.n_objs, np.uint8)
    ref = fr.optimize(g, c, o, obj_fixed=ones, delta=1e-6)
    for jac in (0, 1):
        cg, og, rg = ctx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=jac, numeric_delta=1e-6), obj_fixed=ones)
        assert ctx.lm_solver_used() == 3     # AUTO resolves to the camera chain
        assert np.array_equal(og, o)
        assert_matches_ref(rg, cg, og, ref, ones)


def strip_odometry(pkg, g):
    return pkg.Graph(g.K, g.n_cams, g.n_objs, g.cam_fixed, g.bbox_cam, g.bbox_obj, g.bbox_meas, g.bbox_weight, g.e3d_cam, g.e3d_obj,
                     g.e3d_meas, g.e3d_weight, g.grav_obj, g.grav_normal, g.grav_weight)


@pytest.mark.parametrize("odometry", [True, False])
@pytest.mark.parametrize("n_cams", [60, 129, 200])   # 129, 200: test_nested_dissection_equals_plain_chain's sizes
def test_camera_chain_equals_reduced_camera_system(pkg, ctx, n_cams, odometry):
    """solver 3 against solver 1 on the same localisation graph: the same linear system, another factorisation
    (tolerances of test_nested_dissection_equals_plain_chain, tests/test_gpu_slam.py:373-374)"""
    g, c, o, _ = pkg.synth.make_graph(n_cams, 12, 12 * n_cams, seed=31, slam=True)
    if not odometry:
        g = strip_odometry(pkg, g)
    ones = np.ones(g.n_objs, np.uint8)
    runs = {}
    for solver in (3, 1):
        cg, og, rg = ctx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=solver), obj_fixed=ones)
        assert ctx.lm_solver_used() == solver and np.array_equal(og, o)
        runs[solver] = (cg, rg)
    print("n_cams %d odometry %s: chain vs reduced camera system: chi2 trace rel %.2e, cams %.2e" % (
        n_cams, odometry, float(np.abs(np.array(runs[3][1]["trace_chi2"]) / np.array(runs[1][1]["trace_chi2"]) - 1).max()),
        cam_err(runs[3][0], runs[1][0])))
    assert runs[3][1]["trace_trials"] == runs[1][1]["trace_trials"]
    np.testing.assert_allclose(runs[3][1]["trace_chi2"], runs[1][1]["trace_chi2"], rtol=1e-11)
    assert cam_err(runs[3][0], runs[1][0]) < 1e-9


def test_c3_camera_chain_equals_reduced_camera_system(pkg, ctx):
    g, c, o, _ = pkg.synth.make_config("C3", seed=0, slam=True)
    ones = np.ones(g.n_objs, np.uint8)
    runs = {}
    for solver in (3, 1):
        cg, og, rg = ctx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=solver), obj_fixed=ones)
        assert ctx.lm_solver_used() == solver and np.array_equal(og, o)
        runs[solver] = (cg, rg)
    assert runs[3][1]["trace_trials"] == runs[1][1]["trace_trials"]
    np.testing.assert_allclose(runs[3][1]["trace_chi2"], runs[1][1]["trace_chi2"], rtol=1e-11)
    assert cam_err(runs[3][0], runs[1][0]) < 1e-9


@pytest.mark.parametrize("odometry", [True, False])
def test_known_answer_localisation_on_device(pkg, ctx, odometry):
    g, c, o, truth = known_answer_graph(pkg, odometry=odometry)
    ones = np.ones(g.n_objs, np.uint8)
    co, _, _ = fr.optimize(g, c, o, obj_fixed=ones, delta=1e-6)
    cg, og, rg = ctx.optimize(g, c, o, pkg.default_lm_params(numeric_delta=1e-6), obj_fixed=ones)
    assert ctx.lm_solver_used() == 3 and np.array_equal(og, o)
    seen = slice(0, 12) if odometry else slice(0, 11)
    e_gpu, e_ref = cam_err(cg[seen], truth["cams"][seen]), cam_err(co[seen], truth["cams"][seen])
    print("known answer (odometry %s): camera error device %.3g, reference %.3g" % (odometry, e_gpu, e_ref))
    assert e_gpu < 1e-4 and e_gpu < 10 * e_ref
    if not odometry:   # camera 11 sees no box: not part of the system
        assert np.array_equal(cg[11], np.asarray(c)[11])


# ---- 7. applicability -----------------------------------------------------------------------------------------------------
def test_camera_chain_applicability(pkg, ctx):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=True)
    p3 = pkg.default_lm_params(jacobian_mode=1, linear_solver=3)
    with pytest.raises(pkg.EslError, match="esl_status %d" % STATUS_INVALID):   # a free camera sees a free ellipsoid
        ctx.optimize(g, c, o, p3, obj_fixed=every_other(g))
    with pytest.raises(pkg.EslError, match="esl_status %d" % STATUS_INVALID):
        ctx.optimize(g, c, o, p3)
    # an unflagged graph whose W happens to be empty: every ellipsoid is seen by the fixed camera 0 only
    k2, k3 = g.bbox_cam == 0, g.e3d_cam == 0
    gw = pkg.Graph(g.K, g.n_cams, g.n_objs, g.cam_fixed, g.bbox_cam[k2], g.bbox_obj[k2], g.bbox_meas.reshape(-1, 4)[k2], g.bbox_weight[k2],
                   g.e3d_cam[k3], g.e3d_obj[k3], g.e3d_meas.reshape(-1, 10)[k3], g.e3d_weight[k3], g.grav_obj, g.grav_normal, g.grav_weight,
                   g.odom_i, g.odom_j, g.odom_meas)
    assert k2.sum() > 0
    c3_, o3_, r3 = ctx.optimize(gw, c, o, p3)
    assert ctx.lm_solver_used() == 3
    c1_, o1_, r1 = ctx.optimize(gw, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=1))
    assert r3["trace_trials"] == r1["trace_trials"]
    np.testing.assert_allclose(r3["trace_chi2"], r1["trace_chi2"], rtol=1e-11)
    assert cam_err(c3_, c1_) < 1e-9 and obj_rel(o3_, o1_) < 1e-9
    # AUTO never reports 3 on an unflagged graph, whether the chain would apply or not
    for gg in (g, gw):
        ctx.optimize(gg, c, o, pkg.default_lm_params(jacobian_mode=1))
        assert ctx.lm_solver_used() in (1, 2)


# ---- 8. robust kernels and the per-edge query -----------------------------------------------------------------------------
def test_huber_on_anchored_edges_matches_reference(pkg, ctx):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=True)
    flags = every_other(g)
    from tests import robust_ref as rr
    robust = {"bbox": ("huber", float(np.sqrt(np.median(rr.edge_chi2(g, c, o, "bbox")[0]))))}
    ref = fr.optimize(g, c, o, obj_fixed=flags, robust=robust, delta=1e-6)
    ctx.set_robust(**robust)
    try:
        for jac in (0, 1):
            cg, og, rg = ctx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=jac, numeric_delta=1e-6), obj_fixed=flags)
            assert_fixed_untouched(o, og, flags)
            assert_matches_ref(rg, cg, og, ref, flags)
    finally:
        ctx.set_robust()


def test_edge_chi2_on_shuffled_flagged_graph(pkg, ctx):
    g0, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=True)
    rng = np.random.default_rng(7)
    pb, pe, pg = rng.permutation(len(g0.bbox_cam)), rng.permutation(len(g0.e3d_cam)), rng.permutation(len(g0.grav_obj))
    g = pkg.Graph(g0.K, g0.n_cams, g0.n_objs, g0.cam_fixed, g0.bbox_cam[pb], g0.bbox_obj[pb], g0.bbox_meas.reshape(-1, 4)[pb], g0.bbox_weight[pb],
                  g0.e3d_cam[pe], g0.e3d_obj[pe], g0.e3d_meas.reshape(-1, 10)[pe], g0.e3d_weight[pe], g0.grav_obj[pg], g0.grav_normal,
                  g0.grav_weight, g0.odom_i, g0.odom_j, g0.odom_meas)
    flags = every_other(g)
    from tests import robust_ref as rr
    robust = {"bbox": ("huber", float(np.sqrt(np.median(rr.edge_chi2(g, c, o, "bbox")[0])))),
              "e3d": ("cauchy", float(np.sqrt(np.median(rr.edge_chi2(g, c, o, "e3d")[0]))))}
    ctx.set_robust(**robust)
    try:
        ctx.upload_graph(g, obj_fixed=flags); ctx.upload_states(c, o)
        ctx.lm_begin(pkg.default_lm_params())
        for cls in ("bbox", "e3d", "grav", "odom"):
            chi, w = ctx.edge_chi2(cls)
            chi_ref, w_ref = fr.edge_chi2(g, c, o, cls, obj_fixed=flags, robust=robust)
            np.testing.assert_allclose(chi, chi_ref, rtol=1e-9, atol=1e-12)   # (the tolerances of test_gpu_robust.py's edge_chi2 test)
            np.testing.assert_allclose(w, w_ref, rtol=1e-9)
            if cls != "odom":
                assert (w == 0).sum() >= 1 and (w_ref == 0).sum() == (w == 0).sum()
    finally:
        ctx.set_robust()


# ---- 9. bitwise reproducible ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("all_fixed", [False, True])
def test_flagged_slam_runs_are_bitwise_reproducible(pkg, ctx, all_fixed):
    g, c, o, _ = pkg.synth.make_graph(60, 10, 600, seed=9, slam=True)
    flags = np.ones(g.n_objs, np.uint8) if all_fixed else every_other(g)
    p = pkg.default_lm_params(jacobian_mode=1)
    a = ctx.optimize(g, c, o, p, obj_fixed=flags)
    b = ctx.optimize(g, c, o, p, obj_fixed=flags)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- 10. state rules ------------------------------------------------------------------------------------------------------
def test_state_rules(pkg, ctx):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=True)
    flags = every_other(g)
    p = pkg.default_lm_params(jacobian_mode=1)
    ctx.upload_graph(g, obj_fixed=flags); ctx.upload_states(c, o)
    assert np.array_equal(ctx.graph_obj_fixed(), flags)
    with pytest.raises(pkg.EslError, match="esl_status %d" % STATUS_STATE):
        ctx.append_graph(new_cams=c[:1], new_cam_fixed=[1])
    # the flags survive a states upload, snapshot / restore and a trim
    ctx.snapshot_states()
    r1 = ctx.optimize_resident(p)
    ctx.restore_states()
    ctx.trim()
    assert np.array_equal(ctx.graph_obj_fixed(), flags)
    r2 = ctx.optimize_resident(p)
    assert r1 == r2
    ctx.upload_states(c, o)
    assert np.array_equal(ctx.graph_obj_fixed(), flags)
    r3 = ctx.optimize_resident(p)
    assert r3 == r1
    assert_fixed_untouched(o, ctx.download_states()[1], flags)
    # bad arguments
    import ctypes as C
    L = pkg.lib.load()
    buf = np.zeros(g.n_objs + 1, np.uint8)
    assert L.esl_graph_obj_fixed(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int32(g.n_objs + 1)) == STATUS_INVALID
    assert L.esl_graph_upload_fixed(ctx._h, None, buf.ctypes.data_as(C.POINTER(C.c_uint8))) == STATUS_INVALID
    # entries other than 0 / 1 count as 1
    ctx.upload_graph(g, obj_fixed=flags * 7)
    assert np.array_equal(ctx.graph_obj_fixed(), flags)
    # a plain upload clears the flags and runs as today
    base = pkg.Context(0)
    try:
        want = run_resident(base, g, c, o, p, flagged_call=False)
    finally:
        base.close()
    got = run_resident(ctx, g, c, o, p, flagged_call=False)
    assert not ctx.graph_obj_fixed().any()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_flags_refused_under_a_communicator(pkg):
    g, c, o, _ = pkg.synth.make_graph(20, 5, 60, seed=3, slam=True)
    cx = pkg.Context(0)
    try:
        cx.comm_init_host(1, 0, lambda buf: None)   # one rank: the sum over the ranks is the buffer itself
        with pytest.raises(pkg.EslError, match="esl_status %d" % STATUS_STATE):
            cx.upload_graph(g, obj_fixed=every_other(g))
        cx.upload_graph(g, obj_fixed=np.zeros(g.n_objs, np.uint8))   # no flag set: an ordinary upload
        cx.upload_graph(g)
    finally:
        cx.close()


# ---- 11. full size --------------------------------------------------------------------------------------------------------
def test_c4_localisation_runs_on_the_chain_without_a_dense_system(pkg):
    """BASELINE configs[3] (10,000 cameras, 2,000 ellipsoids), every ellipsoid fixed at its initial state: a property check like
    those of tests/test_gpu_fullsize.py (no CPU reference reaches this size).  The order-59,994 reduced camera system alone would
    be 28.8 GB; the graph and its records are well under 1 GB.  The free-memory figure is device-wide and the machine is shared,
    hence the wide gap between the two."""
    import torch
    g, c, o, _ = pkg.synth.make_config("C4", slam=True)
    ones = np.ones(g.n_objs, np.uint8)
    cx = pkg.Context(0)
    try:
        free0, _ = torch.cuda.mem_get_info(0)
        cx.upload_graph(g, obj_fixed=ones); cx.upload_states(c, o)
        rep = cx.optimize_resident(pkg.default_lm_params(jacobian_mode=1))
        free1, _ = torch.cuda.mem_get_info(0)
        cc, oo = cx.download_states()
        assert cx.lm_solver_used() == 3
        assert not any(cx.lm_solver_stats().values())
        print("C4 localisation: %d iterations, trials %s, chi2 %.6g -> %.6g, free memory dropped by %.2f GB" % (
            rep["iterations"], rep["trace_trials"], rep["chi2_initial"], rep["chi2_final"], (free0 - free1) / 1e9))
        assert rep["iterations"] >= 1 and np.isfinite(rep["chi2_final"])
        tr = [rep["chi2_initial"]] + list(rep["trace_chi2"])
        assert all(b <= a for a, b in zip(tr, tr[1:]))
        assert free0 - free1 < 20e9
        assert np.array_equal(oo, o) and np.array_equal(cc[0], c[0])
    finally:
        cx.close()
