"""ESL_SOLVER_PCG on the device: matrix-free block-Jacobi PCG on the reduced camera system against numpy's solve of the dense S the
library itself builds, against the numpy PCG of tests/pcg_ref.py (iteration counts), against the dense solvers and the CPU checker
(whole LM runs), and its settings, failure handling and refusals."""
import numpy as np
import pytest

from tests import pcg_ref as pr

pytestmark = pytest.mark.gpu


def lower_to_full(S, n, lda):
    """the reduced system as esl_lm_download(6) returns it (column-major, lower triangle, row n = b_s) -> full S, b_s"""
    M = S.reshape(n, lda).T
    L = M[:n, :n]
    return np.tril(L) + np.tril(L, -1).T, M[n, :n].copy()


def cam_err(a, b):
    from oracle import np_oracle as npo
    return max(float(np.linalg.norm(npo.se3_log(npo.T_inv(npo.T_from7(x)) @ npo.T_from7(y)))) for x, y in zip(a, b))


def obj_rel(a, b):
    return float((np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)).max())


def slam_graph_upto(pkg, g, f):
    """the SLAM-mode graph of frames 0 .. f: camera 0 fixed, one odometry edge per consecutive pair"""
    mb, me, mo = g.bbox_cam <= f, g.e3d_cam <= f, g.odom_j <= f
    return pkg.Graph(g.K, f + 1, g.n_objs, g.cam_fixed[:f + 1], g.bbox_cam[mb], g.bbox_obj[mb], g.bbox_meas.reshape(-1, 4)[mb], g.bbox_weight[mb],
                     g.e3d_cam[me], g.e3d_obj[me], g.e3d_meas.reshape(-1, 10)[me], g.e3d_weight[me], g.grav_obj, g.grav_normal, g.grav_weight,
                     g.odom_i[mo], g.odom_j[mo], g.odom_meas.reshape(-1, 7)[mo])


def offenders(pkg):
    """the recipe of tests/test_visibility.py: hand-made offenders on ellipsoid 0 -- a camera looking away, a camera inside the
    ellipsoid, a camera that sees it far outside a 640 x 480 image -- here on a SLAM-mode graph (camera 0 fixed, odometry chain)"""
    from oracle import np_fit
    g, c, o, _ = pkg.synth.make_graph(30, 6, 260, seed=21, slam=True)
    c = c.copy()
    cams = [int(k) for k in g.bbox_cam[g.bbox_obj == 0] if k != 0][:3]
    Twc = np_fit.se3_inv(c[cams[0]]); Twc[3:] = np_fit.q_mul(Twc[3:], np.array([0, 1.0, 0, 0])); c[cams[0]] = np_fit.se3_inv(Twc)
    Twc = np_fit.se3_inv(c[cams[1]]); Twc[:3] = o[0][:3] + 0.01; c[cams[1]] = np_fit.se3_inv(Twc)
    Twc = np_fit.se3_inv(c[cams[2]]); Twc[3:] = np_fit.q_mul(Twc[3:], np.array([0, np.sin(0.6), 0, np.cos(0.6)])); c[cams[2]] = np_fit.se3_inv(Twc)
    gv = pkg.Graph(g.K, g.n_cams, g.n_objs, g.cam_fixed, g.bbox_cam, g.bbox_obj, g.bbox_meas, g.bbox_weight, g.e3d_cam, g.e3d_obj, g.e3d_meas,
                   g.e3d_weight, g.grav_obj, g.grav_normal, g.grav_weight, g.odom_i, g.odom_j, g.odom_meas, g.odom_info,
                   check_visibility=1, image_rows=480, image_cols=640)
    return gv, c, o


@pytest.fixture(scope="module")
def cx(pkg):
    """a context of this module's own: the PCG and robust settings belong to the context"""
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(cx):
    yield
    cx.set_pcg()
    cx.set_robust()


def with_edges(pkg, g, mb, me, **kw):
    """g with the bbox / 3-D edges selected by the masks; kw replaces odometry arrays"""
    od = dict(odom_i=g.odom_i, odom_j=g.odom_j, odom_meas=g.odom_meas, odom_info=g.odom_info)
    od.update(kw)
    return pkg.Graph(g.K, g.n_cams, g.n_objs, g.cam_fixed, g.bbox_cam[mb], g.bbox_obj[mb], g.bbox_meas.reshape(-1, 4)[mb], g.bbox_weight[mb],
                     g.e3d_cam[me], g.e3d_obj[me], g.e3d_meas.reshape(-1, 10)[me], g.e3d_weight[me], g.grav_obj, g.grav_normal, g.grav_weight, **od)


def per_cam_counts(g):
    return np.bincount(np.concatenate([g.bbox_cam, g.e3d_cam]).astype(np.int64), minlength=g.n_cams)


def per_obj_counts(g):
    free = ~g.cam_fixed.astype(bool)
    return np.bincount(np.concatenate([g.bbox_obj[free[g.bbox_cam]], g.e3d_obj[free[g.e3d_cam]]]).astype(np.int64), minlength=g.n_objs)


def has_bbox_and_e3d_pair(g):
    bb = set(zip(g.bbox_cam.tolist(), g.bbox_obj.tolist()))
    return any((c, o) in bb and not g.cam_fixed[c] for c, o in zip(g.e3d_cam.tolist(), g.e3d_obj.tolist()))


def solve_cases(pkg):
    cases = {}
    for nc in (2, 12, 40, 100):
        cases["nc%d" % nc] = pkg.synth.make_graph(nc, 8, 10 * nc, seed=4, slam=True)[:3]
    cases["long_camera_list"] = pkg.synth.make_graph(6, 200, 2000, seed=1, slam=True, frac_3d=0.5)[:3]
    g, c, o = cases["nc40"]
    cases["odometry_only_camera"] = (with_edges(pkg, g, g.bbox_cam != 7, g.e3d_cam != 7), c, o)
    return cases


@pytest.mark.parametrize("name", ["nc2", "nc12", "nc40", "nc100", "long_camera_list", "odometry_only_camera"])
def test_pcg_solves_the_reduced_camera_system(pkg, cx, name):
    g, c, o = solve_cases(pkg)[name]
    free = ~g.cam_fixed.astype(bool)
    if name == "nc2":
        assert free.sum() == 1                                  # one free camera: no off-diagonal block
    if name == "nc100":
        assert per_obj_counts(g).max() > 64                     # an ellipsoid's list takes more than one trip of the wave
    if name == "long_camera_list":
        assert g.n_objs >= 80 and per_cam_counts(g)[free].max() > 64
    if name in ("odometry_only_camera", "nc40"):
        assert (per_cam_counts(g)[free] == 0).any() and len(g.odom_i)   # a free camera that only odometry edges touch
    if name != "nc2":
        assert has_bbox_and_e3d_pair(g)                         # a camera with a bbox AND a 3-D edge on one ellipsoid: cross terms in M_c
    cx.set_pcg(rel_tol=1e-12)
    cx.upload_graph(g); cx.upload_states(c, o)
    cx.lm_begin(pkg.default_lm_params(jacobian_mode=1, linear_solver=4))
    part = cx.lm_linearize()
    lam = 1e-5 * part.max_diag
    ptr, n, lda = cx.lm_reduced_system(lam)
    S, bs = lower_to_full(cx.lm_download(6, lda * n), n, lda)
    out = cx.lm_try_step(lam)
    assert out.solve_ok == 1 and cx.lm_solver_used() == 4
    xc = cx.lm_download(5, n)
    st = cx.lm_pcg_stats()
    ref = np.linalg.solve(S, bs)
    M = cx.lm_download(10, n * 6).reshape(-1, 6, 6)
    res = cx.lm_reduced_residual()
    x_ref, k_ref, r_ref, ok_ref = pr.pcg_dense(S, bs, rel_tol=1e-12, blocks=M)
    print("PCG %s: n = %d, %d iterations (numpy PCG on the downloaded S, same M: %d), |r|/|b| %.2e, max error vs numpy solve %.2e of max|x| %.2e, "
          "true residual %.2e, M vs diag(S) %.2e of max|S| %.2e" % (name, n, st["iterations"], k_ref, st["rel_residual"], np.abs(xc - ref).max(),
                                                                  np.abs(ref).max(), res, np.abs(M - pr.diag_blocks(S)).max(), np.abs(S).max()))
    np.testing.assert_allclose(xc, ref, rtol=0, atol=1e-9 * np.abs(ref).max() + 1e-12)
    assert res < 1e-11
    np.testing.assert_allclose(M, pr.diag_blocks(S), rtol=0, atol=1e-10 * np.abs(S).max())
    assert st["converged"] == 1 and ok_ref and st["rel_residual"] <= 1e-12
    assert st["iterations"] <= 1.25 * k_ref + 2
    assert (st["max_iters"], st["rel_tol"], st["solves"], st["iterations_total"], st["reserved"]) == (1000, 1e-12, 1, st["iterations"], 0)
    cx.lm_commit(False)


def one_trial(pkg, cx, g, c, o, **pcg):
    cx.set_pcg(**pcg)
    cx.upload_graph(g); cx.upload_states(c, o)
    cx.lm_begin(pkg.default_lm_params(jacobian_mode=1, linear_solver=4))
    part = cx.lm_linearize()
    out = cx.lm_try_step(1e-5 * part.max_diag)
    n = 6 * int((~g.cam_fixed.astype(bool)).sum())
    xc = cx.lm_download(5, n)
    st = cx.lm_pcg_stats()
    cx.lm_commit(False)
    return out, xc, st


def test_pcg_does_not_depend_on_check_every_and_is_reproducible(pkg, cx):
    g, c, o, _ = pkg.synth.make_graph(40, 8, 400, seed=4, slam=True)
    runs = [one_trial(pkg, cx, g, c, o, rel_tol=1e-12, check_every=ce) for ce in (1, 8, 1000, 8)]
    out0, x0, st0 = runs[0]
    assert out0.solve_ok == 1 and st0["converged"] == 1 and st0["iterations"] > 8
    for out, x, st in runs[1:]:
        assert np.array_equal(x, x0)
        assert st["iterations"] == st0["iterations"] and st["rel_residual"] == st0["rel_residual"]
        assert (out.chi2, out.scale, out.solve_ok) == (out0.chi2, out0.scale, out0.solve_ok)


def assert_runs_agree(a, b, what):
    """the tolerances test_slam_lm_matches_faithful_dense_oracle holds solvers 1 and 2 to"""
    (ca, oa, ra), (cb, ob, rb) = a, b
    n = min(len(ra["trace_chi2"]), len(rb["trace_chi2"]))
    print("%s: chi2 trace rel %.2e, cams %.2e, centres %.2e, scales rel %.2e" % (
        what, float(np.abs(np.array(ra["trace_chi2"][:n]) / np.array(rb["trace_chi2"][:n]) - 1).max()), cam_err(ca, cb),
        float(np.abs(oa[:, :3] - ob[:, :3]).max()), float(np.abs(oa[:, 7:] / ob[:, 7:] - 1).max())))
    np.testing.assert_allclose(ra["trace_chi2"][:n], rb["trace_chi2"][:n], rtol=5e-7)
    assert ra["chi2_final"] == pytest.approx(rb["chi2_final"], rel=5e-7)
    assert ra["trace_trials"][:n] == rb["trace_trials"][:n]
    assert cam_err(ca, cb) < 5e-6
    np.testing.assert_allclose(oa[:, :3], ob[:, :3], atol=2e-6)
    np.testing.assert_allclose(oa[:, 7:], ob[:, 7:], rtol=1e-6)


@pytest.fixture(scope="module")
def dense_run(pkg, po):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=True)
    return g, c, o, po.optimize(g, c, o, pkg.default_lm_params(numeric_delta=1e-6), solver=0)


@pytest.mark.parametrize("jac", [0, 1])
def test_pcg_lm_run_matches_faithful_dense_oracle(pkg, cx, dense_run, jac):
    g, c, o, ref = dense_run
    cx.set_pcg(rel_tol=1e-12)
    got = cx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=jac, numeric_delta=1e-6, linear_solver=4))
    assert cx.lm_solver_used() == 4
    assert_runs_agree(got, ref, "PCG LM run (30 cameras) jac %d vs the dense checker" % jac)
    assert np.array_equal(got[0][0], c[0])   # camera 0 is fixed
    st = cx.lm_pcg_stats()
    assert st["solves"] == got[2]["total_trials"] and st["converged"] == 1
    assert st["iterations_total"] >= st["solves"]


def test_pcg_c3_matches_reduced_camera_solver(pkg, cx):
    g, c, o, _ = pkg.synth.make_config("C3", slam=True)
    cx.set_pcg(rel_tol=1e-10)
    c1, o1, r1 = cx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, max_iters=3, linear_solver=1))
    assert cx.lm_solver_used() == 1
    c4, o4, r4 = cx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, max_iters=3, linear_solver=4))
    assert cx.lm_solver_used() == 4
    st = cx.lm_pcg_stats()
    print("C3 SLAM, 3 iterations, PCG vs reduced camera system: chi2 trace rel %.2e, cams %.2e, ellipsoids rel %.2e; %d solves, %.1f iterations per solve"
          % (float(np.abs(np.array(r4["trace_chi2"]) / np.array(r1["trace_chi2"]) - 1).max()), cam_err(c4, c1), obj_rel(o4, o1), st["solves"],
             st["iterations_total"] / st["solves"]))
    assert r4["trace_trials"] == r1["trace_trials"]
    np.testing.assert_allclose(r4["trace_chi2"], r1["trace_chi2"], rtol=1e-6)
    assert cam_err(c4, c1) < 1e-4
    assert obj_rel(o4, o1) < 1e-5
    assert st["converged"] == 1 and st["solves"] == r4["total_trials"]   # (solve by solve: test_pcg_every_c3_solve_converges)
    assert st["iterations_total"] / st["solves"] <= 110


def test_pcg_every_c3_solve_converges(pkg, cx):
    """the same run over the step API: every solve reports converged"""
    g, c, o, _ = pkg.synth.make_config("C3", slam=True)
    cx.set_pcg(rel_tol=1e-10)
    cx.upload_graph(g); cx.upload_states(c, o)
    cx.lm_begin(pkg.default_lm_params(jacobian_mode=1, linear_solver=4))
    lam = None
    for it in range(3):
        part = cx.lm_linearize()
        lam = 1e-5 * part.max_diag if lam is None else lam
        out = cx.lm_try_step(lam)
        st = cx.lm_pcg_stats()
        assert out.solve_ok == 1 and st["converged"] == 1 and st["rel_residual"] <= 1e-10 and st["solves"] == it + 1
        assert st["iterations"] <= 110
        accept = out.chi2 < part.chi2
        cx.lm_commit(accept)
        lam = lam / 3 if accept else lam * 2


def loop_closure_graph(pkg):
    from oracle import np_oracle as npo
    g, c, o, truth = pkg.synth.make_graph(40, 8, 400, seed=4, slam=True)
    Z = npo.T_from7(truth["cams"][39]) @ npo.T_inv(npo.T_from7(truth["cams"][3]))   # Tcw_j Tcw_i^-1 of the true poses
    z7 = np.concatenate([Z[:3, 3], pkg.synth._R_to_quat(Z[None, :3, :3])[0]])
    gl = with_edges(pkg, g, np.ones(len(g.bbox_cam), bool), np.ones(len(g.e3d_cam), bool), odom_i=np.append(g.odom_i, 3), odom_j=np.append(g.odom_j, 39),
                    odom_meas=np.concatenate([g.odom_meas.reshape(-1, 7), z7[None]]), odom_info=None)
    return gl, c, o


def test_pcg_with_a_loop_closure(pkg, cx):
    g, c, o = loop_closure_graph(pkg)
    assert len(g.odom_i) == 40
    with pytest.raises(pkg.EslError, match="status -?\\d+: ESL_SOLVER_REDUCED_ELLIPSOID needs"):
        cx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=2))
    cx.set_pcg(rel_tol=1e-12)
    ref = cx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=1))
    got = cx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=4))
    assert cx.lm_solver_used() == 4 and cx.lm_pcg_stats()["converged"] == 1
    assert_runs_agree(got, ref, "PCG vs reduced camera system with a loop closure 3 -> 39")


@pytest.mark.parametrize("case", ["fixed_ellipsoids", "huber_bbox", "dropped_edges"])
def test_pcg_with_flags_kernels_and_drops(pkg, cx, case):
    fx = None
    if case == "dropped_edges":
        g, c, o = offenders(pkg)
    else:
        g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=True)
        if case == "fixed_ellipsoids":
            fx = np.zeros(g.n_objs, np.uint8); fx[::2] = 1
        else:
            cx.set_robust(bbox=("huber", 1.0))
    cx.set_pcg(rel_tol=1e-12)
    ref = cx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=1), obj_fixed=fx)
    assert cx.lm_solver_used() == 1
    got = cx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=4), obj_fixed=fx)
    assert cx.lm_solver_used() == 4 and cx.lm_pcg_stats()["converged"] == 1
    if case == "dropped_edges":
        assert got[2]["n_bbox_dropped"] > 0 and got[2]["n_bbox_dropped"] == ref[2]["n_bbox_dropped"]
    if case == "fixed_ellipsoids":
        assert np.array_equal(got[1][::2], o[::2])
    assert_runs_agree(got, ref, "PCG vs reduced camera system, " + case)


def test_pcg_after_append_equals_upload(pkg, cx):
    F = 16
    g, c, o, _ = pkg.synth.make_graph(F, 8, 14 * F, seed=9, slam=True)
    p = pkg.default_lm_params(jacobian_mode=1, max_iters=3, linear_solver=4)
    f = F - 1
    cx.upload_graph(slam_graph_upto(pkg, g, f - 1)); cx.upload_states(c[:f], o)
    mb, me, mo = g.bbox_cam == f, g.e3d_cam == f, g.odom_j == f
    assert mb.sum() + me.sum() > 0 and mo.sum() == 1
    cx.append_graph(new_cams=c[f:f + 1], new_cam_fixed=[0], bbox=(g.bbox_cam[mb], g.bbox_obj[mb], g.bbox_meas.reshape(-1, 4)[mb], g.bbox_weight[mb]),
                    e3d=(g.e3d_cam[me], g.e3d_obj[me], g.e3d_meas.reshape(-1, 10)[me], g.e3d_weight[me]),
                    odom=(g.odom_i[mo], g.odom_j[mo], g.odom_meas.reshape(-1, 7)[mo]))
    ra = cx.optimize_resident(p)
    ca, oa = cx.download_states()
    assert cx.lm_solver_used() == 4
    cu, ou, ru = cx.optimize(slam_graph_upto(pkg, g, f), c, o, p)
    assert ra["trace_chi2"] == ru["trace_chi2"] and ra["trace_trials"] == ru["trace_trials"]
    assert np.array_equal(ca, cu) and np.array_equal(oa, ou)


def test_pcg_that_does_not_converge_is_a_rejected_trial(pkg, cx):
    g, c, o, _ = pkg.synth.make_graph(40, 8, 400, seed=4, slam=True)
    out, xc, st = one_trial(pkg, cx, g, c, o, max_iters=3)       # (lm_try_step returned ESL_OK: no exception)
    assert out.solve_ok == 0 and st["converged"] == 0 and st["iterations"] == 3 and st["max_iters"] == 3
    ca, oa = cx.download_states()
    assert np.array_equal(ca, c) and np.array_equal(oa, o)      # after lm_commit(False)
    # a whole run with that cap.  Five trials per iteration: every rejection multiplies lambda (by 2, 4, 8, ...), and from about
    # 1e6 times the largest diagonal entry on S is so nearly block diagonal that three iterations DO reach 1e-10 -- with the default
    # ten trials the LM gets there (lambda_0 x 2^45) and takes that tiny step, which is the recovery g2o's loop is written for.
    # Within five trials (lambda <= lambda_0 x 2^10 = 1e-2 of the largest diagonal entry) no solve converges.
    c3, o3, r3 = cx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=4, max_trials=5))
    assert np.array_equal(c3, c) and np.array_equal(o3, o)
    assert r3["stop_reason"] == 1 and r3["total_trials"] == 5 and r3["iterations"] == 1 and r3["chi2_final"] == r3["chi2_initial"]
    st = cx.lm_pcg_stats()
    assert (st["solves"], st["iterations_total"], st["converged"]) == (5, 15, 0)
    # nothing is left poisoned: the reduced camera system on the same context, against a fresh one
    c1, o1, r1 = cx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=1))
    fresh = pkg.Context(0)
    try:
        c2, o2, r2 = fresh.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=1))
    finally:
        fresh.close()
    assert r1["trace_chi2"] == r2["trace_chi2"] and np.array_equal(c1, c2) and np.array_equal(o1, o2) and r1["chi2_final"] < r1["chi2_initial"]


def test_pcg_refusals(pkg, cx):
    for kw in (dict(max_iters=0), dict(rel_tol=0.0), dict(rel_tol=float("nan")), dict(check_every=0)):
        with pytest.raises(pkg.EslError, match="status -?\\d+: esl_lm_set_pcg"):
            cx.set_pcg(**kw)
    g, c, o, _ = pkg.synth.make_graph(12, 8, 120, seed=4, slam=True)
    with pytest.raises(pkg.EslError, match="linear_solver"):
        cx.optimize(g, c, o, pkg.default_lm_params(linear_solver=7))
    # which = 10 after a trial of another solver
    cx.upload_graph(g); cx.upload_states(c, o)
    cx.lm_begin(pkg.default_lm_params(jacobian_mode=1, linear_solver=1))
    part = cx.lm_linearize()
    cx.lm_try_step(1e-5 * part.max_diag)
    with pytest.raises(pkg.EslError, match="did not run ESL_SOLVER_PCG"):
        cx.lm_download(10, 11 * 36)
    cx.lm_commit(False)
    # a context with a (host-transport) communicator
    cm = pkg.Context(0)
    try:
        cm.comm_init_host(1, 0, lambda buf: None)   # one rank: the sum over the ranks is the buffer itself
        with pytest.raises(pkg.EslError, match="ESL_SOLVER_PCG runs on one GPU"):
            cm.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=4))
    finally:
        cm.close()


def test_pcg_leaves_the_dense_blobs_released(pkg):
    """after esl_ctx_trim a PCG run brings neither the reduced camera system nor the camera-first set back: S stays unavailable to
    esl_lm_download, the camera-first statistics stay empty -- until a dense trial asks for them"""
    g, c, o, _ = pkg.synth.make_graph(40, 8, 400, seed=4, slam=True)
    n = 6 * 39
    cxt = pkg.Context(0)
    try:
        for solver in (1, 2):
            cxt.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, max_iters=1, linear_solver=solver))
        lda = cxt.lm_reduced_system(1.0)[2]
        assert cxt.lm_download(6, lda * n).any()
        cxt.trim()
        cxt.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, max_iters=2, linear_solver=4))
        assert cxt.lm_solver_used() == 4 and cxt.lm_pcg_stats()["converged"] == 1
        with pytest.raises(pkg.EslError, match="not available"):
            cxt.lm_download(6, lda * n)
        assert not any(cxt.lm_solver_stats().values())
        cxt.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, max_iters=1, linear_solver=1))
        assert cxt.lm_download(6, lda * n).any()
    finally:
        cxt.close()
