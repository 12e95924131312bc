"""One SLAM-mode trial step on the device -- Schur build, solve for x_c, back-substitution for x_o, the two retractions, the step's
scalars -- against the extended-precision step of tests/slam_step_ref.py recomputed from the device's OWN linearisation (the blocks of
esl_lm_download), at the boundary sizes of slam_step_ref.CASES (their premises: tests/test_slam_step_ref.py), for every solver and two
dampings (1e-5 max_diag; 1e4 max_diag, under which every camera's rotation update takes se3_exp's small-angle branch).

Tolerances.  The device's error against the longdouble reference (max-norm, relative to the quantity's max-norm) may be at most
MARGIN x yardstick + 4 eps, the yardstick being the error numpy's float64 arithmetic makes on the same quantity of the same case
(slam_step_ref.f64_yardsticks: numpy.linalg.solve of the whole system and numpy Schur + numpy.linalg.cholesky + back-substitution, the
larger of the two; for the retractions: oracle/np_oracle.py's float64 retraction of the same state and update).  The margins are the
next power of two at or above 4 x the worst ratio (device error / yardstick) measured on the MI355X over this whole file:

    Schur build (S, b_s)    worst 2.68  (2 cameras / 2 ellipsoids, S, lambda 1e-5 max_diag)                   -> MARGIN_SCHUR   = 16
    solves (x_c, x_o)       worst 3.50  (5 cameras on a fixed map, camera chain, x_c, lambda 1e-5 max_diag)    -> MARGIN_SOLVE   = 16
    retractions             worst 5.52  (2 cameras / 1 ellipsoid, the free camera, lambda 1e-5 max_diag)      -> MARGIN_RETRACT = 32

Per group of cases (Schur / solves / retractions): A 2.68 / 1.39 / 5.52, B 1.26 / 2.64 / 2.46, C 0.86 / 1.34 / 1.86, D 1.35 / 2.40 / 2.33,
E (both sparse forms) 0.58 / 0.57 / 1.28, robust kernels 0.68 / 1.69 / -, F with odometry 1.00 / 3.50 / 4.80, F without - / 3.21 / 5.29.
PCG at rel_tol 1e-13: |S x_c - b_s| / |b_s| at most 8.8e-14 (bound 2e-13), 2 to 25 iterations.  A ratio above 64 would not be a
margin to adopt but a finding in the kernels; none came near.  The same figures are printed by every run (-s), the worst ones when
the module's context closes.
"""
import numpy as np
import pytest

from tests import slam_step_ref as sr

pytestmark = pytest.mark.gpu

LD = sr.LD
FLOOR = 4 * sr.EPS64
MARGIN_SCHUR = 16.0        # S, b_s
MARGIN_SOLVE = 16.0        # x_c, x_o
MARGIN_RETRACT = 32.0      # trial states
YARDSTICK_MAX = 1e-10      # sanity bound on the float64 yardsticks themselves (largest measured: 5.2e-12, x_c of case E)
PCG_REL_TOL = 1e-13
STATUS_INVALID = 2

WORST = {}                  # kind -> (ratio, where): printed at the end of the module


def allow(margin, yardstick):
    return margin * yardstick + FLOOR


def note(kind, where, err, yardstick):
    ratio = err / yardstick if yardstick > 0 else (0.0 if err <= FLOOR else float("inf"))
    if ratio > WORST.get(kind, (-1.0, ""))[0]:
        WORST[kind] = (ratio, where)
    return ratio


@pytest.fixture(scope="module")
def cx(pkg):
    """a context of this module's own: the PCG and the robust settings belong to the context"""
    c = pkg.Context(0)
    c.set_pcg(rel_tol=PCG_REL_TOL)
    yield c
    c.set_pcg()
    c.set_robust()
    c.close()
    print("\nworst ratios device error / float64 yardstick over the module: " +
          ", ".join("%s %.2f (%s)" % (k, v[0], v[1]) for k, v in sorted(WORST.items())))


class Step:
    """everything one trial step leaves on the device"""


def run_step(pkg, cx, g, c, o, solver, f, flags=None):
    """upload, begin, linearise, reduced system, trial step with lambda = f max_diag, the downloads, commit(False).  Returns a Step, or
    None where the library refuses the solver with ESL_ERR_INVALID (asserted)."""
    nf, N = int((~g.cam_fixed.astype(bool)).sum()), g.n_objs
    cx.upload_graph(g, obj_fixed=flags); cx.upload_states(c, o)
    nv, nd = cx.lm_begin(pkg.default_lm_params(jacobian_mode=1, linear_solver=solver))
    assert nd == 0                                   # no dropped box: every edge of the graph is in the sums
    s = Step()
    s.part = cx.lm_linearize()
    s.lam = f * s.part.max_diag
    s.Hoo, s.bo = cx.lm_download(0, N * 45).reshape(N, 45), cx.lm_download(1, N * 9).reshape(N, 9)
    s.Hcc, s.bc = cx.lm_download(3, nf * 36).reshape(nf, 6, 6), cx.lm_download(4, nf * 6).reshape(nf, 6)
    s.W = None if flags is not None else cx.lm_download(9, (len(g.bbox_cam) + len(g.e3d_cam)) * 54)
    _, n, lda = cx.lm_reduced_system(s.lam)
    assert n == 6 * nf
    s.S, s.bs = sr.lower_to_full(cx.lm_download(6, lda * n), n, lda)
    try:
        s.out = cx.lm_try_step(s.lam)
    except pkg.EslError as e:
        assert solver == 2 and "esl_status %d" % STATUS_INVALID in str(e), str(e)
        return None
    assert cx.lm_solver_used() == solver
    s.xc, s.xo = cx.lm_download(5, n), cx.lm_download(2, N * 9).reshape(N, 9)
    s.objs, s.cams = cx.lm_download(7, N * 10).reshape(N, 10), cx.lm_download(8, g.n_cams * 7).reshape(g.n_cams, 7)
    s.pcg = cx.lm_pcg_stats() if solver == 4 else None
    s.stats = cx.lm_solver_stats() if solver == 2 else None
    cx.lm_commit(False)
    return s


def same_linearisation(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("Hoo", "bo", "Hcc", "bc")) and \
        ((a.W is None and b.W is None) or np.array_equal(a.W, b.W)) and a.lam == b.lam


def reference(g, s):
    """the longdouble step and the float64 yardsticks on the blocks of one Step (the odometry blocks from its S)"""
    B = sr.Blocks(g, s.Hoo, s.bo, s.Hcc, s.bc, s.W)
    ref = sr.reference_step(B, s.lam, S_dev=s.S)
    ref["B"] = B
    ref["y"] = sr.f64_yardsticks(B, s.lam, ref["hodo"], ref)
    # numpy's float64 elimination of these systems (conditioning up to ~1e5) is never further than this from the truth: a yardstick
    # beyond it means the reference, not float64, is off, and would only widen what the device is allowed
    assert all(ref["y"][k] <= YARDSTICK_MAX for k in ("S", "bs", "xc", "xo")), ref["y"]
    return ref


def block_mask(mask):
    return np.kron(mask, np.ones((6, 6), dtype=bool))


def check_schur(where, s, ref):
    """(a) diagonal and non-neighbour blocks of S, all of b_s"""
    keep = ~block_mask(ref["mask"])
    e_S = sr.rel_err(np.where(keep, s.S, 0), np.where(keep, ref["S"], 0))
    e_b = sr.rel_err(s.bs, ref["bs"])
    r_S, r_b = note("schur", where + " S", e_S, ref["y"]["S"]), note("schur", where + " b_s", e_b, ref["y"]["bs"])
    print("%s: S error %.2e (yardstick %.2e, ratio %.2f), b_s error %.2e (yardstick %.2e, ratio %.2f)" % (where, e_S, ref["y"]["S"], r_S, e_b, ref["y"]["bs"], r_b))
    assert e_S <= allow(MARGIN_SCHUR, ref["y"]["S"]), (where, e_S, ref["y"]["S"])
    assert e_b <= allow(MARGIN_SCHUR, ref["y"]["bs"]), (where, e_b, ref["y"]["bs"])


def check_solve(where, solver, s, ref):
    """(c) x_c, (d) x_o from the device's own x_c and from the reference's; returns the allowances (x_c, x_o) of this solver"""
    B, y = ref["B"], ref["y"]
    a_c, a_o = allow(MARGIN_SOLVE, y["xc"]), allow(MARGIN_SOLVE, y["xo"])
    assert ref["xc_last"] <= 1e-3 * max(y["xc"], sr.EPS64) * float(np.abs(ref["xc"]).max())      # the reference has converged
    e_c = sr.rel_err(s.xc, ref["xc"])
    xo_own = sr.backsub_ref(B, ref["Dinv"], s.xc)
    e_own, e_o = sr.rel_err(s.xo, xo_own), sr.rel_err(s.xo, ref["xo"])
    if solver == 4:
        r = sr.residual_ld(ref["Sc"], np.asarray(s.xc, dtype=LD), ref["bs"])
        res = float(np.sqrt(r @ r) / np.sqrt(ref["bs"] @ ref["bs"]))
        print("%s: PCG |S x_c - b_s| / |b_s| %.2e after %d iterations (x_c error %.2e, yardstick %.2e); x_o from its own x_c %.2e (yardstick %.2e, ratio %.2f)"
              % (where, res, s.pcg["iterations"], e_c, y["xc"], e_own, y["xo"], note("solve", where + " x_o(own x_c)", e_own, y["xo"])))
        assert s.pcg["converged"] == 1 and s.pcg["rel_tol"] == PCG_REL_TOL
        assert res <= 2 * PCG_REL_TOL, (where, res)
    else:
        r_c, r_o, r_own = note("solve", where + " x_c", e_c, y["xc"]), note("solve", where + " x_o", e_o, y["xo"]), note("solve", where + " x_o(own x_c)", e_own, y["xo"])
        print("%s: x_c error %.2e (yardstick %.2e, ratio %.2f), x_o error %.2e (yardstick %.2e, ratio %.2f), x_o from its own x_c %.2e (ratio %.2f)"
              % (where, e_c, y["xc"], r_c, e_o, y["xo"], r_o, e_own, r_own))
        assert e_c <= a_c, (where, e_c, y["xc"])
        assert e_o <= a_o, (where, e_o, y["xo"])
    assert e_own <= a_o, (where, e_own, y["xo"])
    return a_c, a_o


def check_retractions(where, g, c, o, s, flags=None):
    """(e) the trial states against the longdouble retractions of the uploaded states by the DOWNLOADED x, per vertex"""
    slot = sr.cam_slots(g)
    errs, yards = [], []
    for ci in range(g.n_cams):
        if slot[ci] < 0:
            assert np.array_equal(s.cams[ci], np.asarray(c, dtype=np.float64).reshape(-1, 7)[ci])       # the fixed camera: bit for bit
            continue
        u = s.xc[6 * slot[ci]:6 * slot[ci] + 6]
        want = sr.cam_oplus_ld(c[ci], u)
        scale = max(1.0, float(np.abs(want).max()))
        errs.append(sr.state_err(s.cams[ci], want) / scale)
        yards.append(sr.state_err(sr.cam_oplus_f64(c[ci], u), want) / scale)
        assert abs(float(np.asarray(s.cams[ci, 3:7], dtype=LD) @ np.asarray(s.cams[ci, 3:7], dtype=LD)) - 1) <= 1e-15
    y_c = max(yards) if yards else 0.0
    e_c = max(errs) if errs else 0.0
    errs_o, yards_o = [], []
    for oi in range(g.n_objs):
        if flags is not None and flags[oi]:
            assert np.array_equal(s.objs[oi], np.asarray(o, dtype=np.float64).reshape(-1, 10)[oi])
            continue
        want = sr.obj_oplus_ld(o[oi], s.xo[oi])
        scale = max(1.0, float(np.abs(want).max()))
        errs_o.append(sr.state_err(s.objs[oi], want) / scale)
        yards_o.append(sr.state_err(sr.obj_oplus_f64(o[oi], s.xo[oi]), want) / scale)
        assert abs(float(np.asarray(s.objs[oi, 3:7], dtype=LD) @ np.asarray(s.objs[oi, 3:7], dtype=LD)) - 1) <= 1e-15
    y_o = max(yards_o) if yards_o else 0.0
    e_o = max(errs_o) if errs_o else 0.0
    print("%s: trial cameras %.2e (yardstick %.2e, ratio %.2f), trial ellipsoids %.2e (yardstick %.2e, ratio %.2f)"
          % (where, e_c, y_c, note("retract", where + " cameras", e_c, y_c), e_o, y_o, note("retract", where + " ellipsoids", e_o, y_o)))
    assert all(e <= allow(MARGIN_RETRACT, y_c) for e in errs), (where, e_c, y_c)
    assert all(e <= allow(MARGIN_RETRACT, y_o) for e in errs_o), (where, e_o, y_o)


def check_partials(where, s, ref, chi2_checker):
    """(f) scale = sum_j x_j (lambda x_j + b_j) from the downloads in longdouble, to 1e-12 (at most ~1,900 products: n eps with a factor
    4 of room); solve_ok; chi2 of the trial states against the checker's, to the 1e-9 of the linearisation tests"""
    want = float(sr.step_scale(ref["B"], s.lam, s.xc, s.xo))
    assert s.out.solve_ok == 1
    assert abs(s.out.scale - want) <= 1e-12 * abs(want), (where, s.out.scale, want)
    assert s.out.chi2 == pytest.approx(chi2_checker, rel=1e-9), where


def small_angle_premise(where, f, ref):
    """the large damping puts every camera on se3_exp's small-angle branch, the small one none -- from the reference's x_c"""
    om = np.sqrt((np.asarray(ref["xc"]).reshape(-1, 6)[:, :3] ** 2).sum(axis=1))
    if f == sr.LAM_BIG:
        assert float(om.max()) < sr.SMALL_ANGLE, (where, float(om.max()))
    else:
        assert float(om.min()) > sr.SMALL_ANGLE, (where, float(om.min()))


def run_case(pkg, po, cx, name, g, c, o, solvers, x_form=None):
    """checks a to g of one graph: every solver under both dampings"""
    n = 6 * int((~g.cam_fixed.astype(bool)).sum())
    Hchk = po.build_system(g, c, o, delta=1e-6)[0][:n, :n]
    hodo_by_f = {}
    for f in (sr.LAM_SMALL, sr.LAM_BIG):
        ref, first, got = None, None, {}
        for solver in solvers:
            where = "%s solver %d lambda %.0e" % (name, solver, f)
            s = run_step(pkg, cx, g, c, o, solver, f)
            if s is None:
                print(where + ": refused with ESL_ERR_INVALID")
                continue
            if ref is None or not same_linearisation(s, first) or not np.array_equal(s.S, first.S):
                ref, first = reference(g, s), s              # (the solvers share one linearisation and one S: computed once)
                small_angle_premise(where, f, ref)
            check_schur(where, s, ref)
            a = check_solve(where, solver, s, ref)
            check_retractions(where, g, c, o, s)
            check_partials(where, s, ref, po.build_system(g, s.cams, s.objs, delta=1e-6)[3])
            if solver == 2 and x_form is not None:
                assert s.stats["x_form"] == x_form and s.stats["stride"] == 16, s.stats          # the sparse form ran
            got[solver] = (s, a, ref)
        # (b) the odometry-neighbour blocks with the reference's Schur term added back: H_cc's own blocks, free of lambda
        s1, _, ref1 = got[solvers[0]]
        hodo_by_f[f] = (ref1["hodo"], allow(MARGIN_SCHUR, ref1["y"]["S"]) * float(np.abs(ref1["Sc"]).max()))
        for (i, j), blk in ref1["hodo"].items():
            want = Hchk[6 * i:6 * i + 6, 6 * j:6 * j + 6]
            np.testing.assert_allclose(np.asarray(blk, dtype=np.float64), want, rtol=0, atol=5e-6 * np.abs(Hchk).max(), err_msg="%s block (%d, %d)" % (name, i, j))
        # (g) the direct solvers agree within the sum of their allowances
        if 1 in got and 2 in got:
            (sa, aa, ra), (sb, ab, rb) = got[1], got[2]
            assert np.abs(sa.xc - sb.xc).max() <= (aa[0] + ab[0]) * float(np.abs(ra["xc"]).max())
            assert np.abs(sa.xo - sb.xo).max() <= (aa[1] + ab[1]) * float(np.abs(ra["xo"]).max())
    (h0, t0), (h1, t1) = hodo_by_f[sr.LAM_SMALL], hodo_by_f[sr.LAM_BIG]
    for p in h0:
        d = float(np.abs(h0[p] - h1[p]).max())
        assert d <= t0 + t1, (name, p, d, t0, t1)            # one matrix at both dampings: the odometry block does not depend on lambda


@pytest.mark.parametrize("name", [k for k in sr.CASES if not k.startswith("E_")])
def test_trial_step_matches_extended_precision(pkg, po, cx, name):
    g, c, o = sr.build_case(pkg, name)
    run_case(pkg, po, cx, name, g, c, o, (1, 2, 4))


@pytest.mark.parametrize("form", [1, 2])
def test_trial_step_with_sparse_camera_first_rows(pkg, po, monkeypatch, form):
    """case E: the (257, 40, 6) graph of test_sparse_interior_rows_equal_dense_rows with X = G^-1 W kept sparse (ESL_CF_SPARSE: 1 stored
    per-segment products, 2 blocks straight from the slabs; read when the context is created), so that solver 2 runs its sparse form"""
    g, c, o = sr.build_case(pkg, "E_257c_40e")
    monkeypatch.setenv("ESL_CF_SPARSE", str(form))
    cs = pkg.Context(0)
    try:
        cs.set_pcg(rel_tol=PCG_REL_TOL)
        run_case(pkg, po, cs, "E_257c_40e form %d" % form, g, c, o, (1, 2, 4) if form == 1 else (1, 2), x_form=form)
    finally:
        cs.close()
        monkeypatch.delenv("ESL_CF_SPARSE", raising=False)


@pytest.mark.parametrize("solver", [1, 3])
def test_fixed_ellipsoid_step_reads_zero_after_another_graph(pkg, cx, solver):
    """The smallest shape at which x_o of a fixed ellipsoid did not read as zero (include/esl.h, esl_graph_upload_fixed): 2 cameras
    against a fixed map, on a context whose work area an earlier, larger graph has been through (here case B's 22 cameras and 15
    ellipsoids) -- k_slam_backsub left x_o of an ellipsoid without an active edge unwritten, and esl_lm_download(2) returned whatever the
    earlier graph had left at that place."""
    g, c, o = sr.build_case(pkg, "B_22c_15e")
    before = run_step(pkg, cx, g, c, o, 1, sr.LAM_SMALL)
    assert before.xo.any()
    g, c, o = sr.build_f_case(pkg, 2, True)
    s = run_step(pkg, cx, g, c, o, solver, sr.LAM_SMALL, flags=np.ones(g.n_objs, np.uint8))
    assert not s.xo.any()
    assert np.array_equal(s.objs, o)


@pytest.mark.parametrize("solver", [1, 2])
def test_trial_step_with_robust_kernels(pkg, po, cx, solver):
    """case B (22 cameras, 15 ellipsoids) with the first kind set of test_robust_linearisation_matches_reweighted_oracle: the weights
    enter H_oo, W and H_cc on the device, and checks a, c, d hold on the weighted blocks"""
    from tests.test_gpu_robust import KIND_SETS, widths
    g, c, o = sr.build_case(pkg, "B_22c_15e")
    dl = widths(g, c, o, ["bbox", "e3d", "odom"])
    robust = {cls: (k, dl[cls]) for cls, k in zip(("bbox", "e3d", "odom"), KIND_SETS[0])}
    plain = run_step(pkg, cx, g, c, o, solver, sr.LAM_SMALL)
    cx.set_robust(**robust)
    try:
        for f in (sr.LAM_SMALL, sr.LAM_BIG):
            where = "B_22c_15e robust solver %d lambda %.0e" % (solver, f)
            s = run_step(pkg, cx, g, c, o, solver, f)
            assert s is not None
            if f == sr.LAM_SMALL:
                assert not np.array_equal(s.Hoo, plain.Hoo) and not np.array_equal(s.Hcc, plain.Hcc) and not np.array_equal(s.W, plain.W)   # the weights are in
            ref = reference(g, s)
            check_schur(where, s, ref)
            check_solve(where, solver, s, ref)
    finally:
        cx.set_robust()


@pytest.mark.parametrize("odometry", [True, False])
@pytest.mark.parametrize("n_cams", sr.F_CAMS)
def test_fixed_map_trial_step(pkg, po, cx, n_cams, odometry):
    """case F: every ellipsoid flagged fixed -- ESL_SOLVER_CAMERA_CHAIN (cyclic reduction over nf = n_cams - 1 free cameras) and the
    reduced camera system against the reference; x_o exactly zero, the ellipsoids untouched"""
    from tests import fixed_ref as fr
    g, c, o = sr.build_f_case(pkg, n_cams, odometry)
    ones = np.ones(g.n_objs, np.uint8)
    nf = n_cams - 1
    Hchk = po.build_system(g, c, o, delta=1e-6)[0][:6 * nf, :6 * nf]
    hodo_by_f = {}
    for f in (sr.LAM_SMALL, sr.LAM_BIG):
        got = {}
        for solver in (3, 1):
            where = "F %d cameras%s solver %d lambda %.0e" % (n_cams, "" if odometry else " (no odometry)", solver, f)
            s = run_step(pkg, cx, g, c, o, solver, f, flags=ones)
            assert not s.Hoo.any(), where + ": H_oo of a fixed ellipsoid"
            assert not s.bo.any(), where + ": b_o of a fixed ellipsoid"
            assert not s.xo.any(), where + ": x_o of a fixed ellipsoid"
            ref = reference(g, s)
            small_angle_premise(where, f, ref)
            if odometry:
                check_schur(where, s, ref)
            else:                                              # no Schur term, no odometry: S is H_cc + lambda I, to one rounding
                assert not s.S[~block_mask(np.eye(nf, dtype=bool))].any()
                for k in range(nf):
                    want = ref["S"][6 * k:6 * k + 6, 6 * k:6 * k + 6]
                    assert (np.abs(np.asarray(s.S[6 * k:6 * k + 6, 6 * k:6 * k + 6], dtype=LD) - want) <= sr.EPS64 * np.abs(want)).all()
                assert np.array_equal(s.bs, s.bc.reshape(-1))
            a = check_solve(where, solver, s, ref)
            check_retractions(where, g, c, o, s, flags=ones)
            G = fr.FixedNpGraph(g, s.cams, o, ones); G.drop_nan(); G.finalize()
            check_partials(where, s, ref, G.chi2())
            got[solver] = (s, a, ref)
        (s3, a3, r3), (s1, a1, _) = got[3], got[1]
        assert np.abs(s3.xc - s1.xc).max() <= (a3[0] + a1[0]) * float(np.abs(r3["xc"]).max())
        hodo_by_f[f] = r3["hodo"]
        for (i, j), blk in r3["hodo"].items():
            want = Hchk[6 * i:6 * i + 6, 6 * j:6 * j + 6]
            np.testing.assert_allclose(np.asarray(blk, dtype=np.float64), want, rtol=0, atol=5e-6 * np.abs(Hchk).max())
    for p in hodo_by_f[sr.LAM_SMALL]:                          # no Schur term here: the device's odometry blocks themselves, lambda-free
        assert np.array_equal(hodo_by_f[sr.LAM_SMALL][p], hodo_by_f[sr.LAM_BIG][p])
