"""CPU tests of tests/map_step_ref.py (the extended-precision mapping-mode trial step and the restated Levenberg control that
tests/test_gpu_map_step.py holds both forms of the device's step to) and of the premises of every graph that file runs, from the checker's
system (oracle/pyoracle.py's build_system cut into per-ellipsoid blocks; the robust case: tests/robust_ref.py's reweighted system): the
shapes the table claims, the quality of the reference, the cap on the float64 yardsticks, the distance of every decision of the lock-step
runs from its threshold, and lm_control against the checker's own LM.

lm_control against the checker.  The checker reports a trace per iteration, not the scalars of a trial, and keeps its states in its own
structs.  A run replayed through its pieces (build_system, ldlt_solve, obj_oplus) hands the states on as 10-vectors, whose quaternion is a
rounding away from the checker's own: the chi2 of the first trial states already differs by 1e-14, and from the second iteration on the
checker's numeric differentiation (delta 1e-6) turns the last bits of the states into 1e-10 .. 2e-4 of chi2 and lambda over a run with
rejected trials.  Bit-equality with the checker's trace is therefore not to be had beyond the start.  Asserted instead: chi2 of the start
to 1e-14 (it is added up in groups of ellipsoids here) and lambda_0 = tau max_diag bit for bit; a single trial (max_iters = max_trials = 1)
and the first iteration of every whole run to 1e-12; over whole runs the trials per iteration, the iterations and the stop reason exactly
and chi2 and lambda to 1e-3; the stop rules and the lambda update on made-up scalars, exactly."""
import numpy as np
import pytest

from tests import map_step_ref as mr
from tests import slam_step_ref as sr

LD = sr.LD
YARDSTICK_CAP = 1e-9
DIAG = [0, 9, 17, 24, 30, 35, 39, 42, 44]          # the diagonal in the packed upper triangle
LOCK = [k for k, v in mr.CASES.items() if v.get("lock")]
SMALL = [k for k in mr.CASES if k != "large" and not mr.CASES[k].get("robust")]          # (the C checker has no robust kernels)
_blocks = {}


def robust_of(name, g, c, o):
    cls = mr.CASES[name].get("robust")
    return mr.robust_widths(g, c, o, cls) if cls else None


def checker_system(pkg, po, name):
    """(seen graph, cameras, ellipsoids, active mask, Hoo45, bo, chi2, max_diag) of a case from the checker, once per process"""
    if name not in _blocks:
        g, c, o, flags = mr.build_case(pkg, name)
        gs = mr.seen_graph(g, flags)
        robust = robust_of(name, g, c, o)
        if robust:
            from tests import robust_ref as rr
            G = rr.RobustNpGraph(gs, c, o, robust); G.drop_nan(); G.finalize()
            H, b = G.build(1e-6)
            iu = np.triu_indices(9)
            Hoo, bo = np.zeros((g.n_objs, 45)), np.zeros((g.n_objs, 9))
            for ob, i in G.idx_o.items():
                Hoo[ob], bo[ob] = H[i:i + 9, i:i + 9][iu], b[i:i + 9]
            chi = G.chi2()
        else:
            Hoo, bo, chi = mr.checker_blocks(po, gs, c, o)
        _blocks[name] = (gs, c, o, mr.active_mask(g, flags), Hoo, bo, chi, float(np.abs(Hoo[:, DIAG]).max()))
    return _blocks[name]


@pytest.mark.parametrize("name", list(mr.CASES))
def test_case_premises(pkg, po, name):
    """every graph of tests/test_gpu_map_step.py is the case its row of map_step_ref.CASES says it is"""
    case = mr.CASES[name]
    g, c, o, flags = mr.build_case(pkg, name)
    gs = mr.seen_graph(g, flags)
    assert g.cam_fixed is None and len(g.odom_i) == 0                       # mapping mode
    assert g.n_objs == case["N"] == len(o)
    ch = mr.chunks_per_obj(gs)
    assert int(ch.max()) == case["chunks"], ch
    act = mr.active_mask(g, flags)
    assert tuple(np.nonzero(~act)[0]) == tuple(case.get("inactive", ()))
    _, _, rep = po.optimize(gs, c, o, pkg.default_lm_params(max_iters=1, max_trials=1, numeric_delta=1e-6), solver=po.ORACLE_BLOCK)
    assert rep["n_bbox_dropped"] == 0                                       # every edge is in the sums
    if name == "large":
        nb, ne = mr.edges_per_obj(g)
        assert mr.step_blocks(g.n_objs) == case["step_blocks"] > mr.DECIDE_STRIDE
        assert mr.lin_blocks(g) == case["lin_blocks"] > mr.DECIDE_STRIDE
        assert g.n_objs > mr.STEP_WAVES * mr.DECIDE_STRIDE
        assert (nb + ne).min() >= 2 and (nb + ne).max() <= 4
    if name == "rows":
        assert tuple(ch) == mr.ROWS_CHUNKS and mr.edges_per_obj(g)[0].tolist() == [e[0] for e in mr.ROWS_EDGES]
        assert set(ch) >= {1, 4, 5, 7} and int(np.argmax(ch)) % mr.STEP_WAVES != 0        # the longest: not wave 0 of its workgroup
        k = int(np.argmax(ch))
        assert ch[k - 1] == 1 and ch[k + 1] == 1 and (k - 1) // mr.STEP_WAVES == (k + 1) // mr.STEP_WAVES        # one-row neighbours beside it
    if name == "long_ellipsoid":
        assert ch.tolist() == [5, 1]
    if name == "deficient":
        nb, ne = mr.edges_per_obj(gs)
        ng = np.bincount(gs.grav_obj, minlength=g.n_objs)
        assert (nb[1], ne[1], ng[1]) == (1, 0, 0) and (nb[2], ne[2], ng[2]) == (0, 0, 1) and (nb[3], ne[3], ng[3]) == (0, 0, 0)
        assert flags[5] == 1 and flags.sum() == 1 and mr.edges_per_obj(g)[0][5] > 0 and (nb[5], ne[5], ng[5]) == (0, 0, 0)
    if case.get("robust"):
        from tests import robust_ref as rr
        robust = robust_of(name, g, c, o)
        for cls in case["robust"]:
            w = rr.edge_chi2(g, c, o, cls, robust)[1]
            assert (w < 0.95).any() and (w == 1.0).any(), (cls, w)        # both branches of the kernel: an edge beyond delta, one within


def test_case_table_names_every_boundary():
    n = {k: v["N"] for k, v in mr.CASES.items()}
    assert [n[k] for k in ("N1", "N3", "N4", "N5")] == [1, mr.STEP_WAVES - 1, mr.STEP_WAVES, mr.STEP_WAVES + 1]
    assert [n[k] for k in ("N63", "N64", "N65")] == [mr.SOLVE_LANES - 1, mr.SOLVE_LANES, mr.SOLVE_LANES + 1]
    assert n["large"] > mr.STEP_WAVES * mr.DECIDE_STRIDE
    assert sorted(set(mr.ROWS_CHUNKS)) == [1, 4, 5, 6, 7] and mr.CASES["long_ellipsoid"]["chunks"] == 5
    assert any(v.get("robust") for v in mr.CASES.values()) and any(v.get("jac") == 0 for v in mr.CASES.values())
    assert len(LOCK) >= 3


@pytest.mark.parametrize("name", list(mr.CASES))
def test_reference_quality_and_yardstick_cap(pkg, po, name):
    """On the checker's blocks, under both dampings: the reference solves its own systems to 4 eps of ITS format in error-free residuals
    (normwise backward error) and has converged; every float64 yardstick is at most 1e-9 (the gravity-only blocks under the small damping
    are the worst conditioned)."""
    gs, c, o, act, Hoo, bo, chi, md = checker_system(pkg, po, name)
    for f in (mr.LAM_SMALL, mr.LAM_BIG):
        ref = mr.reference_step(Hoo, bo, f * md, act)
        y = mr.f64_yardsticks(ref)
        xmax = np.abs(ref["x"]).max(axis=1).astype(np.float64)
        print("%s lambda %.0e max_diag: backward error %.1e, last correction / |x| %.1e, yardsticks %s"
              % (name, f, ref["backward"].max(), (ref["last"][act] / xmax[act]).max(), {k: "%.1e" % v for k, v in y.items()}))
        assert ref["backward"].max() <= 4 * float(np.finfo(LD).eps)
        assert (ref["last"][act] <= 1e-3 * sr.EPS64 * xmax[act]).all()
        assert not ref["x"][~act].any()
        assert max(y[k] for k in ("x", "scale")) <= YARDSTICK_CAP, y
        e, yr = mr.retract_errors(np.asarray(mr.retract_ld(o, ref["x"], act), dtype=np.float64), o, ref["x"], act)
        assert e <= 2 * sr.EPS64 and yr <= 1e-14                          # (the rounding of the reference's own states; np_oracle's distance)


def test_reference_against_mpmath_on_the_worst_block(pkg, po):
    """the one-edge and the gravity-only block of the rank-deficient case under the small damping (the worst conditioned of the table): the
    longdouble path against mpmath's LU at 40 digits.  The bound is a quarter of float64's eps, not longdouble's: H + lambda I is formed in
    longdouble, and the rounding of its diagonal (5e-20) is carried to x by the block's condition (measured: 1.3e-17)."""
    mp = pytest.importorskip("mpmath")
    gs, c, o, act, Hoo, bo, chi, md = checker_system(pkg, po, "deficient")
    lam = mr.LAM_SMALL * md
    ref = mr.reference_step(Hoo, bo, lam, act)
    mp.mp.dps = 40
    for ob in (1, 2):
        A = mp.matrix(sr.unpack45(Hoo[ob]).tolist()) + mp.mpf(lam) * mp.eye(9)
        x = mp.lu_solve(A, mp.matrix(bo[ob].tolist()))
        hi = ref["x"][ob].astype(np.float64)
        lo = (ref["x"][ob] - hi).astype(np.float64)
        err = max(abs(mp.mpf(float(hi[i])) + mp.mpf(float(lo[i])) - x[i]) for i in range(9)) / max(abs(v) for v in x)
        assert err <= sr.EPS64 / 4, (ob, float(err))


def test_chi2_from_definitions_matches_the_checker(pkg, po):
    """map_step_ref.chi2_at (lin_ref's edge classes, values only) against the checker's chi2 on a plain, the rank-deficient and the
    robust case (there: tests/robust_ref.py's)"""
    for name in ("N5", "deficient", "robust", "long_ellipsoid"):
        gs, c, o, act, Hoo, bo, chi, md = checker_system(pkg, po, name)
        g, _, _, flags = mr.build_case(pkg, name)
        want, y, _ = mr.chi2_ref(g, c, o, robust_of(name, g, c, o), flags)
        assert float(want) == pytest.approx(chi, rel=1e-12), name
        assert y <= 1e-13, (name, y)


def one_trial(pkg, po, name):
    """the reference's single trial at lambda_0 = tau max_diag on the checker's blocks: (rho, chi2 of the reference's trial states)"""
    gs, c, o, act, Hoo, bo, chi, md = checker_system(pkg, po, name)
    g, _, _, flags = mr.build_case(pkg, name)
    ref = mr.reference_step(Hoo, bo, mr.TAU * md, act)
    trial = np.asarray(mr.retract_ld(o, ref["x"], act), dtype=np.float64)
    robust = robust_of(name, g, c, o)
    chi_t = float(mr.chi2_at(mr.lr.F64, g, c, trial, robust, flags)) if robust else mr.checker_chi2(po, gs, c, trial)
    st = mr.LmState(chi, md, max_iters=1, max_trials=1)
    mr.lm_control(chi, chi_t, ref["scale"], True, st)
    return float(st.rho), st


def test_one_trial_cases_near_rho_zero_are_at_most_one(pkg, po):
    """test (b) leaves the states of a case whose rho at lambda_0 is within 1e-3 of 0 out of its comparison: at most one case may be such,
    judged by the reference alone; and the large case's trial is accepted with rho inside the window where lambda follows it"""
    rhos = {name: one_trial(pkg, po, name)[0] for name in mr.CASES}
    print("rho of the single trial at lambda_0: " + ", ".join("%s %.3g" % kv for kv in rhos.items()))
    assert sum(abs(r) < 1e-3 for r in rhos.values()) <= 1, rhos
    # the case that crosses lm_decide's stride is accepted, with lambda's factor off both clamps: chi2_final and lambda_final of test (b)
    # then depend on every partial of the two strided sums (a refused trial would leave only the sign of rho to them)
    lo, hi = mr.RHO_UNCLAMPED
    assert lo < rhos["large"] < hi, rhos["large"]
    for r in (lo, hi):
        assert 1 / 3 < 1 - (2 * r - 1) ** 3 < 2 / 3


@pytest.mark.parametrize("name", SMALL)
def test_lm_control_reproduces_a_single_checker_trial(pkg, po, name):
    gs, c, o, act, Hoo, bo, chi, md = checker_system(pkg, po, name)
    p = pkg.default_lm_params(max_iters=1, max_trials=1, numeric_delta=1e-6)
    _, oo, rep = po.optimize(gs, c, o, p, solver=po.ORACLE_BLOCK)
    st = mr.LmState(chi, md, max_iters=1, max_trials=1, T=np.float64)
    o2, trials = mr.checker_run(po, gs, c, o, st)
    assert len(trials) == 1 and st.done
    assert (st.it, st.total_trials, st.stop) == (rep["iterations"], rep["total_trials"], rep["stop_reason"]) == (1, 1, mr.STOP_TRIALS)
    assert chi == pytest.approx(rep["chi2_initial"], rel=1e-14) and trials[0]["lam"] == p.tau * md          # (chi2 is added up in groups of ellipsoids here)
    assert float(st.chi) == pytest.approx(rep["chi2_final"], rel=1e-12) and float(st.lam) == pytest.approx(rep["lambda_final"], rel=1e-12)
    np.testing.assert_allclose(o2, oo, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", LOCK)
def test_lock_step_cases_are_away_from_thresholds(pkg, po, name):
    """The checker's LM with the parameters of the lock-step test, replayed trial by trial: no decision sits at a threshold, the run has a
    rejected trial and three iterations or more, and lm_control -- in float64 and in longdouble -- takes the checker's decisions."""
    gs, c, o, act, Hoo, bo, chi, md = checker_system(pkg, po, name)
    p = mr.lm_params(pkg, name)
    p.numeric_delta = 1e-6
    _, oo, rep = po.optimize(gs, c, o, p, solver=po.ORACLE_BLOCK)
    st = mr.LmState(chi, md, p.tau, p.max_iters, p.max_trials, T=np.float64)
    ld = mr.LmState(chi, md, p.tau, p.max_iters, p.max_trials, T=LD)
    same = []

    def shadow(t):          # the longdouble control on the same scalars
        same.append(mr.lm_control(t["chi_cur"], t["chi_trial"], t["scale"], t["ok"], ld) == t["accept"])
    o2, trials = mr.checker_run(po, gs, c, o, st, hook=shadow)
    print("%s: %d iterations, trials %s, stop %d, |rho| from %.3g" % (name, st.it, [t[2] for t in st.trace], st.stop, min(abs(t["rho"]) for t in trials)))
    assert all(abs(t["rho"]) >= 1e-3 for t in trials) and all(t["rho"] != 0 for t in trials) and all(t["ok"] for t in trials)
    assert any(not t["accept"] for t in trials) and st.it >= 3
    first = chi
    for chi_k, _, _ in st.trace:
        assert abs((first - float(chi_k)) * mr.GAIN_FACTOR - first) >= 1e-6 * first, (first, chi_k)
        first = float(chi_k)
    assert max(n for _, _, n in st.trace) < p.max_trials
    # lm_control against the checker's own run
    assert [n for _, _, n in st.trace] == rep["trace_trials"]
    assert (st.it, st.total_trials, st.stop) == (rep["iterations"], rep["total_trials"], rep["stop_reason"])
    assert chi == pytest.approx(rep["chi2_initial"], rel=1e-14)
    assert float(st.trace[0][0]) == pytest.approx(rep["trace_chi2"][0], rel=1e-12) and float(st.trace[0][1]) == pytest.approx(rep["trace_lambda"][0], rel=1e-12)
    np.testing.assert_allclose([float(t[0]) for t in st.trace], rep["trace_chi2"], rtol=1e-3)
    np.testing.assert_allclose([float(t[1]) for t in st.trace], rep["trace_lambda"], rtol=1e-3)
    np.testing.assert_allclose(o2, oo, atol=5e-3)
    # ... and the longdouble control beside the float64 one
    assert all(same) and (ld.it, ld.total_trials, ld.stop) == (st.it, st.total_trials, st.stop)
    assert [n for _, _, n in ld.trace] == [n for _, _, n in st.trace]
    for (_, a, _), (_, b, _) in zip(ld.trace, st.trace):
        assert abs(float(a) - float(b)) <= 32 * sr.EPS64 * float(a)          # (one rounding per trial, at most max_iters x max_trials of them)


def test_lm_control_stop_rules():
    """the rules on made-up scalars: trials run out; rho exactly 0; three iterations without gain; max_iters; an unsolvable step"""
    for T in (np.float64, LD):
        s = mr.LmState(100.0, 1e5, max_trials=3, T=T)
        lam0 = s.lam
        assert [mr.lm_control(100.0, 150.0, 10.0, True, s) for _ in range(3)] == [False] * 3
        assert s.done and (s.stop, s.it, s.total_trials) == (mr.STOP_TRIALS, 1, 3) and s.lam == lam0 * 2 * 4 * 8 and s.chi == 100
        s = mr.LmState(100.0, 1e5, T=T)
        assert not mr.lm_control(100.0, 100.0, 10.0, True, s) and s.done and s.stop == mr.STOP_TRIALS and s.lam == 2 * T(1e-5) * T(1e5)
        s = mr.LmState(100.0, 1e5, T=T)
        chi = 100.0
        for k in range(3):
            assert not s.done
            assert mr.lm_control(chi, chi * (1 - 5e-4), 1.0, True, s)          # gains 0.05 %: below the 0.1 % of the rule
            chi = chi * (1 - 5e-4)
        assert s.done and (s.stop, s.it, s.bad) == (mr.STOP_NO_GAIN, 3, 3)
        s = mr.LmState(100.0, 1e5, max_iters=2, T=T)
        assert mr.lm_control(100.0, 50.0, 60.0, True, s) and not s.done and s.nu == 2
        rho = T(50) / (T(60) + T(1e-3))
        assert s.lam == T(1e-5) * T(1e5) * max(T(1) / T(3), min(1 - (2 * rho - 1) ** 3, T(2) / T(3)))
        assert mr.lm_control(50.0, 20.0, 40.0, True, s) and s.done and (s.stop, s.it) == (mr.STOP_ITERATIONS, 2)
        s = mr.LmState(100.0, 1e5, T=T)
        assert not mr.lm_control(100.0, 1.0, 10.0, False, s) and not s.done and s.trials == 1 and s.chi == 100          # solvable or not decides
        # the clamp of the shrink factor: rho near 1 -> 1/3, rho near 1/2 -> 2/3
        for gain, want in ((99.999, T(1) / T(3)), (50.0, T(2) / T(3))):
            s = mr.LmState(100.0, 1e5, T=T)
            mr.lm_control(100.0, 100.0 - gain, 100.0 - 1e-3, True, s)
            assert abs(float(s.lam / (T(1e-5) * T(1e5)) - want)) <= 1e-9
