"""The mapping-mode LM step on the device, in BOTH of its forms, against the extended-precision step of tests/map_step_ref.py recomputed
from the device's OWN linearisation (H_oo, b_o of esl_lm_download), on the graphs of map_step_ref.CASES (their premises:
tests/test_map_step_ref.py):

  (a) the step API (esl_lm_try_step: k_obj_solve, one lane per ellipsoid with the block in registers; k_chunk_chi2), under the dampings
      1e-5 max_diag and 1e4 max_diag: x_o, the trial ellipsoids, scale, solve_ok, and the trial chi2 against mpmath at 40 digits on the
      edges' definitions and against esl_lm_linearize at the uploaded trial states;
  (b) one trial of the device-resident loop (esl_optimize_resident with max_iters = max_trials = 1: k_lm_step_rows, one wave per
      ellipsoid, lm_solve9_rows, the inline gravity prior; lm_decide at the head of the next launch) at lambda_0 = tau max_diag: its x_o,
      its states, chi2_final, lambda_final and the counters against the reference and lm_control;
  (c) a whole resident run against the same start replayed through the step API with map_step_ref.lm_control taking every decision;
  (d) the two forms' x_o beside each other (printed, not asserted).

Boundaries and the case that crosses each: kStepWaves = 4 -- N1, N3, N4, N5; k_obj_solve's 64 lanes -- N63, N64, N65; lm_decide's sums
with stride 256 over more than 256 step workgroups and more than 256 linearisation workgroups -- large (1030 ellipsoids: 258 and 298),
through (b): its trial is accepted with rho 0.90, inside the window (0.847, 0.937) where lambda's factor 1 - (2 rho - 1)^3 is off both
clamps, so chi2_final is the sum of all 298 + 258 partials and lambda_final moves with that sum and with the summed scale (asserted on the
CPU and again on the device's blocks).  Every other accepted case of (b) has rho above 0.937, where lambda_final is lambda_0 / 3 whatever
the resident form's scale is: the scale of k_lm_step_rows and its sum in lm_decide are pinned by large in (b) and by the lambda traces of
(c), nowhere else.  Chunk rows per ellipsoid 1, 4, 5, 6, 7 with the longest on wave 1 between one-row ellipsoids -- rows (and long_ellipsoid: 5
on wave 0): the "> 4 chunks" tail of k_lm_step_rows is a real path, taken by every ellipsoid with more than 4 rows; rank-deficient,
empty and fixed blocks -- deficient; Huber on the bbox and the gravity class with residuals on both sides of delta -- robust; the inline
numeric gravity prior -- numeric.

Tolerances (the rule of tests/test_gpu_slam_step.py).  The device's error against the reference (x_o: max-norm of an ellipsoid's error over
its max-norm, the worst ellipsoid; scalars: relative; states: slam_step_ref.state_err over max(1, |state|)) may be at most MARGIN x
yardstick + 4 eps, the yardstick being the error of the plain float64 way on the same quantity of the same case (numpy.linalg.solve and
numpy Cholesky per block, the larger; float64 sums; np_oracle's retraction; the float64 evaluation of the edges' definitions; lm_control in
float64) -- never the device's output.  One margin per group, the next power of two at or above 4 x the worst ratio (device error /
yardstick, an error within 4 eps counting as 0) measured on the MI355X over this module:

    solves (x_o)                  worst 11.53  (N1, the resident form: 1.48e-15 against a yardstick of 1.28e-16; the step API on the
                                               same block: 1.18e-16; the step API's worst: 4.99, the one-edge block of deficient)  -> MARGIN_SOLVE   = 64
    scalars (scale, chi2, lambda) worst 10.78  (N1, lambda 1e-5 max_diag, trial chi2 of both forms: 6.11e-15 against 5.66e-16)     -> MARGIN_SCALAR  = 64
    retractions                   worst  2.46  (large, the states of the resident trial: 1.04e-15 against 4.23e-16; the step API on
                                               large: 2.06; every other case within 4 eps of the longdouble retraction)            -> MARGIN_RETRACT = 16

Per family of cases (solves / scalars / retractions): N1 .. N65 11.53 / 10.78 / 0.00, large 0.70 / 1.00 / 2.46, rows 1.42 / 1.47 / 0.00,
long_ellipsoid 0.68 / 0.00 / 0.00, deficient 4.99 / 0.43 / 0.00, robust 3.92 / 0.84 / 0.00, numeric 0.23 / 1.31 / 0.00.  scale and
chi2_initial were within 4 eps everywhere, lambda_final too but on large (9.7e-16, equal to its yardstick; chi2_final there 4.8e-16).  The
two forms' x_o (d): 1e-15 .. 6e-13 of max |x_o| apart, no row bit-equal but the two inactive rows of deficient.  No finding in the arithmetic
of either form: nothing is further from the reference than 12 times what plain float64 arithmetic leaves.

A ratio above 64 would not be a margin to adopt but a finding in the kernels.  Every ratio is printed by every run (-s), the worst ones
when the module's context closes.  (lm_solve9_rows multiplies by 1 / d_k where k_obj_solve divides: about an eps, inside the margin.)

In (c) the two runs are both the device's, and their states part by what their steps differ.  That is bounded to first order, from the
replay's own figures and before any comparison: B, the sum over the accepted trials of (MARGIN_SOLVE x that trial's x_o yardstick + 4 eps)
max |x_o| + 4 eps for the retraction, bounds the distance of the states; 2 G B / chi2, G the 1-norm of the gradient b_o of the iteration's
linearisation, what that moves chi2 by; and, d_rho = 2 (2 G B + scalar allowance x chi2) / (scale + 1e-3) being what it moves a gain ratio by,
18 d_rho per accepted trial what it moves lambda by (|d/d rho (1 - (2 rho - 1)^3)| <= 6, the factor >= 1/3).  The resident trace is held to
the replayed one within the scalar allowance plus these slacks -- the yardstick of chi2 being the larger of the float64 evaluation's errors
at the start and at the final states, that of lambda the distance of the float64 control from the longdouble one on the same scalars --
and the final states within B.  Measured: the same trials per iteration, iterations and stop reason on N5 ([1, 1, 5, 1, 3, 1], no gain), N65
([1, 3, 1, 3, 1, 2, 2, 3, 1, 2], 10 iterations) and rows ([1, 2, 1, 1, 1, 2, 1], no gain); trace chi2 at most 7.7e-14 apart (slack 4e-10),
trace lambda 1.2e-13 (slack 1.8e-8), final states 3.9e-14 (B = 3.9e-11): the slacks are worst-case sums and three orders wide, so what (c)
pins is the sequence of decisions and agreement to 1e-10, not the last digits -- those are (a)'s and (b)'s.  Its ratios are printed under
"lock-step" and are not part of the margins.  The numeric-Jacobian case is not run in lock-step: central differences turn the last bit of a state
into 1e-10 of H_oo, so two runs of it part by 1e-8 after the first accepted step whatever the step kernels do.

Finding.  x_o of an inactive or fixed ellipsoid was not written by either form, so esl_lm_download(2) returned what an earlier graph had
left there (include/esl.h promised zeros for a fixed ellipsoid with esl_graph_upload_fixed, which only the SLAM kernel kept; its note on
esl_lm_download now says so for every ellipsoid that takes no step); both kernels now store the zeros.  test_inactive_rows_read_zero_after_another_graph is the
smallest shape that showed it.
"""
import numpy as np
import pytest

from tests import map_step_ref as mr
from tests import slam_step_ref as sr

pytestmark = pytest.mark.gpu

LD = sr.LD
FLOOR = 4 * sr.EPS64
MARGIN_SOLVE = 64.0         # x_o
MARGIN_SCALAR = 64.0        # scale, chi2, lambda
MARGIN_RETRACT = 16.0       # trial states
YARDSTICK_CAP = 1e-9
DAMPINGS = (mr.LAM_SMALL, mr.LAM_BIG)

WORST = {}                  # group -> (ratio, where)
FAMILY = {}                 # (family, group) -> ratio
STEPS = {}                  # (case, damping) -> Step: shared by (a), (b) and (d)


def allow(margin, yardstick):
    return margin * yardstick + FLOOR


def family(name):
    return "N" if name[0] == "N" else name


def note(group, where, err, yardstick):
    ratio = 0.0 if err <= FLOOR else (err / yardstick if yardstick > 0 else float("inf"))
    if ratio > WORST.get(group, (-1.0, ""))[0]:
        WORST[group] = (ratio, where)
    key = (family(where.split()[0]), group)
    FAMILY[key] = max(FAMILY.get(key, 0.0), ratio)
    return ratio


@pytest.fixture(scope="module")
def cx(pkg):
    """a context of this module's own: the robust setting belongs to the context"""
    c = pkg.Context(0)
    yield c
    c.set_robust()
    c.close()
    print("\nworst ratios device error / float64 yardstick over the module: " +
          ", ".join("%s %.2f (%s)" % (k, v[0], v[1]) for k, v in sorted(WORST.items())))
    fams = sorted({k[0] for k in FAMILY})
    print("per family (solve / scalar / retract): " + ", ".join(
        "%s %s" % (f, " / ".join("%.2f" % FAMILY[(f, g)] if (f, g) in FAMILY else "-" for g in ("solve", "scalar", "retract"))) for f in fams))


class Step:
    """everything one trial step of the step API leaves, and its reference"""


def robust_of(name, g, c, o):
    cls = mr.CASES[name].get("robust")
    return mr.robust_widths(g, c, o, cls) if cls else None


def load(pkg, cx, name, objs=None):
    """the case's graph and states (or `objs` in their place) on the context, its robust setting made the context's"""
    g, c, o, flags = mr.build_case(pkg, name)
    robust = robust_of(name, g, c, o)
    cx.set_robust(**(robust or {}))
    cx.upload_graph(g, obj_fixed=flags)
    cx.upload_states(c, o if objs is None else objs)
    return g, c, o, flags, robust


def step_of(pkg, cx, name, f):
    """(a)'s run of one case under one damping, once per process: begin, linearise, the blocks, the trial step with lambda = f max_diag, its
    downloads, commit(False); then the linearisation at the uploaded trial states; the reference and the yardsticks on the blocks"""
    if (name, f) in STEPS:
        return STEPS[(name, f)]
    g, c, o, flags, robust = load(pkg, cx, name)
    N = g.n_objs
    s = Step()
    s.act = mr.active_mask(g, flags)
    nv, nd = cx.lm_begin(mr.lm_params(pkg, name))
    assert nd == 0                                   # no dropped box: every edge is in the sums
    s.part = cx.lm_linearize()
    s.lam = f * s.part.max_diag
    s.Hoo, s.bo = cx.lm_download(0, N * 45).reshape(N, 45), cx.lm_download(1, N * 9).reshape(N, 9)
    s.out = cx.lm_try_step(s.lam)
    s.xo, s.objs = cx.lm_download(2, N * 9).reshape(N, 9), cx.lm_download(7, N * 10).reshape(N, 10)
    cx.lm_commit(False)
    cx.upload_states(c, s.objs)
    assert cx.lm_begin(mr.lm_params(pkg, name))[1] == 0
    s.chi_lin = cx.lm_linearize().chi2
    s.ref = mr.reference_step(s.Hoo, s.bo, s.lam, s.act)
    s.y = mr.f64_yardsticks(s.ref)
    xmax = np.abs(s.ref["x"]).max(axis=1).astype(np.float64)
    assert (s.ref["last"][s.act] <= 1e-3 * sr.EPS64 * xmax[s.act]).all()          # the reference has converged
    # a yardstick beyond the cap means the reference, not float64, is off, and would only widen what the device is allowed
    assert s.y["x"] <= YARDSTICK_CAP and s.y["scale"] <= YARDSTICK_CAP, s.y
    s.chi_ref, s.y_chi, s.chi_f64 = mr.chi2_ref(g, c, s.objs, robust, flags)
    assert s.y_chi <= YARDSTICK_CAP
    STEPS[(name, f)] = s
    return s


@pytest.mark.parametrize("name", list(mr.CASES))
def test_step_api_trial_matches_extended_precision(pkg, cx, name):
    """(a)"""
    g, c, o, flags = mr.build_case(pkg, name)
    bad = []
    for f in DAMPINGS:
        where = "%s lambda %.0e" % (name, f)
        s = step_of(pkg, cx, name, f)
        ref, y, act = s.ref, s.y, s.act
        e_x, at = mr.block_err(s.xo, ref["x"])
        want_scale = (np.asarray(s.xo, dtype=LD) * (ref["lam"] * np.asarray(s.xo, dtype=LD) + ref["b"]))[act].sum()
        e_s, e_s_own = sr.rel_err([s.out.scale], [ref["scale"]]), sr.rel_err([s.out.scale], [want_scale])
        e_r, y_r = mr.retract_errors(s.objs, o, s.xo, act)
        e_c, e_l = mr.chi2_err(s.out.chi2, s.chi_ref), mr.chi2_err(s.chi_lin, s.chi_ref)
        e_cl = abs(s.out.chi2 - s.chi_lin) / abs(s.chi_lin)
        print("%s: x_o %.2e at ellipsoid %d (yardstick %.2e, ratio %.2f); scale %.2e (yardstick %.2e, ratio %.2f), from its own x_o %.2e; trial states "
              "%.2e (yardstick %.2e, ratio %.2f); trial chi2 %.2e, of the linearisation %.2e (yardstick %.2e, ratios %.2f, %.2f), the two apart %.2e"
              % (where, e_x, at, y["x"], note("solve", where + " x_o", e_x, y["x"]), e_s, y["scale"], note("scalar", where + " scale", e_s, y["scale"]),
                 e_s_own, e_r, y_r, note("retract", where + " trial states", e_r, y_r), e_c, e_l, s.y_chi,
                 note("scalar", where + " trial chi2", e_c, s.y_chi), note("scalar", where + " chi2 of the linearisation", e_l, s.y_chi), e_cl))
        assert s.out.solve_ok == 1, where
        # inactive and fixed ellipsoids: x_o exactly zero, the trial state the state bit for bit
        assert not s.xo[~act].any(), (where, np.nonzero(s.xo.any(axis=1) & ~act)[0])
        assert np.array_equal(s.objs[~act], o[~act]), where
        assert not ref["H"][~act].any() and not ref["b"][~act].any(), where
        for q in np.nonzero(act)[0]:
            assert abs(float(np.asarray(s.objs[q, 3:7], dtype=LD) @ np.asarray(s.objs[q, 3:7], dtype=LD)) - 1) <= 1e-15
        if not e_x <= allow(MARGIN_SOLVE, y["x"]):
            bad.append((where, "x_o", e_x, y["x"]))
        if not e_s <= allow(MARGIN_SCALAR, y["scale"]):
            bad.append((where, "scale", e_s, y["scale"]))
        if not e_s_own <= allow(MARGIN_SCALAR, y["scale"]):
            bad.append((where, "scale of its own x_o", e_s_own, y["scale"]))
        if not e_r <= allow(MARGIN_RETRACT, y_r):
            bad.append((where, "trial states", e_r, y_r))
        if not e_c <= allow(MARGIN_SCALAR, s.y_chi):
            bad.append((where, "trial chi2", e_c, s.y_chi))
        if not e_l <= allow(MARGIN_SCALAR, s.y_chi):
            bad.append((where, "chi2 of the linearisation at the trial states", e_l, s.y_chi))
        if not e_cl <= allow(MARGIN_SCALAR, s.y_chi):
            bad.append((where, "trial chi2 against the linearisation's", e_cl, s.y_chi))
    assert not bad, bad


def control_of(s, T, chi_trial, scale, **kw):
    st = mr.LmState(s.part.chi2, s.part.max_diag, T=T, **kw)
    mr.lm_control(s.part.chi2, chi_trial, scale, True, st)
    return st


@pytest.mark.parametrize("name", list(mr.CASES))
def test_one_resident_trial_matches_extended_precision(pkg, cx, name):
    """(b), and (d) beside it"""
    where = "%s resident" % name
    s = step_of(pkg, cx, name, mr.TAU)
    ref, y, act = s.ref, s.y, s.act
    g, c, o, flags, robust = load(pkg, cx, name)
    N = g.n_objs
    rep = cx.optimize_resident(mr.lm_params(pkg, name, max_iters=1, max_trials=1, tau=mr.TAU))
    xo = cx.lm_download(2, N * 9).reshape(N, 9)
    cams, objs = cx.download_states()
    # the reference's verdict on this trial, and the plain float64 way's
    ctl = control_of(s, LD, s.chi_ref, ref["scale"], max_iters=1, max_trials=1)
    plain = control_of(s, np.float64, s.chi_f64, y["scale_f64"], max_iters=1, max_trials=1)
    rho = float(ctl.rho)
    assert float(plain.rho) * rho > 0
    if name == "large":          # the case for lm_decide's strided sums: accepted, lambda's factor off both clamps (on the device's blocks too)
        assert mr.RHO_UNCLAMPED[0] < rho < mr.RHO_UNCLAMPED[1], rho
        assert 1 / 3 < float(ctl.lam) / s.lam < 2 / 3 and rep["chi2_final"] != rep["chi2_initial"]
    e_x, at = mr.block_err(xo, ref["x"])
    if rho > 0:          # chi2_final is the chi2 of THIS form's trial states (a rounding of x_o away from the step API's): the reference at those
        chi_own, y_chi, chi_own_f64 = mr.chi2_ref(g, c, objs, robust, flags)
        e_chi = mr.chi2_err(rep["chi2_final"], chi_own)
        ctl = control_of(s, LD, chi_own, ref["scale"], max_iters=1, max_trials=1)          # ... and lambda_final follows that chi2
        plain = control_of(s, np.float64, chi_own_f64, y["scale_f64"], max_iters=1, max_trials=1)
        assert float(ctl.rho) > 0 and abs(float(ctl.rho) - rho) <= 1e-9
    else:
        e_chi, y_chi = abs(rep["chi2_final"] - s.part.chi2) / s.part.chi2, 0.0
    y_lam = sr.rel_err([plain.lam], [ctl.lam])
    e_lam = sr.rel_err([rep["lambda_final"]], [ctl.lam])
    print("%s: rho %.3g; x_o %.2e at ellipsoid %d (yardstick %.2e, ratio %.2f); lambda_final %.2e (yardstick %.2e, ratio %.2f); chi2_final %.2e (yardstick "
          "%.2e, ratio %.2f)" % (where, rho, e_x, at, y["x"], note("solve", where + " x_o", e_x, y["x"]), e_lam, y_lam,
                                note("scalar", where + " lambda_final", e_lam, y_lam), e_chi, y_chi, note("scalar", where + " chi2_final", e_chi, y_chi)))
    # (d) the two forms beside each other
    d = sr.rel_err(xo, s.xo) if N else 0.0
    print("%s: x_o of the two forms %.2e apart (of max |x_o|), %d of %d rows bit-equal" % (where, d, int((xo == s.xo).all(axis=1).sum()), N))
    assert (rep["iterations"], rep["total_trials"], rep["stop_reason"]) == (1, 1, mr.STOP_TRIALS) == (ctl.it, ctl.total_trials, ctl.stop)
    assert rep["n_bbox_dropped"] == 0 and rep["trace_trials"] == [1]
    assert abs(rep["chi2_initial"] - s.part.chi2) <= FLOOR * s.part.chi2
    assert not xo[~act].any(), (where, np.nonzero(xo.any(axis=1) & ~act)[0])
    assert np.array_equal(cams, c)
    assert e_x <= allow(MARGIN_SOLVE, y["x"]), (where, e_x, y["x"])
    assert e_lam <= allow(MARGIN_SCALAR, y_lam), (where, e_lam, y_lam)
    assert e_chi <= allow(MARGIN_SCALAR, y_chi), (where, e_chi, y_chi)
    assert rep["trace_chi2"] == [rep["chi2_final"]] and rep["trace_lambda"] == [rep["lambda_final"]]
    if abs(rho) < 1e-3:          # (at most one case of the table: test_one_trial_cases_near_rho_zero_are_at_most_one)
        print("%s: rho within 1e-3 of 0: the states are not compared" % where)
        return
    if rho > 0:
        e_r, y_r = mr.retract_errors(objs, o, xo, act)
        print("%s: accepted; states %.2e (yardstick %.2e, ratio %.2f)" % (where, e_r, y_r, note("retract", where + " states", e_r, y_r)))
        assert e_r <= allow(MARGIN_RETRACT, y_r), (where, e_r, y_r)
        assert np.array_equal(objs[~act], o[~act])
    else:
        assert np.array_equal(objs, o), where


def replay(pkg, cx, name, p, y_chi):
    """The run of test (c) through the step API: lm_control (longdouble) decides from the device's step-API scalars; the float64 control
    runs beside it on the same scalars.  Returns (control, float64 control, final states, per finished iteration (B, slack of chi2, slack
    of lambda)): what the other form's run may be away from this one's because its steps are (docstring of the module)."""
    g, c, o, flags, robust = load(pkg, cx, name)
    N = g.n_objs
    act = mr.active_mask(g, flags)
    assert cx.lm_begin(p)[1] == 0
    part = cx.lm_linearize()
    ctl = mr.LmState(part.chi2, part.max_diag, p.tau, p.max_iters, p.max_trials, T=LD)
    plain = mr.LmState(part.chi2, part.max_diag, p.tau, p.max_iters, p.max_trials, T=np.float64)
    chi, B, lam_slack, slack = part.chi2, 0.0, 0.0, []
    G = float(np.abs(cx.lm_download(1, N * 9)).sum())          # |gradient|_1 of the current linearisation
    while not ctl.done:
        lam, it = float(ctl.lam), ctl.it
        out = cx.lm_try_step(lam)
        accept = mr.lm_control(chi, out.chi2, out.scale, out.solve_ok == 1, ctl)
        assert mr.lm_control(chi, out.chi2, out.scale, out.solve_ok == 1, plain) == accept and plain.done == ctl.done
        assert abs(float(ctl.rho)) >= 1e-3, (name, float(ctl.rho))          # (the premise, on the device's scalars)
        if accept:
            ref = mr.reference_step(cx.lm_download(0, N * 45), cx.lm_download(1, N * 9), lam, act)
            B += allow(MARGIN_SOLVE, mr.f64_yardsticks(ref)["x"]) * float(np.abs(ref["x"]).max()) + FLOOR
            d_rho = 2 * (2 * G * B + allow(MARGIN_SCALAR, y_chi) * chi) / (out.scale + mr.RHO_OFFSET)
            lam_slack += 18 * d_rho
            chi = out.chi2
        cx.lm_commit(accept)
        if ctl.it != it:
            slack.append((B, 2 * G * B / chi, lam_slack))
        if accept and not ctl.done:
            cx.lm_linearize()
            G = float(np.abs(cx.lm_download(1, N * 9)).sum())
    return ctl, plain, cx.download_states()[1], slack


@pytest.mark.parametrize("name", [k for k, v in mr.CASES.items() if v.get("lock")])
def test_resident_run_in_lock_step_with_the_step_api(pkg, cx, name):
    """(c)"""
    g, c, o, flags, robust = load(pkg, cx, name)
    p = mr.lm_params(pkg, name)
    rep = cx.optimize_resident(p)
    _, objs = cx.download_states()
    y_start = mr.chi2_ref(g, c, o, robust, flags)[1]
    ctl, plain, objs_replay, slack = replay(pkg, cx, name, p, y_start)
    trials = [n for _, _, n in ctl.trace]
    print("%s: %d iterations, trials %s, stop %d (resident: %s, stop %d)" % (name, ctl.it, trials, ctl.stop, rep["trace_trials"], rep["stop_reason"]))
    # no decision sits at a threshold (tests/test_map_step_ref.py): a differing sequence is a finding, not noise
    assert rep["trace_trials"] == trials
    assert (rep["iterations"], rep["total_trials"], rep["stop_reason"]) == (ctl.it, ctl.total_trials, ctl.stop)
    assert any(n > 1 for n in trials) and ctl.it >= 3 and len(slack) == ctl.it
    y_chi = max(y_start, mr.chi2_ref(g, c, objs_replay, robust, flags)[1])
    y_lam = max(sr.rel_err([b[1]], [a[1]]) for a, b in zip(ctl.trace, plain.trace))
    e_chi = [sr.rel_err([got], [want[0]]) for got, want in zip(rep["trace_chi2"], ctl.trace)]
    e_lam = [sr.rel_err([got], [want[1]]) for got, want in zip(rep["trace_lambda"], ctl.trace)]
    e_st = max(sr.state_err(objs[q], objs_replay[q]) / max(1.0, float(np.abs(objs_replay[q]).max())) for q in range(g.n_objs))
    where = "%s lock-step" % name
    print("%s: trace chi2 %.2e (yardstick %.2e, ratio %.2f; slack from the states up to %.2e), trace lambda %.2e (yardstick %.2e, ratio %.2f; slack up "
          "to %.2e), final states %.2e (budget %.2e)"
          % (where, max(e_chi), y_chi, note("lock-step", where + " trace chi2", max(e_chi), y_chi), max(k[1] for k in slack), max(e_lam), y_lam,
             note("lock-step", where + " trace lambda", max(e_lam), y_lam), slack[-1][2], e_st, slack[-1][0]))
    for k in range(ctl.it):
        assert e_chi[k] <= allow(MARGIN_SCALAR, y_chi) + slack[k][1], (where, k, e_chi[k], y_chi, slack[k])
        assert e_lam[k] <= allow(MARGIN_SCALAR, y_lam) + slack[k][2], (where, k, e_lam[k], y_lam, slack[k])
    assert rep["chi2_final"] == rep["trace_chi2"][-1] and rep["lambda_final"] == rep["trace_lambda"][-1]
    assert e_st <= slack[-1][0], (where, e_st, slack[-1][0])


def test_inactive_rows_read_zero_after_another_graph(pkg, cx):
    """The smallest shape at which x_o of an inactive ellipsoid did not read as zero: the rank-deficient case (ellipsoid 3 without any edge,
    ellipsoid 5 fixed) on a context whose work area a graph with steps on all of its rows has been through (here N65) -- neither
    k_obj_solve nor k_lm_step_rows wrote those rows, and esl_lm_download(2) returned what the earlier graph had left there."""
    g, c, o, flags, _ = load(pkg, cx, "N65")
    cx.lm_begin(mr.lm_params(pkg, "N65"))
    part = cx.lm_linearize()
    cx.lm_try_step(mr.LAM_SMALL * part.max_diag)
    assert cx.lm_download(2, g.n_objs * 9).reshape(-1, 9)[:6].all(axis=1).all()
    cx.lm_commit(False)
    g, c, o, flags, _ = load(pkg, cx, "deficient")
    act = mr.active_mask(g, flags)
    cx.lm_begin(mr.lm_params(pkg, "deficient"))
    part = cx.lm_linearize()
    cx.lm_try_step(mr.LAM_SMALL * part.max_diag)
    xo = cx.lm_download(2, g.n_objs * 9).reshape(-1, 9)
    cx.lm_commit(False)
    assert not xo[~act].any() and xo[act].any(axis=1).all()
    load(pkg, cx, "N65")
    cx.optimize_resident(mr.lm_params(pkg, "N65", max_iters=1, max_trials=1))
    load(pkg, cx, "deficient")
    cx.optimize_resident(mr.lm_params(pkg, "deficient", max_iters=1, max_trials=1))
    xo = cx.lm_download(2, g.n_objs * 9).reshape(-1, 9)
    assert not xo[~act].any() and xo[act].any(axis=1).all()
