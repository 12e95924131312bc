"""Extended-precision reference of one MAPPING-mode trial step (every camera fixed: the system is block diagonal, one 9 x 9 block per
ellipsoid), recomputed from the device's OWN linearisation (H_oo, b_o of esl_lm_download) the way tests/slam_step_ref.py does it for SLAM
mode: x_o = (H_oo + lambda I)^-1 b_o per active ellipsoid by iterative refinement on error-free residuals, scale = sum x (lambda x + b)
and the retraction in numpy.longdouble.  Beside it: the same quantities the plain float64 way (the yardsticks a float64 device is measured
against), the trial chi2 from the edges' definitions (tests/lin_ref.py's edge classes, values only) in mpmath and in float64, g2o's
Levenberg control and the project's stop rule restated (lm_control), and CASES, the graphs tests/test_gpu_map_step.py runs (their
premises are asserted on the CPU in tests/test_map_step_ref.py).  The step exists twice on the device -- the step API (k_obj_solve, one
lane per ellipsoid; k_chunk_chi2) and the device-resident loop (k_lm_step_rows, one wave per ellipsoid, lm_decide) -- and both are held to
this one reference.  Test infrastructure; numpy + mpmath."""
import numpy as np

from tests import lin_ref as lr
from tests import slam_step_ref as sr

LD = sr.LD
EPS64 = sr.EPS64
LAM_SMALL, LAM_BIG = sr.LAM_SMALL, sr.LAM_BIG          # dampings as multiples of max_diag; LAM_SMALL is also the default tau
TAU = 1e-5
assert TAU == LAM_SMALL                                   # lambda_0 of a resident run is the small damping of the step-API tests
BBOX_CHUNK, E3D_CHUNK = 64, 32                            # edges per chunk row (csrc/esl_graph_layout.hpp: build_chunks)
STEP_WAVES = 4                                            # ellipsoids per workgroup of k_lm_step_rows (kStepWaves)
LIN_WAVES = 4                                             # chunks per workgroup of the linearisation (kLinWaves), 3-D chunks two per wave
SOLVE_LANES = 64                                          # ellipsoids per workgroup of k_obj_solve
DECIDE_STRIDE = 64 * STEP_WAVES                           # lm_decide's sums over blk_chi and sp_in advance by the workgroup's 256 threads


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
def edges_per_obj(g):
    return (np.bincount(np.asarray(g.bbox_obj, dtype=np.int64), minlength=g.n_objs),
            np.bincount(np.asarray(g.e3d_obj, dtype=np.int64), minlength=g.n_objs))


def chunks_per_obj(g):
    """chunk rows per ellipsoid: its bbox edges by 64, its 3-D edges by 32"""
    nb, ne = edges_per_obj(g)
    return (nb + BBOX_CHUNK - 1) // BBOX_CHUNK + (ne + E3D_CHUNK - 1) // E3D_CHUNK


def lin_blocks(g):
    """workgroups of the resident loop's linearisation (n_lin_blocks of optimize_mapping_device): lm_decide adds one chi2 partial of each"""
    nb, ne = edges_per_obj(g)
    ids_bb, ids_e3 = int(((nb + BBOX_CHUNK - 1) // BBOX_CHUNK).sum()), int(((ne + E3D_CHUNK - 1) // E3D_CHUNK).sum())
    return (ids_e3 + 2 * LIN_WAVES - 1) // (2 * LIN_WAVES) + (ids_bb + LIN_WAVES - 1) // LIN_WAVES


def step_blocks(n_objs):
    return max(1, (n_objs + STEP_WAVES - 1) // STEP_WAVES)


def active_mask(g, flags=None):
    """an ellipsoid without edge and without gravity prior is inactive; so is one flagged fixed (its edges leave the mapping graph)"""
    nb, ne = edges_per_obj(g)
    ng = np.bincount(np.asarray(g.grav_obj, dtype=np.int64), minlength=g.n_objs)
    act = (nb + ne + ng) > 0
    if flags is not None:
        act &= np.asarray(flags).reshape(-1) == 0
    return act


# ---- the step ----------------------------------------------------------------------------------------------------------------------
def blocks_ld(Hoo45, bo):
    Hoo45 = np.asarray(Hoo45)
    N = Hoo45.size // 45
    H = np.array([sr.unpack45(np.asarray(p, dtype=LD)) for p in Hoo45.reshape(N, 45)], dtype=LD).reshape(N, 9, 9)
    return H, np.asarray(bo, dtype=LD).reshape(N, 9)


def reference_step(Hoo45, bo, lam, active):
    """dict(H, b: the blocks in longdouble; x (N, 9), last (N,): solve_ref's solution and last correction per ellipsoid, zero where inactive;
    scale: sum_j x_j (lambda x_j + b_j) in longdouble; backward (N,): |b - (H + lambda I) x| / (|H + lambda I| |x| + |b|) in max-norms, from
    error-free residuals)"""
    H, b = blocks_ld(Hoo45, bo)
    N = len(H)
    lam = LD(lam)
    I9 = np.eye(9, dtype=LD)
    x = np.zeros((N, 9), dtype=LD)
    last, backward = np.zeros(N), np.zeros(N)
    for o in np.nonzero(active)[0]:
        A = H[o] + lam * I9
        x[o], last[o] = sr.solve_ref(A, b[o])
        r = sr.residual_ld(A, x[o], b[o])
        den = float(np.abs(A).sum(axis=1).max()) * float(np.abs(x[o]).max()) + float(np.abs(b[o]).max())
        backward[o] = float(np.abs(r).max()) / den if den > 0 else 0.0
    scale = (x * (lam * x + b))[np.asarray(active, dtype=bool)].sum() if N else LD(0)
    return dict(H=H, b=b, lam=lam, active=np.asarray(active, dtype=bool), x=x, last=last, scale=LD(scale), backward=backward)


def block_err(a, ref):
    """sr.rel_err per ellipsoid (max-norm of the row's error over the row's max-norm), the worst kept: (error, row)"""
    a = np.asarray(a).reshape(len(ref), -1)
    worst, at = 0.0, -1
    for o in range(len(ref)):
        e = sr.rel_err(a[o], ref[o])
        if e > worst:
            worst, at = e, o
    return worst, at


def f64_yardsticks(ref):
    """the step the plain float64 way, twice -- numpy.linalg.solve per block, and numpy.linalg.cholesky per block with two triangular
    solves -- against the reference: dict(x: the larger of the two block_err; x_solve, x_chol; scale: the larger relative error of
    sum x (lambda x + b) formed in float64 from either solution; scale_f64: that sum)"""
    H, b, lam = ref["H"].astype(np.float64), ref["b"].astype(np.float64), float(ref["lam"])
    N = len(H)
    xs, xc = np.zeros((N, 9)), np.zeros((N, 9))
    for o in np.nonzero(ref["active"])[0]:
        A = H[o] + lam * np.eye(9)
        xs[o] = np.linalg.solve(A, b[o])
        L = np.linalg.cholesky(A)
        xc[o] = np.linalg.solve(L.T, np.linalg.solve(L, b[o]))
    out = dict(x_solve=block_err(xs, ref["x"])[0], x_chol=block_err(xc, ref["x"])[0])
    out["x"] = max(out["x_solve"], out["x_chol"])
    sc = [float((x * (lam * x + b))[ref["active"]].sum()) for x in (xs, xc)]
    err = [sr.rel_err([s], [ref["scale"]]) for s in sc]
    out["scale"] = max(err)
    out["scale_f64"] = sc[int(np.argmax(err))]          # the float64 value itself (for the control's yardstick)
    return out


def retract_ld(objs, x, active):
    """trial states: ell (+) x in longdouble for the active ellipsoids, the state itself (exactly) for the others"""
    objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    out = np.array(objs, dtype=LD)
    for o in np.nonzero(active)[0]:
        out[o] = sr.obj_oplus_ld(objs[o], x[o])
    return out


def retract_errors(got, objs, x, active):
    """(worst error of the states `got` against the longdouble retraction of objs by x, worst error of np_oracle's float64 retraction
    against it): sr.state_err relative to max(1, |state|), over the active ellipsoids"""
    objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    got = np.asarray(got).reshape(-1, 10)
    e, y = 0.0, 0.0
    for o in np.nonzero(active)[0]:
        want = sr.obj_oplus_ld(objs[o], x[o])
        s = max(1.0, float(np.abs(want).max()))
        e = max(e, sr.state_err(got[o], want) / s)
        y = max(y, sr.state_err(sr.obj_oplus_f64(objs[o], np.asarray(x[o], dtype=np.float64)), want) / s)
    return e, y


# ---- chi2 of a state from the edges' definitions (values only: lin_ref's edge classes on vertices without unknowns) ---------------------
def _rho0(ar, kind, delta, e):
    """g2o's Huber rho(e) in the arithmetic `ar`; kind None: no kernel"""
    if kind is None:
        return e
    assert kind == "huber"
    d = ar.c(delta)
    return e if e <= d * d else 2 * ar.sqrt(e) * d - d * d


def chi2_at(ar, g, cams, objs, robust=None, skip=None):
    """sum over the edges of rho0(r^T Omega r) at the given states; robust: {class: ("huber", delta)}; skip: ellipsoids whose edges are
    left out (fixed ones).  A box whose outline is no real ellipse must not occur (asserted)."""
    robust = robust or {}
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    skip = np.zeros(g.n_objs, dtype=bool) if skip is None else np.asarray(skip).reshape(-1) != 0
    cv = [lr.cam_vertex(ar, c) for c in cams]
    ov = [lr.obj_vertex(ar, o) for o in objs]
    tot = ar.c(0)
    kb, ke, kg = robust.get("bbox", (None, 0)), robust.get("e3d", (None, 0)), robust.get("grav", (None, 0))
    meas = g.bbox_meas.reshape(-1, 4)
    for k in range(len(g.bbox_cam)):
        a, b = int(g.bbox_cam[k]), int(g.bbox_obj[k])
        if skip[b]:
            continue
        r = lr.edge_bbox(ar, cv[a], ov[b], g.K, [float(v) for v in meas[k]], {})
        assert r is not None, ("a dropped box", k)
        tot = tot + _rho0(ar, kb[0], kb[1], ar.c(g.bbox_weight[k]) * sum((v * v for v in r), ar.c(0)))
    m10 = g.e3d_meas.reshape(-1, 10)
    for k in range(len(g.e3d_cam)):
        a, b = int(g.e3d_cam[k]), int(g.e3d_obj[k])
        if skip[b]:
            continue
        r = lr.edge_e3d(ar, cv[a], ov[b], cv[a], ov[b], m10[k], {})
        tot = tot + _rho0(ar, ke[0], ke[1], ar.c(g.e3d_weight[k]) * sum((v * v for v in r), ar.c(0)))
    for b in np.asarray(g.grav_obj, dtype=np.int64):
        if skip[b]:
            continue
        r = lr.edge_grav(ar, ov[b], g.grav_normal, {})[0]
        tot = tot + _rho0(ar, kg[0], kg[1], ar.c(g.grav_weight) * r * r)
    return tot


def chi2_ref(g, cams, objs, robust=None, skip=None, digits=40):
    """(chi2 at 40 digits, error of the float64 evaluation against it: the yardstick of a chi2 of these states, that float64 value)"""
    mp = lr.MP(digits)
    want = chi2_at(mp, g, cams, objs, robust, skip)
    plain = chi2_at(lr.F64, g, cams, objs, robust, skip)
    return want, lr.rel_err(mp, [plain], [want]), plain


def chi2_err(got, want, digits=40):
    return lr.rel_err(lr.MP(digits), [got], [want])


# ---- Levenberg's control (g2o's OptimizationAlgorithmLevenberg::solve and SparseOptimizer::optimize as this project runs them) ---------
STOP_ITERATIONS, STOP_TRIALS, STOP_NO_GAIN, STOP_EMPTY = 0, 1, 2, 3
RHO_OFFSET = 1e-3           # added to the step's predicted gain before the ratio is formed
GAIN_FACTOR = 1e3           # an iteration whose gain times this is below its first chi2 counts as bad ...
BAD_LIMIT = 3               # ... and this many in a row end the run
# 1 - (2 rho - 1)^3 lies strictly inside [1/3, 2/3] for rho in (0.8467, 0.9368): there, and only there, lambda of an accepted trial moves with rho,
# that is with the summed chi2 AND the summed scale; above it the factor is 1/3 whatever they are
RHO_UNCLAMPED = (0.85, 0.93)


class LmState:
    """What the control carries from trial to trial, in the scalar type T (numpy.longdouble: the reference; numpy.float64: the plain
    way, and the arithmetic of the checker).  trace: per finished iteration (chi2, lambda, trials)."""

    def __init__(self, chi0, max_diag, tau=TAU, max_iters=10, max_trials=10, T=LD):
        self.T = T
        self.max_iters, self.max_trials = int(max_iters), int(max_trials)
        self.lam = T(tau) * T(max_diag)          # computeLambdaInit
        self.nu = T(2)
        self.chi = T(chi0)                       # chi2 of the current estimate
        self.first_chi = T(chi0)                 # ... as the running iteration found it
        self.it = self.trials = self.total_trials = self.bad = 0
        self.rho = None
        self.done, self.stop = self.max_iters <= 0, STOP_ITERATIONS
        self.trace = []


def lm_control(chi_cur, chi_trial, scale, ok, state):
    """One trial's verdict.  chi_cur: chi2 of the current estimate; chi_trial: of the trial states; scale: the step's sum x (lambda x + b);
    ok: every block was solvable.  Updates `state` (lambda, nu, counters, trace, done / stop) and returns whether the trial is accepted.

    The rule: the gain ratio rho = (chi_cur - chi_trial) / (scale + 1e-3), an unsolvable step counting as an infinitely bad trial.  A trial
    with rho > 0 (and a finite chi2) is taken: lambda shrinks by 1 - (2 rho - 1)^3 held within [1/3, 2/3], nu goes back to 2.  Any other
    is refused: lambda grows by nu, nu doubles.  An iteration tries again while rho < 0 and it has trials left.  After an iteration: the
    run ends when the trials ran out or rho is exactly 0; else the iteration is bad if (first chi2 - chi2) 1e3 < first chi2, and three bad
    ones in a row end the run; else when max_iters iterations are done."""
    s, T = state, state.T
    assert not s.done
    chi_cur, chi_trial, scale = T(chi_cur), T(chi_trial), T(scale)
    if not ok:
        chi_trial = T(np.finfo(np.float64).max)
    rho = (chi_cur - chi_trial) / (scale + T(RHO_OFFSET))
    accept = bool(rho > 0) and bool(np.isfinite(chi_trial))
    if accept:
        t = 2 * rho - 1
        alpha = min(1 - t ** 3, T(2) / T(3))
        s.lam = s.lam * max(T(1) / T(3), alpha)
        s.nu = T(2)
        s.chi = chi_trial
    else:
        s.lam = s.lam * s.nu
        s.nu = s.nu * 2
        s.chi = chi_cur
    s.rho = rho
    s.trials += 1
    if rho < 0 and s.trials < s.max_trials:
        return accept
    s.total_trials += s.trials
    s.trace.append((s.chi, s.lam, s.trials))
    if s.trials == s.max_trials or rho == 0:
        s.done, s.stop = True, STOP_TRIALS
    else:
        s.bad = s.bad + 1 if (s.first_chi - s.chi) * T(GAIN_FACTOR) < s.first_chi else 0
        if s.bad >= BAD_LIMIT:
            s.done, s.stop = True, STOP_NO_GAIN
    s.it += 1
    if s.it >= s.max_iters:
        s.done = True
    s.first_chi = s.chi
    s.trials = 0
    return accept


# ---- the checker's system cut into blocks ------------------------------------------------------------------------------------------------
def checker_blocks(po, g, cams, objs, delta=1e-6, group=48):
    """(Hoo45 (N, 45), bo (N, 9), chi2) of oracle/pyoracle.py's build_system, taken in groups of ellipsoids (the system is block diagonal;
    a dense matrix of all of it would not fit for the large case).  An ellipsoid the checker leaves out (no edge) has a zero block."""
    N = g.n_objs
    Hoo, bo, chi = np.zeros((N, 45)), np.zeros((N, 9)), 0.0
    iu = np.triu_indices(9)
    objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    for s in range(0, N, group):
        keep = np.arange(s, min(N, s + group))
        sub = g.subset_objects(keep)
        H, b, fidx, c = po.build_system(sub, cams, objs[keep], delta=delta)
        chi += c
        for k, o in enumerate(keep):
            i = int(fidx[g.n_cams + k])
            if i >= 0:
                Hoo[o] = H[i:i + 9, i:i + 9][iu]
                bo[o] = b[i:i + 9]
    return Hoo, bo, chi


def checker_chi2(po, g, cams, objs, group=48):
    return checker_blocks(po, g, cams, objs, group=group)[2]


def checker_run(po, g, cams, objs, state, delta=1e-6, hook=None):
    """The checker's mapping-mode LM replayed trial by trial on its own pieces -- build_system for H, b and chi2, its pivoted LDLT per block
    (ldlt_solve), its retraction (obj_oplus) -- with lm_control (on `state`) taking the decisions.  Returns (objs, trials): per trial
    dict(it, lam, chi_cur, chi_trial, scale, ok, rho, accept)."""
    objs = np.array(objs, dtype=np.float64).reshape(-1, 10)
    act = active_mask(g)
    trials = []
    while not state.done:
        Hoo, bo, chi = checker_blocks(po, g, cams, objs, delta)
        it = state.it
        while not state.done and state.it == it:
            lam = float(state.lam)
            trial = objs.copy()
            scale, ok = 0.0, True
            for o in np.nonzero(act)[0]:
                good, x = po.ldlt_solve(sr.unpack45(Hoo[o]) + lam * np.eye(9), bo[o])
                ok = ok and good
                for j in range(9):
                    scale += x[j] * (lam * x[j] + bo[o, j])
                trial[o] = po.obj_oplus(objs[o], x)
            chi_trial = checker_chi2(po, g, cams, trial)
            accept = lm_control(chi, chi_trial, scale, ok, state)
            trials.append(dict(it=it, lam=lam, chi_cur=chi, chi_trial=chi_trial, scale=scale, ok=ok, rho=float(state.rho), accept=accept))
            if hook:
                hook(trials[-1])
            if accept:
                objs = trial
                chi = chi_trial
    return objs, trials


# ---- the graphs of tests/test_gpu_map_step.py ----------------------------------------------------------------------------------------------
def _rows_scene():
    """Seven ellipsoids before 130 cameras on an arc, their chunk rows 1, 7, 1, 4 | 5, 1, 6: the ellipsoid with seven rows (130 bbox edges = 3
    rows, 100 3-D edges = 4) is wave 1 of the first workgroup of k_lm_step_rows, between two ellipsoids of one row; the one with exactly
    four (65 + 40 edges) is wave 3; the second workgroup holds five rows (65 + 65 edges) on wave 0 and six (65 + 97) on wave 2"""
    b = lr._Build(21)
    n = 130
    for i in range(n):
        a = -1.25 + 2.5 * i / (n - 1)
        b.cam([3.3 * np.cos(a), 3.3 * np.sin(a), 1.1 + 0.2 * np.sin(3 * a)], [0.0, 0.0, 0.35], roll=0.05 * np.cos(5 * a))
    place = [([-0.45, 0.5, 0.3], [0.01, -0.02, 0.4], [0.2, 0.25, 0.3]), ([0.0, 0.15, 0.35], [0.01, 0.02, -0.7], [0.4, 0.25, 0.35]),
             ([0.35, -0.55, 0.3], [-0.02, 0.01, 0.3], [0.2, 0.3, 0.3]), ([-0.5, -0.45, 0.25], [0.02, 0.02, 1.1], [0.25, 0.2, 0.25]),
             ([0.55, 0.55, 0.3], [-0.01, 0.03, -0.2], [0.3, 0.2, 0.3]), ([0.0, -0.9, 0.2], [0.02, -0.01, 0.9], [0.2, 0.2, 0.2]),
             ([0.6, -0.1, 0.28], [0.0, 0.02, 2.0], [0.22, 0.3, 0.28])]
    o = [b.obj(*p) for p in place]
    for oi, (nb, ne) in zip(o, ROWS_EDGES):
        for i in range(nb):
            b.bbox(i, oi)
        for i in range(ne):
            b.e3d(n - 1 - i, oi)
        b.grav(oi)
    return b.graph()


ROWS_EDGES = ((1, 0), (130, 100), (3, 0), (65, 40), (65, 65), (2, 0), (65, 97))          # (bbox, 3-D) edges per ellipsoid of _rows_scene
ROWS_CHUNKS = (1, 7, 1, 4, 5, 1, 6)


def _deficient_graph(pkg):
    """the graph of test_rank_deficient_ellipsoid_blocks_take_the_oracles_decisions: ellipsoid 1 keeps one bbox edge (rank 4), 2 only the
    gravity prior (rank 1), 3 nothing at all (inactive); here ellipsoid 5 is flagged fixed on top"""
    g0, c, o, _ = pkg.synth.make_graph(30, 6, 300, seed=12)
    keep = np.ones(len(g0.bbox_obj), bool)
    for obj, n_keep in ((1, 1), (2, 0), (3, 0)):
        idx = np.nonzero(g0.bbox_obj == obj)[0]
        keep[idx[n_keep:]] = False
    k3 = ~np.isin(g0.e3d_obj, [1, 2, 3])
    g = pkg.Graph(g0.K, g0.n_cams, g0.n_objs, None, g0.bbox_cam[keep], g0.bbox_obj[keep], g0.bbox_meas.reshape(-1, 4)[keep],
                  g0.bbox_weight[keep], g0.e3d_cam[k3], g0.e3d_obj[k3], g0.e3d_meas.reshape(-1, 10)[k3], g0.e3d_weight[k3],
                  np.array([0, 2, 4, 5]), g0.grav_normal, g0.grav_weight)
    return g, c, o


def _between(truth, start, s):
    """ellipsoids on the way from the true ones (s = 0) to make_graph's start (s = 1): centres and scales on the line, the quaternion on the
    chord and normalised"""
    q0, q1 = truth[:, 3:7], start[:, 3:7] * np.where((truth[:, 3:7] * start[:, 3:7]).sum(axis=1, keepdims=True) < 0, -1.0, 1.0)
    out = (1 - s) * truth + s * start
    q = (1 - s) * q0 + s * q1
    out[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return out


def _trimmed(pkg, g, lo, hi, e3d_max):
    """the graph with ellipsoid o keeping its first lo + o % (hi - lo + 1) bbox edges and its first e3d_max 3-D edges"""
    def first(obj, limit):
        rank = np.zeros(len(obj), dtype=np.int64)
        seen = {}
        for k, o in enumerate(obj.tolist()):
            rank[k] = seen.get(o, 0)
            seen[o] = rank[k] + 1
        return rank < limit(np.asarray(obj, dtype=np.int64))
    kb = first(g.bbox_obj, lambda o: lo + o % (hi - lo + 1))
    ke = first(g.e3d_obj, lambda o: np.full(len(o), e3d_max))
    return pkg.Graph(g.K, g.n_cams, g.n_objs, None, g.bbox_cam[kb], g.bbox_obj[kb], g.bbox_meas.reshape(-1, 4)[kb], g.bbox_weight[kb],
                     g.e3d_cam[ke], g.e3d_obj[ke], g.e3d_meas.reshape(-1, 10)[ke], g.e3d_weight[ke], g.grav_obj, g.grav_normal, g.grav_weight)


SMALL_ARGS = dict(n_cams=30, n_objs=6, n_bbox_target=300, seed=12)
LANES_ARGS = dict(n_cams=40, n_objs=65, n_bbox_target=600, seed=5)
LARGE_ARGS = dict(n_cams=60, n_objs=1030, n_bbox_target=20000, seed=7, frac_3d=0.02)
LARGE_START = 4.5             # ellipsoids 4.5 times as far from the truth as make_graph starts them: the single trial at lambda_0 is then accepted
                              # with a gain ratio of 0.90 (from make_graph's own start it is refused, rho -0.48, with 2 or 3 boxes per ellipsoid)
LARGE_TRIM = (2, 3, 1)        # 2 or 3 bbox edges and at most one 3-D edge per ellipsoid
ROBUST_ARGS = dict(n_cams=30, n_objs=6, n_bbox_target=200, seed=3)
NUMERIC_ARGS = dict(n_cams=30, n_objs=6, n_bbox_target=200, seed=4)

# name: dict(kind, ...; premises asserted by tests/test_map_step_ref.py::test_case_premises):
#   "make": make_graph(**args) in mapping mode, `take`: its first so many ellipsoids;  "rows": _rows_scene in mapping mode (lin_ref's builders);
#   "deficient": _deficient_graph, `fixed`: ellipsoids flagged through obj_fixed
#   N ellipsoids; chunks: rows of the ellipsoid with the most; inactive: ellipsoids the step must not touch; jac: jacobian_mode (1 analytic);
#   robust: Huber on these classes (widths: robust_widths); lock: run in the lock-step test (its checker run has a rejected trial and three
#   iterations or more, away from every threshold: test_map_step_ref.py::test_lock_step_cases_are_away_from_thresholds)
# Boundaries, smallest shape that crosses each:
#   kStepWaves = 4 (ellipsoids per workgroup of k_lm_step_rows): N = 1, 3 (part of one), 4 (one, full), 5 (a second with one wave live)
#   k_obj_solve's 64 lanes: N = 63, 64 (one workgroup, full), 65 (a second with one lane live)
#   lm_decide's strided sums (stride 256): N = 1030 -> 258 step workgroups and, every ellipsoid holding a bbox chunk, 258 + 40 = 298
#     linearisation workgroups: both loops take a second pass (in 2 and in 42 lanes).  Its start (LARGE_START) makes the single resident trial
#     an ACCEPTED one with rho inside RHO_UNCLAMPED, so that chi2_final is the sum over all 298 + 258 partials and lambda_final moves with it
#     and with the summed scale: a partial left out of either sum shows in both
#   chunk rows: 1, 4 (the preloaded rows exactly), 5 (one row in the serial tail), 6, 7 -- "rows"; lin_ref's long_ellipsoid has exactly 5, on wave 0
CASES = {
    "N1": dict(kind="make", args=SMALL_ARGS, take=1, N=1, chunks=2),
    "N3": dict(kind="make", args=SMALL_ARGS, take=3, N=3, chunks=2),
    "N4": dict(kind="make", args=SMALL_ARGS, take=4, N=4, chunks=2),
    "N5": dict(kind="make", args=SMALL_ARGS, take=5, N=5, chunks=2, lock=True),
    "N63": dict(kind="make", args=LANES_ARGS, take=63, N=63, chunks=2),
    "N64": dict(kind="make", args=LANES_ARGS, take=64, N=64, chunks=2),
    "N65": dict(kind="make", args=LANES_ARGS, take=65, N=65, chunks=2, lock=True),
    "large": dict(kind="make", args=LARGE_ARGS, trim=LARGE_TRIM, start=LARGE_START, N=1030, chunks=2, step_blocks=258, lin_blocks=298),
    "rows": dict(kind="rows", N=7, chunks=7, lock=True),
    "long_ellipsoid": dict(kind="scene", scene="long_ellipsoid", N=2, chunks=5),
    "deficient": dict(kind="deficient", fixed=(5,), N=6, chunks=2, inactive=(3, 5)),
    "robust": dict(kind="make", args=ROBUST_ARGS, N=6, chunks=2, robust=("bbox", "grav")),
    "numeric": dict(kind="make", args=NUMERIC_ARGS, N=6, chunks=2, jac=0),
}
NUMERIC_DELTA = 1e-6          # of the numeric-Jacobian case (the checker's delta in every comparison of this suite)

_built = {}


def build_case(pkg, name):
    """(graph, cameras, ellipsoids, obj_fixed flags or None) of one row of CASES, built once per process"""
    if name in _built:
        return _built[name]
    c = CASES[name]
    flags = None
    if c["kind"] == "make":
        key = ("make", tuple(sorted(c["args"].items())))
        if key not in _built:
            _built[key] = pkg.synth.make_graph(**c["args"])
        g, cams, objs, truth = _built[key]
        if c.get("start") is not None:
            objs = _between(truth["objs"], objs, c["start"])
        if c.get("take"):
            keep = np.arange(c["take"])
            g, objs = g.subset_objects(keep), objs[keep].copy()
        if c.get("trim"):
            g = _trimmed(pkg, g, *c["trim"])
    elif c["kind"] == "rows":
        g, cams, objs = _rows_scene()
        g = lr.mapping_graph(g)
    elif c["kind"] == "scene":
        g, cams, objs = lr.scene(c["scene"])
        g = lr.mapping_graph(g)
    else:
        g, cams, objs = _deficient_graph(pkg)
    if c.get("fixed"):
        flags = np.zeros(g.n_objs, np.uint8)
        flags[list(c["fixed"])] = 1
    _built[name] = (g, np.ascontiguousarray(cams, dtype=np.float64), np.ascontiguousarray(objs, dtype=np.float64), flags)
    return _built[name]


def seen_graph(g, flags):
    """the graph a mapping-mode run sees: without the edges of the ellipsoids flagged fixed"""
    if flags is None:
        return g
    from tests import fixed_ref as fr
    return fr.without_edges_of(g, flags)


def lm_params(pkg, name, **kw):
    c = CASES[name]
    return pkg.default_lm_params(jacobian_mode=c.get("jac", 1), numeric_delta=NUMERIC_DELTA if c.get("jac", 1) == 0 else 1e-9, **kw)


def robust_widths(g, cams, objs, classes):
    """Huber width per class: the root of the median raw chi2 of the class's edges, so that both branches are taken"""
    from tests import robust_ref as rr
    return {k: ("huber", float(np.sqrt(np.median(rr.edge_chi2(g, cams, objs, k)[0])))) for k in classes}
