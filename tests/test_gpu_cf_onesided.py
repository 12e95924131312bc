"""Camera-first elimination, form 3 (esl_cf.hpp, "one-sided assembly"): the interior cameras' part of T from
    X(:, o1)^T X(:, o2) = sum over o1's list entries k at interior slots of the segment of V_k^T Y_slot(k)(o2),   Y = L_ii^T (L_p^-T X),
(k_cf_seg_back + k_cf_T_onesided) instead of the stored per-segment products.  The same linear system as every other form, summed
in another order: it is held against the dense X (ESL_CF_SPARSE=0), the stored products (=1) and the reduced camera system with the
bounds tests/test_gpu_slam.py holds those forms to among themselves, and against itself bit for bit where only the stream order, the
context or the layout's lifetime changes.
"""
import functools

import numpy as np
import pytest

from tests.test_gpu_cf_sep_overlap import ITERS, _awkward_graph, _context, _same_bits, _two_runs
from tests.test_gpu_slam import cam_err, obj_rel

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _graph(n_cams, n_objs, per_cam):
    import importlib
    pkg = importlib.import_module("object-oriented-slam_amd")
    return pkg.synth.make_graph(n_cams, n_objs, per_cam * n_cams, seed=41, slam=True)[:3]


def _first_trial_and_run(pkg, monkeypatch, g, c, o, env, solver):
    """x_c, x_o, chi2 and |S x - b| / |b| of the first trial at lambda = 1e-5 max diag, then a whole LM run with the profile on."""
    if env is None:
        monkeypatch.delenv("ESL_CF_SPARSE", raising=False)
    else:
        monkeypatch.setenv("ESL_CF_SPARSE", env)
    cx = pkg.Context(0)
    try:
        cx.upload_graph(g); cx.upload_states(c, o)
        cx.lm_begin(pkg.default_lm_params(jacobian_mode=1, linear_solver=solver))
        part = cx.lm_linearize()
        tr = cx.lm_try_step(1e-5 * part.max_diag)
        assert cx.lm_solver_used() == solver
        st = cx.lm_solver_stats()
        xc, xo = cx.lm_download(5, 6 * (g.n_cams - 1)), cx.lm_download(2, 9 * g.n_objs)
        res = cx.lm_reduced_residual() if tr.solve_ok == 1 else float("nan")
        cx.lm_commit(False)
        cx.profile_enable(2)
        cc, oo, rep = cx.optimize(g, c, o, pkg.default_lm_params(jacobian_mode=1, linear_solver=solver))
        return dict(xc=xc, xo=xo, chi=tr.chi2, ok=tr.solve_ok, res=res, cams=cc, objs=oo, rep=rep, st=st, classes=set(cx.profile_get()))
    finally:
        cx.close()
        monkeypatch.delenv("ESL_CF_SPARSE", raising=False)


_REFS = {}


def _refs(pkg, monkeypatch, key, g, c, o):
    """The yardsticks of one graph, computed once: dense X, stored products, reduced camera system."""
    if key not in _REFS:
        _REFS[key] = {tag: _first_trial_and_run(pkg, monkeypatch, g, c, o, env, solver)
                      for tag, env, solver in (("dense", "0", 2), ("stored", "1", 2), ("camera", None, 1))}
        assert _REFS[key]["dense"]["st"]["x_form"] == 0 and _REFS[key]["stored"]["st"]["x_form"] == 1
    return _REFS[key]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _hold_against(tag, new, ref, x_tol, chi_tol, trace_tol, state_tol, res_tol=None):
    d_xc, d_xo = _rel(new["xc"], ref["xc"]), _rel(new["xo"], ref["xo"])
    print("form 3 vs %s: x_c %.2e x_o %.2e, |Sx-b|/|b| %.2e, chi2 rel %.2e, run: chi2 rel %.2e cams %.2e objs %.2e" % (
        tag, d_xc, d_xo, new["res"], abs(new["chi"] / ref["chi"] - 1), abs(new["rep"]["chi2_final"] / ref["rep"]["chi2_final"] - 1),
        cam_err(new["cams"], ref["cams"]), obj_rel(new["objs"], ref["objs"])))
    assert new["ok"] == ref["ok"]
    if res_tol is not None:
        assert new["res"] < res_tol
    assert d_xc < x_tol and d_xo < x_tol
    assert new["chi"] == pytest.approx(ref["chi"], rel=chi_tol)
    assert new["rep"]["trace_trials"] == ref["rep"]["trace_trials"]
    np.testing.assert_allclose(new["rep"]["trace_chi2"], ref["rep"]["trace_chi2"], rtol=trace_tol)
    assert cam_err(new["cams"], ref["cams"]) < state_tol and obj_rel(new["objs"], ref["objs"]) < state_tol


@pytest.mark.parametrize("n_cams,n_objs,per_cam", [(257, 40, 6), (300, 80, 10), (500, 50, 10), (1100, 60, 6)])
def test_onesided_equals_dense_rows_stored_products_and_camera_system(pkg, monkeypatch, n_cams, n_objs, per_cam):
    """256 free cameras (the last one IS a separator), 299 (short last segment), 499; 1,099 free cameras = 69 segments: the segment
    bitmaps need a second 64-bit word (the smallest size at which the word loop runs twice)."""
    g, c, o = _graph(n_cams, n_objs, per_cam)
    ref = _refs(pkg, monkeypatch, (n_cams, n_objs, per_cam), g, c, o)
    new = _first_trial_and_run(pkg, monkeypatch, g, c, o, "3", 2)
    st = new["st"]
    assert st["x_form"] == 3 and "sparse_block_products" in new["classes"], st
    assert st["segments"] == (n_cams - 1 + 15) // 16 and st["product_flops"] > 0 and st["product_bytes"] > 0
    if n_cams == 1100:
        assert st["segments"] == 69
    for tag in ("dense", "stored", "camera"):
        _hold_against(tag, new, ref[tag], x_tol=1e-10, chi_tol=1e-12, trace_tol=1e-11, state_tol=1e-9, res_tol=1e-13)


def test_onesided_on_awkward_structures(pkg, monkeypatch):
    """An ellipsoid seen only by separator cameras (no interior entry anywhere), one seen only by the fixed camera, one inside a
    single segment, a segment with no interior observation, a short last segment: against the dense X."""
    g, c, o = _awkward_graph(pkg)
    new = _first_trial_and_run(pkg, monkeypatch, g, c, o, "3", 2)
    ref = _first_trial_and_run(pkg, monkeypatch, g, c, o, "0", 2)
    assert new["st"]["x_form"] == 3 and ref["st"]["x_form"] == 0
    assert new["st"]["separators"] == (g.n_cams - 1) // 16 and new["st"]["segments"] == (g.n_cams - 1 + 15) // 16
    _hold_against("dense (awkward structures)", new, ref, x_tol=1e-9, chi_tol=1e-11, trace_tol=1e-10, state_tol=1e-8)


def _assert_same_runs(a, b):
    for call, (x, y) in enumerate(zip(a, b)):
        assert np.isfinite(y["cams"]).all() and np.isfinite(y["objs"]).all()
        assert list(x["trials"]) == list(y["trials"]), call
        for key in ("cams", "objs", "xc", "xo", "chi2", "lam"):
            assert np.array_equal(np.asarray(x[key]), np.asarray(y[key])) and _same_bits(x[key], y[key]), (call, key)


@pytest.mark.parametrize("n_cams,n_objs,per_cam", [(300, 80, 10), (1100, 60, 6)])
def test_onesided_same_bits_serial_order_side_order_and_fresh_context(pkg, monkeypatch, n_cams, n_objs, per_cam):
    """One arithmetic order for T whatever ESL_CF_OVERLAP is: the serial order, the side-stream order and a rerun of the latter in
    a fresh context give the same bits over two consecutive optimize calls on the resident graph."""
    g, c, o = _graph(n_cams, n_objs, per_cam)
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    runs = []
    for overlap in (False, True, True):
        cx = _context(pkg, monkeypatch, overlap)
        try:
            res, st = _two_runs(pkg, cx, g, c, o)
            assert st["x_form"] == 3
            runs.append(res)
        finally:
            cx.close()
    _assert_same_runs(runs[0], runs[1])
    _assert_same_runs(runs[1], runs[2])
    assert len(runs[1][1]["trials"]) > 0


def test_onesided_trim_between_optimize_calls(pkg, monkeypatch):
    """esl_ctx_trim frees Y with the rest of the layout: the next optimize rebuilds it and gives the bits of a run that never trimmed."""
    g, c, o = _graph(300, 80, 10)
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    p = pkg.default_lm_params(jacobian_mode=1, linear_solver=2, max_iters=ITERS)
    out = {}
    for trim in (False, True):
        cx = _context(pkg, monkeypatch, True)
        try:
            cx.upload_graph(g); cx.upload_states(c, o)
            cx.optimize_resident(p)
            if trim:
                cx.trim()
            rep = cx.optimize_resident(p)
            assert cx.lm_solver_stats()["x_form"] == 3
            out[trim] = (cx.download_states(), rep)
        finally:
            cx.close()
    (s0, r0), (s1, r1) = out[False], out[True]
    assert list(r0["trace_trials"]) == list(r1["trace_trials"]) and _same_bits(r0["trace_chi2"], r1["trace_chi2"])
    assert _same_bits(s0[0], s1[0]) and _same_bits(s0[1], s1[1])


def test_onesided_destroy_straight_after_optimize_resident(pkg, monkeypatch):
    """Destroying the context as soon as optimize_resident has returned, twice: the second context finds the device fit."""
    g, c, o = _graph(300, 80, 10)
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    p = pkg.default_lm_params(jacobian_mode=1, linear_solver=2, max_iters=ITERS)
    reps = []
    for _ in range(2):
        cx = _context(pkg, monkeypatch, True)
        try:
            cx.upload_graph(g); cx.upload_states(c, o)
            reps.append(cx.optimize_resident(p))
        finally:
            cx.close()
    assert list(reps[0]["trace_trials"]) == list(reps[1]["trace_trials"]) and _same_bits(reps[0]["trace_chi2"], reps[1]["trace_chi2"])
    assert reps[0]["chi2_final"] < reps[0]["chi2_initial"]


@pytest.mark.parametrize("env,form", [(None, 3), ("1", 1), ("2", 2)])
def test_default_selection(pkg, monkeypatch, env, form):
    """228 ellipsoids = 2,052 unknowns, the first count at which the library keeps X sparse of its own accord (n_o >= 2048), at the
    256 free cameras the sparse form starts from, with four boxes per camera (the rule also asks the sparse form's flops to be under
    half the dense update's: 0.24 here, 0.8 at eight per camera): unset -> the one-sided form, ESL_CF_SPARSE=1 / 2 -> the stored
    products / the blocks straight from the slabs, as before."""
    g, c, o = _graph(257, 228, 4)
    if env is None:
        monkeypatch.delenv("ESL_CF_SPARSE", raising=False)
    else:
        monkeypatch.setenv("ESL_CF_SPARSE", env)
    cx = pkg.Context(0)
    try:
        cx.upload_graph(g); cx.upload_states(c, o)
        rep = cx.optimize_resident(pkg.default_lm_params(jacobian_mode=1, linear_solver=2, max_iters=1))
        assert cx.lm_solver_used() == 2 and cx.lm_solver_stats()["x_form"] == form
        assert np.isfinite(rep["chi2_final"]) and rep["chi2_final"] < rep["chi2_initial"]
    finally:
        cx.close()
