"""Camera-first elimination, the rank-K update capped to one workgroup per CU so that the segments' products are resident beside it
(esl_slam.hip, slam_try_step_cf; ESL_CF_OVERLAP=4, the default).  The cap is launch LDS only -- no kernel's arithmetic and no address
changes -- so a context created with ESL_CF_OVERLAP=0 (everything in stream order, uncapped) and one created with 4 must agree BIT
FOR BIT: states, traces, x_c and x_o, over two consecutive optimize calls on the resident graph.

The cap applies where the update runs on k_chol_update_v in its assign form, i.e. where the whole lower triangle of T passes the
launcher's size rule (1,024 tiles of 256 x 128): from order 8,073 = 897 ellipsoids on (tests/test_update_v_applies.py).  The graphs
here are that one -- the smallest that runs the capped launch -- and the one an ellipsoid below it, which must take the uncapped,
unassigned order whatever the switch says; which side a graph is on is asked of the library's own rule (pkg.lib.update_v_applies).
Equality at C4 itself stays with tests/test_gpu_fullsize.py (its default context is a capped one)."""
import os

import numpy as np
import pytest

from test_gpu_cf_sep_overlap import ITERS, _awkward_graph, _same_bits, _two_runs

pytestmark = pytest.mark.gpu

N_CAP = 897   # the smallest number of ellipsoids whose T (order 8,073) takes the capped launch


@pytest.fixture(autouse=True)
def _sparse_form(monkeypatch):
    """X kept sparse with stored products -- the form with a side stream -- also on these graphs (299 free cameras, ~900 ellipsoids), which the
    library would run with the dense X (tests/test_gpu_cf_sep_overlap.py forces it the same way)."""
    monkeypatch.setenv("ESL_CF_SPARSE", "1")


def _context(pkg, overlap):
    """A context whose ESL_CF_OVERLAP was `overlap` when it was created (read there and kept in the context); None: unset."""
    saved = os.environ.pop("ESL_CF_OVERLAP", None)
    try:
        if overlap is not None:
            os.environ["ESL_CF_OVERLAP"] = str(overlap)
        return pkg.Context(0)
    finally:
        os.environ.pop("ESL_CF_OVERLAP", None)
        if saved is not None:
            os.environ["ESL_CF_OVERLAP"] = saved


def _assign_form(pkg, n_objs):
    n_o = 9 * n_objs
    ld = (n_o + 1 + 127) // 128 * 128
    return pkg.lib.update_v_applies(ld, n_o + 1, 0, n_o, True, ld)


class _Serial:
    """Graphs and their serial-order runs, each made once for the module; the serial contexts stay alive beside the ones under test."""

    def __init__(self, pkg):
        self.pkg, self.graphs, self.runs, self.ctxs = pkg, {}, {}, []

    def graph(self, n_objs):
        if n_objs not in self.graphs:
            self.graphs[n_objs] = self.pkg.synth.make_graph(300, n_objs, 30 * n_objs, seed=41, slam=True)[:3]
        return self.graphs[n_objs]

    def run(self, n_objs):
        if n_objs not in self.runs:
            cx = _context(self.pkg, 0)
            self.ctxs.append(cx)
            self.runs[n_objs] = _two_runs(self.pkg, cx, *self.graph(n_objs))
        return self.runs[n_objs]

    def close(self):
        for cx in self.ctxs:
            cx.close()


@pytest.fixture(scope="module")
def serial(pkg):
    s = _Serial(pkg)
    yield s
    s.close()


def _check(pkg, serial, n_objs, overlap):
    cx = _context(pkg, overlap)
    try:
        got, st1 = _two_runs(pkg, cx, *serial.graph(n_objs))
    finally:
        cx.close()
    ref, st0 = serial.run(n_objs)
    assert st0 == st1 and st1["x_form"] == 1, st1
    for call, (a, b) in enumerate(zip(ref, got)):
        assert np.isfinite(b["cams"]).all() and np.isfinite(b["objs"]).all()
        assert list(a["trials"]) == list(b["trials"]), call
        for key in ("cams", "objs", "xc", "xo", "chi2", "lam"):
            assert _same_bits(a[key], b[key]), (call, key)
    assert len(got[1]["trials"]) > 0 and got[0]["chi2"][-1] < got[0]["chi2"][0]   # (the second call ran trials of its own; chi2 fell)


@pytest.mark.parametrize("overlap", [4, None, 1])
def test_capped_update_equals_serial_order(pkg, serial, overlap):
    """The smallest graph with the capped launch: the cap (4), the default (unset: the same), and the uncapped side order (1)."""
    assert _assign_form(pkg, N_CAP)
    _check(pkg, serial, N_CAP, overlap)


def test_one_ellipsoid_below_the_assign_form(pkg, serial):
    """No assign form, so no update beside the products and nothing to cap: the products run beside k_cf_forward<1> alone."""
    assert not _assign_form(pkg, N_CAP - 1)
    _check(pkg, serial, N_CAP - 1, 4)


def test_trim_between_optimize_calls(pkg, serial):
    """esl_ctx_trim between two calls of a capped context: the next optimize rebuilds the layout and gives the bits of a run that
    never trimmed."""
    g, c, o = serial.graph(N_CAP)
    p = pkg.default_lm_params(jacobian_mode=1, linear_solver=2, max_iters=ITERS)
    ref = serial.run(N_CAP)[0][1]
    cx = _context(pkg, 4)
    try:
        cx.upload_graph(g); cx.upload_states(c, o)
        cx.optimize_resident(p)
        cx.trim()
        rep = cx.optimize_resident(p)
        assert cx.lm_solver_stats()["x_form"] == 1
        cams, objs = cx.download_states()
    finally:
        cx.close()
    assert list(rep["trace_trials"]) == list(ref["trials"]) and _same_bits(rep["trace_chi2"], ref["chi2"])
    assert _same_bits(cams, ref["cams"]) and _same_bits(objs, ref["objs"])


def test_destroy_straight_after_optimize_resident(pkg, serial):
    """Destroying a capped context as soon as optimize_resident has returned: the device is fit for the next context."""
    g, c, o = serial.graph(N_CAP)
    p = pkg.default_lm_params(jacobian_mode=1, linear_solver=2, max_iters=ITERS)
    ref = serial.run(N_CAP)[0][0]
    for _ in range(2):
        cx = _context(pkg, 4)
        try:
            cx.upload_graph(g); cx.upload_states(c, o)
            rep = cx.optimize_resident(p)
        finally:
            cx.close()
        assert list(rep["trace_trials"]) == list(ref["trials"]) and _same_bits(rep["trace_chi2"], ref["chi2"])


def test_awkward_structures_are_untouched_by_the_new_value(pkg):
    """The awkward-structure graph of tests/test_gpu_cf_sep_overlap.py (order 126: no assign form): value 4 runs it as value 1 does,
    and that is the serial order's bits."""
    g, c, o = _awkward_graph(pkg)
    cxs = [_context(pkg, 0), _context(pkg, 4)]
    try:
        (a, st0), (b, st1) = [_two_runs(pkg, cx, g, c, o) for cx in cxs]
    finally:
        for cx in cxs:
            cx.close()
    assert st0 == st1 and st1["x_form"] == 1 and st1["separators"] == (g.n_cams - 1) // 16
    for call in range(2):
        assert list(a[call]["trials"]) == list(b[call]["trials"])
        for key in ("cams", "objs", "xc", "xo", "chi2", "lam"):
            assert _same_bits(a[call][key], b[call][key]), (call, key)
