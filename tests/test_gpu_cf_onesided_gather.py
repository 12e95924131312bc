"""The one-sided assembly fed whole records through LDS (esl_cf.hpp k_cf_T_onesided_lds, the default of form 3) against the per-lane
gather it replaces (k_cf_T_onesided, ESL_CF_OS_KERNEL=0 when the context is created): the same MFMAs on the same operands in the
same order, so everything is compared bit for bit.  The new kernel reads a pair list of element offsets, the old one a list of
record numbers; each context builds its own list at layout time, so the comparison covers the list as well.  esl_lm_download(6)
returns the reduced camera system of solver 1, not this solver's T, and is not compared.  The premises on the blocks' lengths that
these graphs are chosen for are asserted on the CPU in tests/test_cf_onesided_pairs.py.
"""
import numpy as np
import pytest

from tests.test_gpu_cf_onesided import _assert_same_runs, _graph
from tests.test_gpu_cf_sep_overlap import _awkward_graph, _same_bits, _two_runs

pytestmark = pytest.mark.gpu


def _context(pkg, monkeypatch, kernel, overlap=None):
    """A context whose ESL_CF_OS_KERNEL (and ESL_CF_OVERLAP) were these when it was created; both are read there and kept."""
    monkeypatch.setenv("ESL_CF_OS_KERNEL", kernel)
    if overlap is not None:
        monkeypatch.setenv("ESL_CF_OVERLAP", overlap)
    try:
        return pkg.Context(0)
    finally:
        monkeypatch.delenv("ESL_CF_OS_KERNEL", raising=False)
        monkeypatch.delenv("ESL_CF_OVERLAP", raising=False)


def _first_trial(pkg, cx, g, c, o):
    cx.upload_graph(g); cx.upload_states(c, o)
    cx.lm_begin(pkg.default_lm_params(jacobian_mode=1, linear_solver=2))
    part = cx.lm_linearize()
    tr = cx.lm_try_step(1e-5 * part.max_diag)
    assert cx.lm_solver_used() == 2
    out = dict(xc=cx.lm_download(5, 6 * (g.n_cams - 1)), xo=cx.lm_download(2, 9 * g.n_objs), chi=tr.chi2, ok=tr.solve_ok)
    cx.lm_commit(False)
    return out


def _everything(pkg, cx, g, c, o):
    first = _first_trial(pkg, cx, g, c, o)
    runs, st = _two_runs(pkg, cx, g, c, o)
    assert st["x_form"] == 3, st
    return first, runs, st


def _assert_same(a, b):
    (fa, ra, sa), (fb, rb, sb) = a, b
    assert fa["ok"] == fb["ok"] == 1
    assert np.isfinite(fb["xc"]).all() and np.isfinite(fb["xo"]).all()
    for key in ("xc", "xo", "chi"):
        assert np.array_equal(np.asarray(fa[key]), np.asarray(fb[key])) and _same_bits(fa[key], fb[key]), key
    _assert_same_runs(ra, rb)
    assert len(rb[1]["trials"]) > 0
    assert sa == sb


def _new_and_old(pkg, monkeypatch, g, c, o, overlap=None):
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    res = []
    for kernel in ("1", "0"):
        cx = _context(pkg, monkeypatch, kernel, overlap)
        try:
            res.append(_everything(pkg, cx, g, c, o))
        finally:
            cx.close()
    _assert_same(res[0], res[1])
    return res[0]


@pytest.mark.parametrize("n_cams,n_objs,per_cam", [(257, 40, 6), (300, 80, 10), (500, 50, 10), (1100, 60, 6)])
def test_lds_assembly_equals_lane_gather_bit_for_bit(pkg, monkeypatch, n_cams, n_objs, per_cam):
    """Empty blocks, blocks of one pair, of exactly one and two batches (8, 16 pairs), of one and several lists of 64, odd lengths
    (half a K-step of padding), b rows up to 219 entries; two bitmap words at 1,100 cameras."""
    g, c, o = _graph(n_cams, n_objs, per_cam)
    _new_and_old(pkg, monkeypatch, g, c, o)


def test_lds_assembly_on_awkward_structures(pkg, monkeypatch):
    g, c, o = _awkward_graph(pkg)
    _new_and_old(pkg, monkeypatch, g, c, o)


def test_lds_assembly_serial_order_and_smaller_graph_after_larger(pkg, monkeypatch):
    """ESL_CF_OVERLAP=0 (every launch in stream order), and a context that ran a larger graph first: the smaller graph's layout
    reuses the arena, the images in LDS and the list are rebuilt -- the same bits as a context that only ever saw the smaller graph."""
    g, c, o = _graph(300, 80, 10)
    ref = _new_and_old(pkg, monkeypatch, g, c, o, overlap="0")
    gl, cl, ol = _graph(500, 50, 10)
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    cx = _context(pkg, monkeypatch, "1")
    try:
        _everything(pkg, cx, gl, cl, ol)
        again = _everything(pkg, cx, g, c, o)
    finally:
        cx.close()
    _assert_same(ref, again)
