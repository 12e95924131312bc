"""Form 3 with Y built in one two-directional ("twisted") sweep per segment and no interior slab (csrc/esl_cf_sweep.hpp: k_cf_twist,
k_cf_sweep, k_cf_wxo, k_cf_z_fwd; the default) against the parent's slab sweeps (ESL_CF_SWEEP=0 when the context is created:
k_cf_forward<2> + k_cf_seg_back + the slab's z), against the dense X (ESL_CF_SPARSE=0) and against the reduced camera system.  The
sweep solves each segment from both ends instead of by substitution -- the same Y up to rounding (tests/test_cf_twisted.py: held to
4 cond(G_p) eps on the CPU) -- so it is held to the bounds tests/test_gpu_cf_stride.py holds another elimination order to;
ESL_CF_SWEEP=0 against itself, and the sweep under another stream order or after a larger graph in the same context, bit for bit.
The column kinds these graphs contain (one head at either end or in the middle of a segment, several heads, twins, a short last
segment) are asserted on the CPU in tests/test_cf_twisted.py.
"""
import numpy as np
import pytest

from tests.test_gpu_cf_onesided import _first_trial_and_run, _graph, _hold_against, _refs
from tests.test_gpu_cf_onesided_gather import _assert_same, _everything
from tests.test_gpu_cf_sep_overlap import _awkward_graph
from tests.test_gpu_cf_stride import _awkward_graph32

pytestmark = pytest.mark.gpu

# tests/test_gpu_cf_stride.py's bounds
TIGHT = dict(x_tol=1e-10, chi_tol=1e-12, trace_tol=1e-11, state_tol=1e-9, res_tol=1e-13)
AWKWARD = dict(x_tol=1e-9, chi_tol=1e-11, trace_tol=1e-10, state_tol=1e-8)


def _env(monkeypatch, **kw):
    for k, v in kw.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _run(pkg, monkeypatch, g, c, o, sweep, stride=None, sparse="3", solver=2):
    """first trial and a whole run (tests/test_gpu_cf_onesided.py) in a context created with these switches"""
    _env(monkeypatch, ESL_CF_SWEEP=sweep, ESL_CF_STRIDE=stride)
    try:
        return _first_trial_and_run(pkg, monkeypatch, g, c, o, sparse, solver)
    finally:
        _env(monkeypatch, ESL_CF_SWEEP=None, ESL_CF_STRIDE=None)


def _context(pkg, monkeypatch, sweep, overlap=None, stride=None):
    _env(monkeypatch, ESL_CF_SWEEP=sweep, ESL_CF_OVERLAP=overlap, ESL_CF_STRIDE=stride)
    try:
        return pkg.Context(0)
    finally:
        _env(monkeypatch, ESL_CF_SWEEP=None, ESL_CF_OVERLAP=None, ESL_CF_STRIDE=None)


@pytest.mark.parametrize("n_cams,n_objs,per_cam,stride", [(257, 40, 6, None), (257, 40, 6, 32), (257, 40, 6, 48), (300, 80, 10, None), (300, 80, 10, 32),
                                                          (300, 80, 10, 48), (1100, 60, 6, None)])
def test_sweep_equals_slab_sweeps_dense_rows_and_camera_system(pkg, monkeypatch, n_cams, n_objs, per_cam, stride):
    """Strides 32 and 48 forced on 256 and 299 free cameras: a short last segment; 1,099 free cameras: two bitmap words."""
    g, c, o = _graph(n_cams, n_objs, per_cam)
    ref = _refs(pkg, monkeypatch, (n_cams, n_objs, per_cam), g, c, o)
    new = _run(pkg, monkeypatch, g, c, o, None, stride)
    old = _run(pkg, monkeypatch, g, c, o, "0", stride)
    assert new["st"] == old["st"] and new["st"]["x_form"] == 3 and new["st"]["stride"] == (stride or 16), new["st"]
    assert list(new["rep"]["trace_trials"]) == list(old["rep"]["trace_trials"])
    for tag, other in (("the slab sweeps", old), ("dense", ref["dense"]), ("camera", ref["camera"])):
        _hold_against("%s, stride %s" % (tag, stride), new, other, **TIGHT)


@pytest.mark.parametrize("which", ["16", "32"])
def test_sweep_on_awkward_structures(pkg, monkeypatch, which):
    g, c, o = _awkward_graph(pkg) if which == "16" else _awkward_graph32(pkg)
    stride = None if which == "16" else 32
    new = _run(pkg, monkeypatch, g, c, o, None, stride)
    old = _run(pkg, monkeypatch, g, c, o, "0", stride)
    dense = _first_trial_and_run(pkg, monkeypatch, g, c, o, "0", 2)
    camera = _first_trial_and_run(pkg, monkeypatch, g, c, o, None, 1)
    assert new["st"] == old["st"] and new["st"]["x_form"] == 3 and dense["st"]["x_form"] == 0
    assert list(new["rep"]["trace_trials"]) == list(old["rep"]["trace_trials"])
    for tag, other in (("the slab sweeps", old), ("dense", dense), ("camera", camera)):
        _hold_against("%s (awkward structures, stride %s)" % (tag, which), new, other, **AWKWARD)


def test_slab_sweeps_twice_and_each_form_in_either_stream_order_bit_for_bit(pkg, monkeypatch):
    """ESL_CF_SWEEP=0 in two contexts (the parent's arrays); each form with ESL_CF_OVERLAP=0 and unset: one arithmetic order whatever
    the streams do."""
    g, c, o = _graph(300, 80, 10)
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    res = {}
    for key, sweep, overlap in (("old", "0", None), ("old again", "0", None), ("old serial", "0", "0"), ("new", None, None), ("new serial", None, "0")):
        cx = _context(pkg, monkeypatch, sweep, overlap)
        try:
            res[key] = _everything(pkg, cx, g, c, o)
        finally:
            cx.close()
    _assert_same(res["old"], res["old again"])
    _assert_same(res["old"], res["old serial"])
    _assert_same(res["new"], res["new serial"])
    (fn, rn, _), (fo, ro, _) = res["new"], res["old"]
    assert [list(r["trials"]) for r in rn] == [list(r["trials"]) for r in ro]
    assert not np.array_equal(fn["xo"], fo["xo"])     # (another route to Y: the two do differ)


def test_smaller_graph_after_larger_in_one_context(pkg, monkeypatch):
    """A context that ran a larger graph first: the arena is reused, P, Q, the last slots' rows and the by-slot index are laid out
    again -- the bits of a context that only ever saw the smaller graph.  Stride 32 forced: a short last segment in both."""
    g, c, o = _graph(300, 80, 10)
    gl, cl, ol = _graph(500, 50, 10)
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    cx = _context(pkg, monkeypatch, None, stride=32)
    try:
        alone = _everything(pkg, cx, g, c, o)
    finally:
        cx.close()
    cx = _context(pkg, monkeypatch, None, stride=32)
    try:
        _everything(pkg, cx, gl, cl, ol)
        again = _everything(pkg, cx, g, c, o)
    finally:
        cx.close()
    _assert_same(alone, again)
