"""The one-sided assembly on the list with twins merged and the shorter side walked (esl_cf.hpp k_cf_os_list, k_cf_v_merge; the default
of form 3) against the parent's list (ESL_CF_OS_LIST=0 when the context is created: the row side over every entry, from V), against
the dense X (ESL_CF_SPARSE=0) and against the reduced camera system.  The new list adds the same products in another association --
(V_a + V_b)^T Y for V_a^T Y + V_b^T Y, and Y(o1)^T V for V^T Y(o1) transposed -- so it is held to the bounds
tests/test_gpu_cf_stride.py holds another elimination order to; ESL_CF_OS_LIST=0 against itself, and either list under another
stream order or after a larger graph in the same context, bit for bit.  The premises on the graphs (blocks that walk the column
side, ties, mixed blocks, runs of two, the block lengths) are asserted on the CPU in tests/test_cf_os_sides.py.
"""
import numpy as np
import pytest

from tests import cf_os_sides_ref as sides
from tests import cf_plan_ref
from tests.test_gpu_cf_onesided import _assert_same_runs, _first_trial_and_run, _graph, _hold_against, _refs
from tests.test_gpu_cf_onesided_gather import _assert_same, _everything
from tests.test_gpu_cf_sep_overlap import _awkward_graph
from tests.test_gpu_cf_stride import _awkward_graph32

pytestmark = pytest.mark.gpu

TIGHT = dict(x_tol=1e-10, chi_tol=1e-12, trace_tol=1e-11, state_tol=1e-9, res_tol=1e-13)
AWKWARD = dict(x_tol=1e-9, chi_tol=1e-11, trace_tol=1e-10, state_tol=1e-8)


def _env(monkeypatch, **kw):
    for k, v in kw.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _run(pkg, monkeypatch, g, c, o, os_list, stride=None, sparse="3", solver=2):
    """first trial and a whole run (tests/test_gpu_cf_onesided.py) in a context created with these switches"""
    _env(monkeypatch, ESL_CF_OS_LIST=os_list, ESL_CF_STRIDE=stride)
    try:
        return _first_trial_and_run(pkg, monkeypatch, g, c, o, sparse, solver)
    finally:
        _env(monkeypatch, ESL_CF_OS_LIST=None, ESL_CF_STRIDE=None)


def _context(pkg, monkeypatch, os_list, overlap=None, stride=None):
    _env(monkeypatch, ESL_CF_OS_LIST=os_list, ESL_CF_OVERLAP=overlap, ESL_CF_STRIDE=stride)
    try:
        return pkg.Context(0)
    finally:
        _env(monkeypatch, ESL_CF_OS_LIST=None, ESL_CF_OVERLAP=None, ESL_CF_STRIDE=None)


@pytest.mark.parametrize("n_cams,n_objs,per_cam,stride", [(257, 40, 6, None), (257, 40, 6, 32), (257, 40, 6, 48), (300, 80, 10, None), (300, 80, 10, 32),
                                                          (300, 80, 10, 48), (500, 50, 10, None), (1100, 60, 6, None)])
def test_merged_shorter_side_list_equals_parent_list_dense_rows_and_camera_system(pkg, monkeypatch, n_cams, n_objs, per_cam, stride):
    """Strides 32 and 48 forced on 256 and 299 free cameras: a short last segment; 1,099 free cameras: two bitmap words."""
    g, c, o = _graph(n_cams, n_objs, per_cam)
    ref = _refs(pkg, monkeypatch, (n_cams, n_objs, per_cam), g, c, o)
    new = _run(pkg, monkeypatch, g, c, o, None, stride)
    old = _run(pkg, monkeypatch, g, c, o, "0", stride)
    assert new["st"] == old["st"] and new["st"]["x_form"] == 3 and new["st"]["stride"] == (stride or 16), new["st"]
    assert "sparse_block_products" in new["classes"]
    assert list(new["rep"]["trace_trials"]) == list(old["rep"]["trace_trials"])
    for tag, other in (("the parent's list", old), ("dense", ref["dense"]), ("camera", ref["camera"])):
        _hold_against("%s, stride %s" % (tag, stride), new, other, **TIGHT)


@pytest.mark.parametrize("which", ["16", "32"])
def test_merged_shorter_side_list_on_awkward_structures(pkg, monkeypatch, which):
    g, c, o = _awkward_graph(pkg) if which == "16" else _awkward_graph32(pkg)
    stride = None if which == "16" else 32
    new = _run(pkg, monkeypatch, g, c, o, None, stride)
    old = _run(pkg, monkeypatch, g, c, o, "0", stride)
    dense = _first_trial_and_run(pkg, monkeypatch, g, c, o, "0", 2)
    camera = _first_trial_and_run(pkg, monkeypatch, g, c, o, None, 1)
    assert new["st"] == old["st"] and new["st"]["x_form"] == 3 and dense["st"]["x_form"] == 0
    for tag, other in (("the parent's list", old), ("dense", dense), ("camera", camera)):
        _hold_against("%s (awkward structures, stride %s)" % (tag, which), new, other, **AWKWARD)


def test_parent_list_twice_and_each_list_in_either_stream_order_bit_for_bit(pkg, monkeypatch):
    """ESL_CF_OS_LIST=0 in two contexts; each list with ESL_CF_OVERLAP=0 and unset: one arithmetic order whatever the streams do."""
    g, c, o = _graph(300, 80, 10)
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    res = {}
    for key, os_list, overlap in (("old", "0", None), ("old again", "0", None), ("old serial", "0", "0"), ("new", None, None), ("new serial", None, "0")):
        cx = _context(pkg, monkeypatch, os_list, overlap)
        try:
            res[key] = _everything(pkg, cx, g, c, o)
        finally:
            cx.close()
    _assert_same(res["old"], res["old again"])
    _assert_same(res["old"], res["old serial"])
    _assert_same(res["new"], res["new serial"])
    (fn, rn, _), (fo, ro, _) = res["new"], res["old"]
    assert [list(r["trials"]) for r in rn] == [list(r["trials"]) for r in ro]
    assert not np.array_equal(fn["xo"], fo["xo"])     # (another association of the sums: the lists do differ)


def test_smaller_graph_after_larger_rebuilds_list_and_merged_records(pkg, monkeypatch):
    """A context that ran a larger graph first: the arena is reused, the list and Vm are rebuilt -- the bits of a context that only
    ever saw the smaller graph.  Stride 32 forced: a short last segment in both."""
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


def test_counts_of_the_list_the_device_built_are_the_host_plan(pkg, monkeypatch, tmp_path):
    """esl_lm_os_counts after one trial equals what tests/cf_os_sides_main.cpp, compiled here, prints for the same lists and switches
    (the library checks the list it fills against the same length, so a trial that ran built a list of exactly that many pairs)."""
    g, c, o = _graph(300, 80, 10)
    exe = sides.build(tmp_path)
    assert exe, "no host compiler"
    L = cf_plan_ref.lists(g)
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    for os_list, stride in ((None, None), (None, 48), ("0", 32)):
        cx = _context(pkg, monkeypatch, os_list, stride=stride)
        try:
            assert not any(cx.lm_os_counts().values())
            cx.upload_graph(g); cx.upload_states(c, o)
            cx.lm_begin(pkg.default_lm_params(jacobian_mode=1, linear_solver=2))
            tr = cx.lm_try_step(1e-5 * cx.lm_linearize().max_diag)
            assert tr.solve_ok == 1 and cx.lm_solver_used() == 2
            got = cx.lm_os_counts()
        finally:
            cx.close()
        pl = sides.run(exe, L, tmp_path, os_list=0 if os_list == "0" else 1, sparse=3, stride=stride or 0)
        print("ESL_CF_OS_LIST", os_list, "ESL_CF_STRIDE", stride, got)
        want = [pl["os_npairs"], pl["osm_row_npairs"], pl["osm_npairs"], pl["os_list_npairs"], pl["osm_flops"] if pl["os_list"] else pl["os_flops"],
                8.0 * pl["os_list_npairs"]]
        assert list(got.values()) == [float(x) for x in want], (got, want)
        assert got["list_pairs"] == (got["row_side_pairs"] if os_list == "0" else got["merged_shorter_side_pairs"]) > 0
    monkeypatch.setenv("ESL_CF_SPARSE", "1")     # another form: no list, zeros
    cx = pkg.Context(0)
    try:
        cx.upload_graph(g); cx.upload_states(c, o)
        cx.lm_begin(pkg.default_lm_params(jacobian_mode=1, linear_solver=2))
        cx.lm_try_step(1e-5 * cx.lm_linearize().max_diag)
        assert cx.lm_solver_stats()["x_form"] == 1 and not any(cx.lm_os_counts().values())
    finally:
        cx.close()
