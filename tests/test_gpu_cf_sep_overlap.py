"""Camera-first elimination, the side-stream order of a trial (esl_slam.hip, slam_try_step_cf): the separators' chain beside the
interior rows' pipeline, the segments' products beside the separators' forward recurrence.  No kernel's arithmetic and no address
changes, so a context created with ESL_CF_OVERLAP=0 (everything in stream order) and one created with the switch on must agree
BIT FOR BIT -- states, traces, x_c and x_o -- over two consecutive optimize calls on the resident graph (the second call is the one
a missing dependency between trial t's readers and trial t + 1's side-stream writers would show in).

The side order needs X kept sparse with stored products, which the library offers from 256 free cameras on with the stride fixed
at 16 (ESL_CF_SPARSE=1 forces it below its size threshold, as tests/test_gpu_slam.py does).  Two structures one might want are
therefore out of reach of the code under test and are replaced by the nearest the library can run:
  * a 100-camera graph is dissected (7 segments) but keeps X dense: it runs here as a graph on the UNTOUCHED dissected path;
  * "exactly two segments, one separator" cannot occur in any form (dissection starts at 48 free cameras = 3 segments; the sparse
    form has at least 16): the smallest sparse chain, 256 free cameras whose last camera IS a separator, stands in for it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = 3


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def _context(pkg, monkeypatch, overlap):
    """A context whose ESL_CF_OVERLAP was `overlap` when it was created (the switch is read there and kept in the context): False /
    True, or the A/B values "2" (the separators' chain on the side stream only) and "3" (the products' early start only)."""
    monkeypatch.setenv("ESL_CF_OVERLAP", overlap if isinstance(overlap, str) else ("1" if overlap else "0"))
    try:
        return pkg.Context(0)
    finally:
        monkeypatch.delenv("ESL_CF_OVERLAP", raising=False)


def _two_runs(pkg, cx, g, c, o):
    """Two consecutive optimize calls of ITERS LM iterations on the resident graph; everything the comparison looks at."""
    p = pkg.default_lm_params(jacobian_mode=1, linear_solver=2, max_iters=ITERS)
    cx.upload_graph(g); cx.upload_states(c, o)
    out = []
    for _ in range(2):
        rep = cx.optimize_resident(p)
        assert cx.lm_solver_used() == 2
        cams, objs = cx.download_states()
        xc, xo = cx.lm_download(5, 6 * (g.n_cams - 1)), cx.lm_download(2, 9 * g.n_objs)
        out.append(dict(cams=cams, objs=objs, xc=xc, xo=xo, chi2=rep["trace_chi2"], lam=rep["trace_lambda"], trials=rep["trace_trials"]))
    return out, cx.lm_solver_stats()


def _compare(pkg, monkeypatch, g, c, o, x_form, min_segments, on=True):
    monkeypatch.setenv("ESL_CF_SPARSE", "1")
    res = {}
    cxs = {bool(ov): _context(pkg, monkeypatch, ov) for ov in (False, on)}   # both alive in one process
    try:
        for ov, cx in cxs.items():
            res[ov] = _two_runs(pkg, cx, g, c, o)
    finally:
        for cx in cxs.values():
            cx.close()
    (serial, st0), (side, st1) = res[False], res[True]
    assert st0 == st1 and st1["x_form"] == x_form and st1["segments"] >= min_segments, st1
    for call, (a, b) in enumerate(zip(serial, side)):
        assert np.isfinite(b["cams"]).all() and np.isfinite(b["objs"]).all()
        assert list(a["trials"]) == list(b["trials"]), call
        for key in ("cams", "objs", "xc", "xo", "chi2", "lam"):
            assert _same_bits(a[key], b[key]), (call, key)
    assert len(side[1]["trials"]) > 0   # (the second call ran trials of its own)
    return st1


def _awkward_graph(pkg):
    """The structures of test_sparse_interior_rows_on_awkward_structures: an ellipsoid seen only by separator cameras, one seen only
    by the fixed camera, one inside a single segment, a segment without an interior observation, a short last segment."""
    g0, c, o, _ = pkg.synth.make_graph(330, 14, 3300, seed=43, slam=True)

    def keep(cam, obj):
        k = np.ones(len(cam), bool)
        k &= ~((obj == 0) & ~((cam % 16 == 0) & (cam > 0)))
        k &= ~((obj == 1) & (cam != 0))
        k &= ~((obj == 2) & ~((cam >= 17) & (cam <= 30)))
        k &= ~((cam >= 81) & (cam <= 95))
        return k
    kb, k3 = keep(g0.bbox_cam, g0.bbox_obj), keep(g0.e3d_cam, g0.e3d_obj)
    extra_cam = np.array([16, 32, 48, 0, 0, 20, 25], np.int32); extra_obj = np.array([0, 0, 0, 1, 1, 2, 2], np.int32)
    bb, _, _ = pkg.synth.project_bboxes(c, o, g0.K, extra_cam, extra_obj)
    okb = np.isfinite(bb).all(1)
    g = pkg.Graph(g0.K, g0.n_cams, g0.n_objs, g0.cam_fixed,
                  np.concatenate([g0.bbox_cam[kb], extra_cam[okb]]), np.concatenate([g0.bbox_obj[kb], extra_obj[okb]]),
                  np.concatenate([g0.bbox_meas.reshape(-1, 4)[kb], bb[okb]]), np.concatenate([g0.bbox_weight[kb], np.full(okb.sum(), 0.7)]),
                  g0.e3d_cam[k3], g0.e3d_obj[k3], g0.e3d_meas.reshape(-1, 10)[k3], g0.e3d_weight[k3],
                  g0.grav_obj, g0.grav_normal, g0.grav_weight, g0.odom_i, g0.odom_j, g0.odom_meas, g0.odom_info)
    cams_of = lambda ob: set(np.concatenate([g.bbox_cam[g.bbox_obj == ob], g.e3d_cam[g.e3d_obj == ob]]).tolist())
    assert cams_of(0) and all(cm % 16 == 0 and cm > 0 for cm in cams_of(0)) and cams_of(1) == {0} and cams_of(2) <= set(range(17, 31))
    assert not (set(range(81, 96)) & set(np.concatenate([g.bbox_cam, g.e3d_cam]).tolist()))
    return g, c, o


@pytest.mark.parametrize("n_cams,n_objs,per_cam", [(257, 40, 6), (300, 80, 10), (500, 50, 10)])
def test_side_order_equals_serial_order_bit_for_bit(pkg, monkeypatch, n_cams, n_objs, per_cam):
    """Sparse stored-products form: 256 free cameras (16 separators, the last camera IS one: the shortest separator chain the form
    has), 299 (short last segment), 499."""
    g, c, o, _ = pkg.synth.make_graph(n_cams, n_objs, per_cam * n_cams, seed=41, slam=True)
    st = _compare(pkg, monkeypatch, g, c, o, x_form=1, min_segments=16)
    assert st["separators"] == (n_cams - 1) // 16


@pytest.mark.parametrize("half", ["2", "3"])
def test_each_half_alone_equals_serial_order(pkg, monkeypatch, half):
    """The switch's A/B values: the separators' chain on the side stream alone, the products' early start alone."""
    g, c, o, _ = pkg.synth.make_graph(300, 80, 3000, seed=41, slam=True)
    _compare(pkg, monkeypatch, g, c, o, x_form=1, min_segments=16, on=half)


def test_side_order_on_awkward_structures(pkg, monkeypatch):
    g, c, o = _awkward_graph(pkg)
    st = _compare(pkg, monkeypatch, g, c, o, x_form=1, min_segments=4)
    assert st["separators"] == (g.n_cams - 1) // 16 and st["segments"] == (g.n_cams - 1 + 15) // 16


def test_dissected_dense_form_is_untouched_by_the_switch(pkg, monkeypatch):
    """About 100 cameras and 8 ellipsoids: dissected (stride 16, 7 segments) but below the sparse form's 256 free cameras, so X
    stays dense and the switch must change nothing."""
    g, c, o, _ = pkg.synth.make_graph(100, 8, 800, seed=47, slam=True)
    st = _compare(pkg, monkeypatch, g, c, o, x_form=0, min_segments=4)
    assert st["stride"] == 16


def test_plain_chain_is_untouched_by_the_switch(pkg, monkeypatch):
    """30 cameras: no dissection at all (the plain chain), with the switch on and off."""
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=53, slam=True)
    st = _compare(pkg, monkeypatch, g, c, o, x_form=0, min_segments=1)
    assert st["stride"] == 0 and st["separators"] == 0


def test_trim_between_optimize_calls(pkg, monkeypatch):
    """esl_ctx_trim frees what the side stream reads (slabs, products, the separators' blocks): the next optimize rebuilds the
    layout and gives the bits of a run that never trimmed."""
    g, c, o, _ = pkg.synth.make_graph(300, 80, 3000, seed=41, slam=True)
    monkeypatch.setenv("ESL_CF_SPARSE", "1")
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
            assert cx.lm_solver_stats()["x_form"] == 1
            out[trim] = (cx.download_states(), rep)
        finally:
            cx.close()
    (s0, r0), (s1, r1) = out[False], out[True]
    assert list(r0["trace_trials"]) == list(r1["trace_trials"]) and _same_bits(r0["trace_chi2"], r1["trace_chi2"])
    assert _same_bits(s0[0], s1[0]) and _same_bits(s0[1], s1[1])


def test_destroy_straight_after_optimize_resident(pkg, monkeypatch):
    """Destroying the context as soon as optimize_resident has returned: the side stream and its events go away with it, and the
    device is fit for the next context."""
    g, c, o, _ = pkg.synth.make_graph(300, 80, 3000, seed=41, slam=True)
    monkeypatch.setenv("ESL_CF_SPARSE", "1")
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
