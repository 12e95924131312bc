"""Camera-first elimination, form 3 with camera segments of two and three chunks (esl_cf_plan.hpp, "choosing the segment length"): every
32nd or 48th free camera is a separator instead of every 16th.  Another, equally exact elimination order of the same linear system:
a forced stride is held against the dense X (ESL_CF_SPARSE=0) and the reduced camera system with the bounds
tests/test_gpu_cf_onesided.py holds the stride-16 form to, and against itself bit for bit where only the stream order or the layout's
lifetime changes; stride 16 forced is the library's unset path, bit for bit.  The rule that chooses the stride of a large graph is a
host function and is checked on a table of counts without a GPU.
"""
import numpy as np
import pytest

from tests import cf_plan_ref
from tests.test_gpu_cf_onesided import _assert_same_runs, _first_trial_and_run, _graph, _hold_against, _refs
from tests.test_gpu_cf_sep_overlap import ITERS, _same_bits, _two_runs

gpu = pytest.mark.gpu


def _context(pkg, monkeypatch, stride, overlap=True):
    """A context whose ESL_CF_STRIDE and ESL_CF_OVERLAP were these when it was created (both are read there and kept)."""
    if stride is None:
        monkeypatch.delenv("ESL_CF_STRIDE", raising=False)
    else:
        monkeypatch.setenv("ESL_CF_STRIDE", str(stride))
    if overlap is None:
        monkeypatch.delenv("ESL_CF_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("ESL_CF_OVERLAP", "1" if overlap else "0")
    try:
        return pkg.Context(0)
    finally:
        monkeypatch.delenv("ESL_CF_STRIDE", raising=False)
        monkeypatch.delenv("ESL_CF_OVERLAP", raising=False)


def _forced(pkg, monkeypatch, g, c, o, stride):
    monkeypatch.setenv("ESL_CF_STRIDE", str(stride))
    try:
        return _first_trial_and_run(pkg, monkeypatch, g, c, o, "3", 2)
    finally:
        monkeypatch.delenv("ESL_CF_STRIDE", raising=False)


def _assert_layout(st, n_free, stride):
    assert st["x_form"] == 3 and st["stride"] == stride, st
    assert st["separators"] == n_free // stride and st["segments"] == -(-n_free // stride), st
    assert st["product_flops"] > 0 and st["product_bytes"] > 0


@gpu
@pytest.mark.parametrize("n_cams,n_objs,per_cam,stride", [(257, 40, 6, 32), (257, 40, 6, 48), (300, 80, 10, 32), (300, 80, 10, 48),
                                                          (2150, 30, 4, 32)])
def test_forced_stride_equals_dense_rows_and_camera_system(pkg, monkeypatch, n_cams, n_objs, per_cam, stride):
    """256 free cameras: the last one is a separator at stride 32 (and the last segment at 48 is 16 slots: one whole chunk); 299: a
    short last segment (11 slots at stride 32 and 48: less than the first chunk of the segment); 2,149 free cameras at stride 32 = 68
    segments: the segment bitmaps need a second 64-bit word (the smallest size at which the word loop runs twice)."""
    g, c, o = _graph(n_cams, n_objs, per_cam)
    ref = _refs(pkg, monkeypatch, (n_cams, n_objs, per_cam), g, c, o)
    new = _forced(pkg, monkeypatch, g, c, o, stride)
    _assert_layout(new["st"], n_cams - 1, stride)
    assert "sparse_block_products" in new["classes"]
    if n_cams == 2150:
        assert new["st"]["segments"] == 68
    for tag in ("dense", "camera"):
        _hold_against("%s, stride %d" % (tag, stride), new, ref[tag], x_tol=1e-10, chi_tol=1e-12, trace_tol=1e-11, state_tol=1e-9, res_tol=1e-13)


def _awkward_graph32(pkg):
    """The structures of tests/test_gpu_cf_sep_overlap.py's _awkward_graph at the slots of stride 32 (free camera k has slot k - 1:
    segment p = cameras 32 p + 1 .. 32 p + 32, the last one its separator): ellipsoid 0 seen only by separator cameras, 1 only by the
    fixed camera, 2 only inside segment 1, 3 only by interior cameras of the SECOND chunk of segment 2 (cameras 81 .. 95: its column of
    the slab is zero over the first chunk and the forward sweep carries it across the chunk boundary), segment 4 (cameras 129 .. 159)
    without an interior observation, a short last segment (329 free cameras)."""
    g0, c, o, _ = pkg.synth.make_graph(330, 14, 3300, seed=43, slam=True)

    def keep(cam, obj):
        k = np.ones(len(cam), bool)
        k &= ~((obj == 0) & ~((cam % 32 == 0) & (cam > 0)))
        k &= ~((obj == 1) & (cam != 0))
        k &= ~((obj == 2) & ~((cam >= 33) & (cam <= 62)))
        k &= ~((obj == 3) & ~((cam >= 81) & (cam <= 95)))
        k &= ~((cam >= 129) & (cam <= 159))
        return k
    kb, k3 = keep(g0.bbox_cam, g0.bbox_obj), keep(g0.e3d_cam, g0.e3d_obj)
    extra_cam = np.array([32, 64, 96, 0, 0, 40, 50, 85, 90], np.int32); extra_obj = np.array([0, 0, 0, 1, 1, 2, 2, 3, 3], np.int32)
    bb, _, _ = pkg.synth.project_bboxes(c, o, g0.K, extra_cam, extra_obj)
    okb = np.isfinite(bb).all(1)
    g = pkg.Graph(g0.K, g0.n_cams, g0.n_objs, g0.cam_fixed,
                  np.concatenate([g0.bbox_cam[kb], extra_cam[okb]]), np.concatenate([g0.bbox_obj[kb], extra_obj[okb]]),
                  np.concatenate([g0.bbox_meas.reshape(-1, 4)[kb], bb[okb]]), np.concatenate([g0.bbox_weight[kb], np.full(okb.sum(), 0.7)]),
                  g0.e3d_cam[k3], g0.e3d_obj[k3], g0.e3d_meas.reshape(-1, 10)[k3], g0.e3d_weight[k3],
                  g0.grav_obj, g0.grav_normal, g0.grav_weight, g0.odom_i, g0.odom_j, g0.odom_meas, g0.odom_info)
    cams_of = lambda ob: set(np.concatenate([g.bbox_cam[g.bbox_obj == ob], g.e3d_cam[g.e3d_obj == ob]]).tolist())
    assert cams_of(0) and all(cm % 32 == 0 and cm > 0 for cm in cams_of(0)) and cams_of(1) == {0}
    assert cams_of(2) and cams_of(2) <= set(range(33, 63)) and cams_of(3) and cams_of(3) <= set(range(81, 96))
    assert not (set(range(129, 160)) & set(np.concatenate([g.bbox_cam, g.e3d_cam]).tolist()))
    return g, c, o


@gpu
def test_stride_32_on_awkward_structures(pkg, monkeypatch):
    g, c, o = _awkward_graph32(pkg)
    new = _forced(pkg, monkeypatch, g, c, o, 32)
    ref = _first_trial_and_run(pkg, monkeypatch, g, c, o, "0", 2)
    assert ref["st"]["x_form"] == 0
    _assert_layout(new["st"], g.n_cams - 1, 32)
    _hold_against("dense (awkward structures, stride 32)", new, ref, x_tol=1e-9, chi_tol=1e-11, trace_tol=1e-10, state_tol=1e-8)


@gpu
def test_stride_16_forced_is_the_unset_path_bit_for_bit(pkg, monkeypatch):
    g, c, o = _graph(300, 80, 10)
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    runs = []
    for stride in (None, 16):
        cx = _context(pkg, monkeypatch, stride, overlap=None)
        try:
            res, st = _two_runs(pkg, cx, g, c, o)
            _assert_layout(st, 299, 16)
            runs.append(res)
        finally:
            cx.close()
    _assert_same_runs(runs[0], runs[1])
    assert len(runs[1][1]["trials"]) > 0


@gpu
def test_default_selection_keeps_stride_16_on_a_small_system(pkg, monkeypatch):
    """228 ellipsoids = 2,052 unknowns: the library keeps X sparse of its own accord and assembles T one-sided, and far below the
    8,192 unknowns from which the separators' update carries the build the stride stays 16."""
    g, c, o = _graph(257, 228, 4)
    monkeypatch.delenv("ESL_CF_SPARSE", raising=False)
    cx = _context(pkg, monkeypatch, None, overlap=None)
    try:
        cx.upload_graph(g); cx.upload_states(c, o)
        rep = cx.optimize_resident(pkg.default_lm_params(jacobian_mode=1, linear_solver=2, max_iters=1))
        assert cx.lm_solver_used() == 2
        _assert_layout(cx.lm_solver_stats(), 256, 16)
        assert np.isfinite(rep["chi2_final"]) and rep["chi2_final"] < rep["chi2_initial"]
    finally:
        cx.close()


@gpu
def test_stride_32_same_bits_serial_order_and_side_order(pkg, monkeypatch):
    g, c, o = _graph(300, 80, 10)
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    runs = []
    for overlap in (False, None):
        cx = _context(pkg, monkeypatch, 32, overlap=overlap)
        try:
            res, st = _two_runs(pkg, cx, g, c, o)
            _assert_layout(st, 299, 32)
            runs.append(res)
        finally:
            cx.close()
    _assert_same_runs(runs[0], runs[1])
    assert len(runs[1][1]["trials"]) > 0


@gpu
def test_stride_32_trim_between_optimize_calls(pkg, monkeypatch):
    """esl_ctx_trim frees the layout; the next optimize rebuilds it at the context's stride and gives the bits of a run that never
    trimmed."""
    g, c, o = _graph(300, 80, 10)
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    p = pkg.default_lm_params(jacobian_mode=1, linear_solver=2, max_iters=ITERS)
    out = {}
    for trim in (False, True):
        cx = _context(pkg, monkeypatch, 32, overlap=None)
        try:
            cx.upload_graph(g); cx.upload_states(c, o)
            cx.optimize_resident(p)
            if trim:
                cx.trim()
            rep = cx.optimize_resident(p)
            _assert_layout(cx.lm_solver_stats(), 299, 32)
            out[trim] = (cx.download_states(), rep)
        finally:
            cx.close()
    (s0, r0), (s1, r1) = out[False], out[True]
    assert list(r0["trace_trials"]) == list(r1["trace_trials"]) and _same_bits(r0["trace_chi2"], r1["trace_chi2"])
    assert _same_bits(s0[0], s1[0]) and _same_bits(s0[1], s1[1])


@gpu
def test_the_plan_the_device_ran_is_the_host_plan(pkg, monkeypatch, tmp_path):
    """The layout the library ships is cf_plan_build's (csrc/esl_cf_plan.hpp), which tests/test_cf_plan.py pins on the CPU: after one trial
    all ten numbers of esl_lm_solver_stats equal what tests/cf_plan_main.cpp, compiled here, prints for the same lists and switches -- the
    flops as exact doubles.  256 free cameras, 40 ellipsoids: X dense with nothing set (9 N < 2,048), forms 1 and 2, form 3 at strides 32
    and 48 (a short last segment).  (The device's memory size only decides between forms 1 and 2, at gigabytes: this graph's need is a
    few megabytes, so the program's default stands for it.)"""
    g, c, o = _graph(257, 40, 6)
    exe = cf_plan_ref.build(tmp_path)
    assert exe, "no host compiler"
    L = cf_plan_ref.lists(g)
    for sparse, stride, form in ((None, None, 0), ("1", None, 1), ("2", None, 2), ("3", 32, 3), ("3", 48, 3)):
        if sparse is None:
            monkeypatch.delenv("ESL_CF_SPARSE", raising=False)
        else:
            monkeypatch.setenv("ESL_CF_SPARSE", sparse)
        cx = _context(pkg, monkeypatch, stride, overlap=None)
        try:
            cx.upload_graph(g); cx.upload_states(c, o)
            cx.lm_begin(pkg.default_lm_params(jacobian_mode=1, linear_solver=2))
            tr = cx.lm_try_step(1e-5 * cx.lm_linearize().max_diag)
            assert tr.solve_ok == 1 and cx.lm_solver_used() == 2
            st = list(cx.lm_solver_stats().values())
        finally:
            cx.close()
            monkeypatch.delenv("ESL_CF_SPARSE", raising=False)
        want = cf_plan_ref.solver_stats(cf_plan_ref.run(exe, L, tmp_path, sparse=-1 if sparse is None else int(sparse), stride=stride or 0))
        print("ESL_CF_SPARSE", sparse, "ESL_CF_STRIDE", stride, "stats", st)
        assert st[0] == form and st == [float(x) for x in want], (st, want)


# ---- the rule that chooses the stride (esl_cf_plan.hpp, cf_stride_choose): a host function, no GPU ----------------------------------------
# ms per trial = update flops / (0.83 x 79 TFLOP/s) + entry-products x 0.078 ms per million + slab elements x 1.30 ms / 1.35e8; a wider
# stride is taken when it is under 0.95 of the stride-16 figure, the cheapest of them; 16 below 8,192 unknowns.
_UPD, _PAIR, _SLAB = 0.83 * 79.0e9, (7.82 - 4.21) / (77.35e6 - 31.05e6), 1.30 / 1.35e8
# the counts of 10k cameras / 2k ellipsoids at stride 16 / 32 / 48 (esl_lm_solver_stats and scripts/cf_onesided_counts.py)
_C4 = ((1.0639e12, 5.3434e11, 3.5813e11), (31.05e6, 57.57e6, 77.35e6), (1.352e8, 2.510e8, 3.377e8))
_RULE_TABLE = [
    # (n_o, update flops, entry-products, slab elements, stride, why)
    (18000,) + _C4 + (48, "19.9 / 15.1 / 14.7 ms: the update's 10.8 ms outweigh 3.6 ms of products and 2 ms of slabs"),
    (8192,) + _C4 + (48, "the first order at which the rule looks at the counts"),
    (8191,) + _C4 + (16, "below it: 16 whatever the counts say"),
    (18000, _C4[0], (100e6, 400e6, 900e6), _C4[2], 16, "every camera sees every ellipsoid: the products grow with the square of the segment"),
    (18000, (3.2785e11, 2.95e11, 2.9e11), (32.06e6, 33.3e6, 60e6), (2.6e8, 2.7e8, 4e8), 16, "10.0 against 9.7 ms: inside the 5 % margin"),
    (18000, (8e11, 4e11, 3.9e11), (30e6, 50e6, 90e6), (1.3e8, 2.4e8, 3.3e8), 32, "the staircase gives nothing beyond 32: 15.8 / 12.3 / 16.1 ms"),
]


@pytest.mark.parametrize("n_o,upd,pairs,slab,stride,why", _RULE_TABLE)
def test_stride_rule_on_a_table_of_counts(pkg, n_o, upd, pairs, slab, stride, why):
    got, ms = pkg.lib.cf_stride_choose(n_o, upd, pairs, slab)
    want_ms = [u / _UPD + p * _PAIR + s * _SLAB for u, p, s in zip(upd, pairs, slab)]
    print(why, ["%.2f" % v for v in want_ms])
    assert ms == pytest.approx(want_ms, rel=1e-12)
    assert got == stride, why
