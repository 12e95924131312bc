"""The device's linearisation with analytic Jacobians (esl_lm_linearize, jacobian_mode = 1: the mode the bench and nearly every solver
test run) against the forward-mode multiprecision reference of tests/lin_ref.py, on the built scenes of lin_ref.SCENES (their premises:
tests/test_lin_ref.py), in SLAM mode and in mapping mode (every camera fixed), and with the tangency residual on two of them.  Every
block esl_lm_download exposes (H_oo, b_o, H_cc, b_c, the per-edge W), chi2, max_diag and the per-edge chi2 of esl_edge_chi2 are compared;
the counts of esl_lm_begin exactly; W of a dropped box and of a fixed camera's edge must be exactly zero.

Tolerances (the rule of tests/test_gpu_slam_step.py).  The device's error against mpmath at 40 digits (max-norm of the difference over the
quantity's max-norm; H_oo, H_cc, W per block, the worst kept) may be at most MARGIN x yardstick + 4 eps, the yardstick being the error of
the float64 forward-mode evaluation of the same quantity of the same scene -- never the device's output, never a host build of
esl_math.hpp.  One margin per group (lin_ref.MARGIN), the next power of two at or above 4 x the worst ratio (device error / yardstick,
an error within 4 eps counting as 0) measured on the MI355X over this module:

    Jacobian blocks (H_oo, H_cc, W)        worst 1.20  (long_camera, SLAM mode, W)                              -> MARGIN jac    = 8
    gradients (b_o, b_c)                   worst 2.22  (long_ellipsoid, SLAM mode, tangency residual, b_o)      -> MARGIN grad   = 16
    scalars (chi2, edge chi2, max_diag)    worst 8.81  (long_ellipsoid, SLAM mode, tangency residual, chi2:
                                                       1.15e-15 against a yardstick of 1.30e-16, below one eps) -> MARGIN scalar = 64

Per scene (Jacobian blocks / gradients / scalars): minimal 1.01 / 1.05 / 7.87, long_ellipsoid 1.00 / 2.22 / 8.81, long_camera 1.20 / 0.79 /
2.06, branches 1.01 / 0.54 / 2.81, dropped 1.00 / 1.05 / 2.49.  Most blocks sit at a ratio of 1.00: their error is the conditioning of the
quantity on the float64 inputs, which the device and the yardstick share.  No finding: nothing the device computes is further from the
reference than plain float64 arithmetic explains.
A ratio above 64 would not be a margin to adopt but a finding in the kernels.  Every ratio is printed by every run (-s),
the worst ones when the module ends.
"""
import numpy as np
import pytest

from tests import lin_ref as lr

pytestmark = pytest.mark.gpu

WORST = {}                  # group -> (ratio, where)
CONFIGS = [(name, slam, mode) for name in lr.SCENES for slam in (True, False) for mode in ((0, 1) if name in lr.TANGENCY_SCENES else (0,))]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst ratios device error / float64 yardstick over the module: " +
          ", ".join("%s %.2f (%s)" % (k, v[0], v[1]) for k, v in sorted(WORST.items())))


class Dev:
    """what the device leaves of one linearisation, in lin_ref.Lin's fields"""


def linearise(pkg, ctx, g, c, o, slam, mode):
    gg = g if slam else lr.mapping_graph(g)
    nf = int((~g.cam_fixed.astype(bool)).sum()) if slam else 0
    N, ne = g.n_objs, len(g.bbox_cam) + len(g.e3d_cam)
    ctx.upload_graph(gg); ctx.upload_states(c, o)
    d = Dev()
    d.n_valid, d.n_dropped = ctx.lm_begin(pkg.default_lm_params(jacobian_mode=1, e3d_half_turn=1, bbox_residual=mode))
    part = ctx.lm_linearize()
    d.chi2, d.max_diag = part.chi2, part.max_diag
    d.Hoo, d.bo = ctx.lm_download(0, N * 45).reshape(N, 45), ctx.lm_download(1, N * 9).reshape(N, 9)
    d.Hcc = d.bc = d.W = None
    if nf:
        d.Hcc, d.bc = ctx.lm_download(3, nf * 36).reshape(nf, 6, 6), ctx.lm_download(4, nf * 6).reshape(nf, 6)
        d.W = ctx.lm_download(9, ne * 54).reshape(54, ne).T.reshape(ne, 6, 9)
    d.edge_chi2, d.edge_w = {}, {}
    for cls in ("bbox", "e3d", "grav") + (("odom",) if slam else ()):
        d.edge_chi2[cls], d.edge_w[cls] = ctx.edge_chi2(cls)
    return d


@pytest.mark.parametrize("name,slam,mode", CONFIGS, ids=["%s-%s%s" % (n, "slam" if s else "mapping", "-tangency" if m else "") for n, s, m in CONFIGS])
def test_linearisation_matches_forward_mode_reference(pkg, ctx, name, slam, mode):
    g, c, o = lr.scene(name)
    ref, y = lr.lin_of(name, lr.MP(40), mode, slam), lr.yardsticks(name, mode, slam)
    assert max(y.values()) <= lr.YARDSTICK_MAX, y          # a yardstick beyond it would only widen what the device is allowed
    d = linearise(pkg, ctx, g, c, o, slam, mode)
    assert (d.n_valid, d.n_dropped) == (ref.n_valid, ref.n_dropped)
    err = lr.errors(lr.MP(40), d, ref)
    assert set(err) == set(y)
    where = "%s %s%s" % (name, "SLAM" if slam else "mapping", " tangency" if mode else "")
    bad = []
    for q in sorted(err):
        grp = lr.GROUP[q]
        r = lr.ratio(err[q], y[q])
        print("%s: %s error %.2e (yardstick %.2e, ratio %.2f)" % (where, q, err[q], y[q], r))
        if r > WORST.get(grp, (-1.0, ""))[0]:
            WORST[grp] = (r, "%s %s" % (where, q))
        if not err[q] <= lr.allow(grp, y[q]):
            bad.append((q, err[q], y[q]))
    assert not bad, (where, bad)
    # exact zeros: W of a dropped box and of a fixed camera's edge; a dropped box reports weight 0, every other edge weight 1
    if d.W is not None:
        for u in range(len(d.W)):
            if not np.asarray(ref.W[u], dtype=bool).any():
                assert not d.W[u].any(), (where, u)
    for cls, v in ref.edge_chi2.items():
        if cls in d.edge_w and len(v):
            assert d.edge_w[cls].tolist() == [0.0 if x is None else 1.0 for x in v], (where, cls)
