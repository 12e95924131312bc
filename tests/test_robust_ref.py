"""Robust kernels (esl_lm_set_robust / esl_edge_chi2): the numpy reference against g2o's closed forms and against the plain
oracle, and the C-ABI surface as the header and the Python layer declare it.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import robust_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("delta", [0.5, 1.0, 3.0])
def test_robustify_matches_g2o_closed_forms(delta):
    d2 = delta * delta
    eps = 1e-9 * d2
    for e in (0.0, d2 - eps, d2, d2 + eps, 4 * d2, 100 * d2):
        assert rr.robustify("none", delta, e) == (e, 1.0)
        r0, r1 = rr.robustify("huber", delta, e)
        if e <= d2:
            assert (r0, r1) == (e, 1.0)
        else:
            assert r0 == pytest.approx(2 * delta * np.sqrt(e) - d2, rel=1e-15) and r1 == pytest.approx(delta / np.sqrt(e), rel=1e-15)
        r0, r1 = rr.robustify("pseudo_huber", delta, e)
        assert r0 == pytest.approx(2 * d2 * (np.sqrt(1 + e / d2) - 1), rel=1e-12, abs=1e-300)
        assert r1 == pytest.approx(1 / np.sqrt(1 + e / d2), rel=1e-15)
        r0, r1 = rr.robustify("cauchy", delta, e)
        assert r0 == pytest.approx(d2 * np.log1p(e / d2), rel=1e-12, abs=1e-300) and r1 == pytest.approx(1 / (1 + e / d2), rel=1e-15)
        r0, r1 = rr.robustify("tukey", delta, e)
        if e <= d2:
            assert r0 == pytest.approx(d2 * (1 - (1 - e / d2) ** 3), rel=1e-12, abs=1e-300)
            assert r1 == pytest.approx(3 * (1 - e / d2) ** 2, rel=1e-9, abs=1e-12)
        else:
            assert (r0, r1) == (d2, 0.0)   # Tukey's outliers carry no weight
    # derivative check: rho1 = d rho0 / de away from the branch points
    for kind in ("huber", "pseudo_huber", "cauchy", "tukey"):
        for e in (0.3 * d2, 2.5 * d2):
            if kind == "tukey" and e > d2:
                continue
            h = 1e-6 * d2
            num = (rr.robustify(kind, delta, e + h)[0] - rr.robustify(kind, delta, e - h)[0]) / (2 * h)
            assert rr.robustify(kind, delta, e)[1] == pytest.approx(num, rel=1e-6)


@pytest.mark.parametrize("slam", [False, True])
def test_robust_reference_without_kernels_is_the_plain_oracle(pkg, slam):
    from oracle import np_oracle as npo
    g, c, o, _ = pkg.synth.make_graph(8, 3, 40, seed=2, slam=slam)
    ca, oa, ra = npo.optimize(g, c, o, delta=1e-6)
    cb, ob, rb = rr.optimize(g, c, o, robust={}, delta=1e-6)
    assert ra["trace"] == rb["trace"]
    assert np.array_equal(ca, cb) and np.array_equal(oa, ob)


def test_robust_reference_downweights_outliers(pkg):
    g, c, o, _ = pkg.synth.make_graph(8, 3, 40, seed=2)
    e, w = rr.edge_chi2(g, c, o, "bbox", robust={"bbox": ("huber", 1.0)})
    assert len(e) == len(g.bbox_cam)
    assert np.all((w == 1.0) == (e <= 1.0))
    np.testing.assert_allclose(w[e > 1.0], 1.0 / np.sqrt(e[e > 1.0]))


def test_robust_abi_is_declared_and_exported(pkg):
    """esl_robust_params is 48 bytes and the two entry points are in the header and the Python layer's export list (ABI 5 additive)."""
    assert C.sizeof(pkg.abi.EslRobustParams) == 48
    hdr = open(os.path.join(ROOT, "include", "esl.h")).read()
    for name in ("esl_lm_set_robust", "esl_edge_chi2"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in pkg.lib.EXPORTS
    assert re.search(r"#define ESL_ABI_VERSION 5\b", hdr)
    p = pkg.default_robust_params(bbox=("huber", 2.0), odom=("tukey", 3.0))
    assert list(p.kind) == [1, 0, 0, 4] and list(p.delta) == [2.0, 1.0, 1.0, 3.0]
    with pytest.raises(ValueError):
        pkg.default_robust_params(bbox=("saturated", 1.0))
