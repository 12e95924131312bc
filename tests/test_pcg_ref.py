"""ESL_SOLVER_PCG without a GPU: the numpy reference (tests/pcg_ref.py) against numpy.linalg.solve on the C oracle's system, and the
public surface of the feature (constant, header, exported symbols, struct size)."""
import ctypes
import os

import numpy as np

from tests import pcg_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_pcg_variants_agree_and_solve_the_reduced_system(pkg, po):
    g, c, o, _ = pkg.synth.make_graph(30, 6, 200, seed=3, slam=True)
    H, b, fidx, _ = po.build_system(g, c, o, delta=1e-6)
    n = 6 * int((~g.cam_fixed.astype(bool)).sum())
    lam = 1e-5 * np.abs(np.diag(H)).max()
    Hcc, W, D, bc, bo = pr.split_system(H, b, n, lam)
    Hll = H[n:, n:] + lam * np.eye(len(b) - n)
    assert np.array_equal(Hll, np.kron(np.eye(len(D)), np.ones((9, 9))) * Hll)   # the ellipsoid block IS block diagonal
    S, bs = pr.schur_dense(Hcc, W, D, bc, bo)
    # numpy.linalg.solve on the float64 Schur complement numpy itself forms
    Hpp, Hpl = H[:n, :n] + lam * np.eye(n), H[:n, n:]
    S64 = Hpp - Hpl @ np.linalg.solve(Hll, Hpl.T)
    ref = np.linalg.solve(S64, b[:n] - Hpl @ np.linalg.solve(Hll, b[n:]))
    np.testing.assert_allclose(np.array(S, dtype=np.float64), S64, rtol=0, atol=1e-13 * np.abs(S64).max())
    xd, kd, rd, okd = pr.pcg_dense(S, bs, rel_tol=1e-12)
    xm, km, rm, okm, bs_m, blocks = pr.pcg_matrix_free(Hcc, W, D, bc, bo, rel_tol=1e-12)
    print("reference PCG, 29 free cameras: dense %d iterations (|r|/|b| %.2e), matrix-free %d (%.2e); max error vs solve %.2e / %.2e of max|x| %.2e"
          % (kd, rd, km, rm, np.abs(xd - ref).max(), np.abs(xm - ref).max(), np.abs(ref).max()))
    assert okd and okm and kd <= 60 and km <= 60
    assert rd <= 1e-12 and rm <= 1e-12
    np.testing.assert_allclose(np.array(bs_m - bs, dtype=np.float64), 0, atol=1e-15 * float(np.abs(bs).max()))
    np.testing.assert_allclose(np.array(blocks - pr.diag_blocks(S), dtype=np.float64), 0, atol=1e-15 * float(np.abs(S).max()))
    assert np.abs(xd - xm).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(xd - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.abs(xm - ref).max() <= 1e-9 * np.abs(ref).max()
    # the stopping rule's corner cases: a zero right-hand side, and a cap that is reached
    x0, k0, r0, ok0 = pr.pcg_dense(S, np.zeros(n))
    assert ok0 and k0 == 0 and r0 == 0 and not x0.any()
    x3, k3, r3, ok3 = pr.pcg_dense(S, bs, rel_tol=1e-12, max_iters=3)
    assert not ok3 and k3 == 3 and r3 > 1e-12


def test_pcg_bindings_and_header(pkg):
    assert pkg.abi.SOLVER_PCG == 4
    txt = open(os.path.join(ROOT, "include", "esl.h")).read()
    for s in ("ESL_SOLVER_PCG = 4", "esl_lm_set_pcg", "esl_lm_pcg_stats", "esl_pcg_params_default", "#define ESL_PCG_STATS 8"):
        assert s in txt, s
    L = pkg.lib.load()
    for s in ("esl_lm_set_pcg", "esl_lm_pcg_stats", "esl_pcg_params_default"):
        assert hasattr(L, s) and s in pkg.lib.EXPORTS
    assert ctypes.sizeof(pkg.abi.EslPcgParams) == 16
    assert L.esl_abi_version() == 5
    p = pkg.abi.EslPcgParams()
    L.esl_pcg_params_default(ctypes.byref(p))
    assert (p.max_iters, p.check_every, p.rel_tol) == (1000, 8, 1e-10)
    d = pkg.abi.default_pcg_params()
    assert (d.max_iters, d.check_every, d.rel_tol) == (1000, 8, 1e-10)
    assert hasattr(pkg.Context, "set_pcg") and hasattr(pkg.Context, "lm_pcg_stats")
