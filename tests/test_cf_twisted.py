"""The two-directional ("twisted") solve of a camera segment (tests/cf_twisted_ref.py: the numpy statement of csrc/esl_cf_sweep.hpp)
against a dense solve of G_p in extended precision (tests/slam_step_ref.py solve_ref: numpy.linalg.solve refined on longdouble
residuals), on segments of 15, 31 and 47 slots (strides 16, 32, 48) and on a short last segment, for every kind of column the sweep
treats differently.  No GPU.

The bound.  Y = L^T G_p^-1 w is the solution of a linear system with G_p; a solve that is as good as fp64 allows leaves a relative
error of a few cond(G_p) eps, the figure in which this repository's CPU tests state what another association of an fp64 computation
may move (FLOOR = 4 eps for a single rounded quantity, tests/lin_ref.py; here carried through the solve by its condition):

    max |Y - Y_ref| <= 4 cond(G_p) eps max |Y_ref|,        cond(G_p) computed here from the segment's own matrix.

Both routes -- the sweep and the parent's substitution (k_cf_forward<2> + k_cf_seg_back) -- are held to it, so the sweep is never
accepted for being under a fixed number.  Measured (seed 0): cond 1.8e2 .. 2.4e2, the sweep at most 0.012 of the bound (2.0e-15), the
substitution the same size; the figures are printed by every run (-s).

The premises of tests/test_gpu_cf_twisted.py are asserted here from its graphs alone: each contains the column kinds below.
"""
import functools
import importlib

import numpy as np
import pytest

from tests import cf_plan_ref as ref
from tests import cf_twisted_ref as tw
from tests import slam_step_ref as sr

EPS = sr.EPS64
KINDS = ["head at the first slot", "head at the last interior slot", "head in the middle", "heads at the two ends", "three heads",
         "twins at one slot", "right-hand side"]


def _columns(n, rng):
    """w (n, 6, 7): one column per kind"""
    w = np.zeros((n, 6, len(KINDS)))
    r = lambda: rng.standard_normal(6)
    w[0, :, 0] = r()
    w[n - 1, :, 1] = r()
    w[n // 2, :, 2] = r()
    w[0, :, 3] = r(); w[n - 1, :, 3] = r()
    w[1, :, 4] = r(); w[n // 2, :, 4] = r(); w[n - 2, :, 4] = r()
    w[n // 3, :, 5] = r() + r()          # (a bounding-box and a 3-D edge of one camera: their W blocks add up)
    w[:, :, 6] = rng.standard_normal((n, 6))
    return w


@pytest.mark.parametrize("n", [15, 31, 47, 7], ids=["stride 16", "stride 32", "stride 48", "short last segment"])
def test_twisted_sweep_against_dense_extended_precision_solve(n):
    rng = np.random.default_rng(0)
    A, B = tw.random_segment(n, rng)
    G = tw.dense(A, B)
    cond = float(np.linalg.cond(G))
    bound = 4 * cond * EPS
    m = tw.segment_matrices(A, B)
    w = _columns(n, rng)
    V = tw.scaled_records(m, w)
    Y, Ys = tw.sweep(m, V), tw.substitution(m, V)
    LD = sr.LD
    for k, kind in enumerate(KINDS):
        z, last = sr.solve_ref(G, w[:, :, k].reshape(6 * n))
        assert last <= 1e-3 * EPS * float(np.abs(z).max())          # the reference has converged
        yref = np.stack([np.asarray(m["L"][i], dtype=LD).T @ z[6 * i:6 * i + 6] for i in range(n)])
        scale = float(np.abs(yref).max())
        e_tw = float(np.abs(Y[:, :, k] - yref).max()) / scale
        e_sub = float(np.abs(Ys[:, :, k] - yref).max()) / scale
        res = float(np.abs(G @ np.concatenate([np.linalg.solve(m["L"][i].T, Y[i, :, k]) for i in range(n)]) - w[:, :, k].reshape(6 * n)).max()
                    / np.abs(w[:, :, k]).max())
        print("%2d slots, %-30s cond %.1e bound %.1e: sweep %.1e (%.3f of the bound), substitution %.1e, sweep's residual %.1e" % (
            n, kind, cond, bound, e_tw, e_tw / bound, e_sub, res))
        assert e_tw <= bound and e_sub <= bound, (kind, e_tw, e_sub, bound)


def test_matrices_are_what_the_definitions_say():
    """P_i^-1 = L^-1 (D+ + D- - A) L^-T and Q_i = L_i^-1 B_i^T D-_{i+1}^-1 L_{i+1}, from unscaled pivots computed separately"""
    rng = np.random.default_rng(1)
    n = 31
    A, B = tw.random_segment(n, rng)
    m = tw.segment_matrices(A, B)
    Dp, Dm = [None] * n, [None] * n
    Dp[0] = A[0]
    for i in range(1, n):
        Dp[i] = A[i] - B[i - 1] @ np.linalg.solve(Dp[i - 1], B[i - 1].T)
    Dm[n - 1] = A[n - 1]
    for i in range(n - 2, -1, -1):
        Dm[i] = A[i] - B[i].T @ np.linalg.solve(Dm[i + 1], B[i])
    cond = float(np.linalg.cond(tw.dense(A, B)))
    for i in range(n):
        L = m["L"][i]
        assert np.allclose(L @ L.T, Dp[i], rtol=0, atol=64 * cond * EPS * np.abs(Dp[i]).max())
        tp = np.linalg.solve(L, np.linalg.solve(L, Dp[i] + Dm[i] - A[i]).T).T
        assert np.allclose(m["P"][i] @ tp, np.eye(6), rtol=0, atol=64 * cond * EPS)
        if i + 1 < n:
            q = np.linalg.solve(L, B[i].T) @ np.linalg.solve(Dm[i + 1], m["L"][i + 1])
            assert np.allclose(m["Q"][i], q, rtol=0, atol=64 * cond * EPS * max(1.0, np.abs(q).max()))
        else:
            assert np.array_equal(m["P"][i], np.eye(6)) and not m["Q"][i].any()


# ---- the premises of the GPU test ---------------------------------------------------------------------------------------------------
SHAPES = {"257": (257, 40, 6), "300": (300, 80, 10), "1100": (1100, 60, 6)}


@functools.lru_cache(maxsize=None)
def _pkg():
    return importlib.import_module("object-oriented-slam_amd")


def _kinds(L, S):
    """Which column kinds the graph's (segment, ellipsoid) columns contain at segments of S slots: from the lists alone."""
    nf = L["nf"]
    slot, obj = np.asarray(L["ue_slot"]), np.asarray(L["ue_obj"])
    p, pos = slot // S, slot % S
    interior = pos != S - 1
    seen = set()
    short = False
    for key in set(zip(p[interior].tolist(), obj[interior].tolist())):
        sel = interior & (p == key[0]) & (obj == key[1])
        at = pos[sel]
        n = min(S - 1, nf - key[0] * S)          # interior slots of this segment
        short |= n < S - 1
        heads = np.unique(at)
        if len(heads) == 1:
            seen.add("first" if heads[0] == 0 else "last" if heads[0] == n - 1 else "middle")
        elif len(heads) == 2:
            seen.add("two")
            if heads[0] == 0 and heads[1] == n - 1:
                seen.add("two ends")
        else:
            seen.add("three")
        if len(at) > len(heads):
            seen.add("twins")
        if heads[0] == 0 and len(heads) > 1:
            seen.add("several from the first slot")
        if heads[-1] == n - 1 and len(heads) > 1:
            seen.add("several to the last slot")
    if short:
        seen.add("short last segment")
    return seen


def test_premises_of_the_gpu_test():
    pkg = _pkg()
    from tests.test_gpu_cf_sep_overlap import _awkward_graph
    from tests.test_gpu_cf_stride import _awkward_graph32
    need = {"first", "last", "middle", "two", "three", "twins", "several from the first slot", "several to the last slot"}
    union = set()
    for name, (n_cams, n_objs, per_cam) in SHAPES.items():
        g = pkg.synth.make_graph(n_cams, n_objs, per_cam * n_cams, seed=41, slam=True)[0]
        L = ref.lists(g)
        for S in ((16,) if name == "1100" else (16, 32, 48)):
            seen = _kinds(L, S)
            print(name, S, sorted(seen))
            assert need <= seen, (name, S, need - seen)
            assert ("short last segment" in seen) == (L["nf"] % S not in (0, S - 1))
            union |= seen
    for tag, g, S in (("awkward", _awkward_graph(pkg)[0], 16), ("awkward32", _awkward_graph32(pkg)[0], 32)):
        seen = _kinds(ref.lists(g), S)
        print(tag, S, sorted(seen))
        # (14 ellipsoids under ten detections a camera: long columns -- what these two graphs add is many heads, from the first slot
        # on and up to the last one, and their short last segment)
        assert {"three", "twins", "several from the first slot", "several to the last slot", "short last segment"} <= seen, (tag, seen)
        union |= seen
    # a column with exactly two heads, one at either end of its segment, in at least one of the graphs; the right-hand side's column
    # (an entry at every slot) is in every segment of every graph
    assert "two ends" in union
