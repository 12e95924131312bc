"""CPU tests of tests/lin_ref.py, the forward-mode multiprecision reference tests/test_gpu_lin.py holds the device's linearisation to:
the premises of every scene in both arithmetics (a), the reference against the numerically differentiated checker (b), 40 against 60
digits (c), that the bound of test_gpu_lin.py is not vacuous (d), and esl_math.hpp's per-edge formulas, compiled for the host
(tests/lin_math_main.cpp, plain and with -fsanitize=undefined), against the reference edge by edge (e).

(e) uses the rule of test_gpu_lin.py per edge: error of r, J_a, J_b (max-norm over the quantity's max-norm, against mpmath at 40 digits) at
most HOST_MARGIN x the error of the float64 forward-mode evaluation of the same quantity + 4 eps.  Measured on the host build over all
scenes, both box residuals, both builds (-s prints every class; an error within 4 eps counts as 0):  worst ratio 12.2 (J_c of a bbox edge of
long_camera: 3.9e-15 against a yardstick of 3.2e-16; next, r of a 3-D edge of long_ellipsoid, 11.9)  ->  HOST_MARGIN = 64.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import lin_ref as lr
from tests import slam_step_ref as sr

HOST_MARGIN = 64.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITHS = (lr.MP(40), lr.F64)


def decisions(ev):
    """the discrete decisions of an evaluated graph, and the asserts that each is taken away from its boundary"""
    out = []
    for e in ev["e3d"] + ev["odom"]:
        d = e.info["d"]
        assert abs(d - lr.LOG_SMALL) >= 1e-7, (e.cls, e.k, d)
        out.append((e.cls, e.k, "small" if d > lr.LOG_SMALL else "acos"))
    for e in ev["e3d"]:
        assert e.info["runner_up"] >= e.info["norm"] * (1 + 1e-3), (e.k, e.info)
        out.append(("e3d", e.k, "yaw", e.info["yaw"]))
    for e in ev["bbox"]:
        if "C22" not in e.info:             # tangency: no branch but the mask
            continue
        if e.r is None:
            assert e.info["C22"] > 1e-3, e.info          # clearly no real outline
        else:
            assert e.info["C22"] < -1e-3 and e.info["du_rel"] > 1e-4 and e.info["dv_rel"] > 1e-4, e.info
        out.append(("bbox", e.k, "nan" if e.r is None else "real"))
    for e in ev["grav"]:
        assert 1 - abs(e.info["cos"]) >= 1e-8, e.info
        out.append(("grav", e.k, e.info["cos"] > 0))
    return out


def masks(g):
    return [tuple(bool(x >= lr.MASK_BELOW) for x in m) for m in g.bbox_meas.reshape(-1, 4)]


@pytest.mark.parametrize("name", list(lr.SCENES))
def test_scene_premises(name):
    """(a) every scene's premises, in the reference and in float64 arithmetic, and the same discrete decisions in both"""
    g, c, o = lr.scene(name)
    evs = [lr.edges_of(name, ar) for ar in ARITHS]
    dec = [decisions(ev) for ev in evs]
    assert dec[0] == dec[1]
    assert np.abs(np.linalg.norm(c[:, 3:7], axis=1) - 1).max() < 4e-16 and np.abs(np.linalg.norm(o[:, 3:7], axis=1) - 1).max() < 4e-16
    per_obj = np.bincount(g.bbox_obj, minlength=g.n_objs), np.bincount(g.e3d_obj, minlength=g.n_objs)
    free = ~g.cam_fixed.astype(bool)
    for ev in evs:
        L = lr.assemble(lr.F64 if ev is evs[1] else lr.MP(40), g, ev)
        assert L.n_dropped == (1 if name == "dropped" else 0)
        if name in ("minimal", "dropped"):
            assert g.n_cams == 2 and free.tolist() == [False, True]
            assert [len(ev[k]) for k in ("bbox", "e3d", "grav", "odom")] == ([2, 1, 1, 1] if name == "minimal" else [4, 1, 2, 1])
        if name == "minimal":
            assert g.n_objs == 1
        if name == "long_ellipsoid":
            # one more than a chunk of bbox edges (64) and than two chunks of 3-D edges (32), all from free cameras; a one-edge neighbour
            assert g.n_cams == 66 and free.sum() == 65 and len(g.odom_i) == 65
            assert per_obj[0].tolist() == [65, 1] and per_obj[1].tolist() == [65, 0]
            assert free[g.bbox_cam].all() and free[g.e3d_cam].all()
        if name == "long_camera":
            assert g.n_cams == 3 and free.sum() == 2 and g.n_objs == 70
            assert np.bincount(g.bbox_cam, minlength=3).tolist() == [70, 70, 70]          # longer than a wave of 64
        if name == "branches":
            e3 = ev["e3d"]
            assert [e.info["yaw"] for e in e3[:4]] == list(lr.YAWS)                          # each of the four yaws wins once
            ang = [float(np.arccos(e.info["d"])) for e in e3[4:]]
            np.testing.assert_allclose(ang, lr.BRANCH_THETAS, rtol=1e-6)
            assert [e.info["d"] > lr.LOG_SMALL for e in e3[4:]] == [True, False, False]
            assert any(free[e.a] for e in e3[4:5]) and any(free[e.a] for e in e3[5:6]) and any(free[e.a] for e in e3[6:])
            od = ev["odom"]
            assert max(abs(float(x)) for x in od[1].r) < 1e-12 and od[1].info["d"] > lr.LOG_SMALL          # consistent: E = I to rounding
            assert max(abs(float(x)) for x in od[0].r) > 0.1 and od[0].info["d"] < lr.LOG_SMALL
            th = [float(e.r[0]) for e in ev["grav"]]
            assert 5e-4 < th[0] < 2e-3 and th[1] > 0.1                                         # nearly aligned, generic
            assert sorted(4 - sum(m) for m in masks(g)) == [0, 0, 1, 2, 4]
            for e in ev["bbox"]:                                                               # a masked entry: residual 0 and a zero row
                for i, on in enumerate(masks(g)[e.k]):
                    assert on or (e.r[i] == 0 and not e.Ja[i].any() and not e.Jb[i].any())
        if name == "dropped":
            bad = [e for e in ev["bbox"] if e.r is None]
            assert len(bad) == 1 and free[bad[0].a] and L.n_valid == 3
            assert sum(1 for e in ev["bbox"] if not free[e.a]) == 2
            for e in ev["bbox"]:
                if e.r is None or not free[e.a]:
                    assert not L.W[L.pos[e.k]].any()
            assert L.edge_chi2["bbox"][bad[0].k] is None


def as_dense(g, L):
    """Lin's blocks in the checker's dense layout (cameras first, then ellipsoids), the blocks it does not hold left zero, and their mask"""
    n, m = 6 * L.nf, 9 * L.N
    H, b, have = np.zeros((n + m, n + m)), np.zeros(n + m), np.zeros((n + m, n + m), dtype=bool)
    f = lambda a: np.array([[float(x) for x in row] for row in a])
    for s in range(L.nf):
        H[6 * s:6 * s + 6, 6 * s:6 * s + 6] = f(L.Hcc[s]); have[6 * s:6 * s + 6, 6 * s:6 * s + 6] = True
        b[6 * s:6 * s + 6] = [float(x) for x in L.bc[s]]
    for o in range(L.N):
        H[n + 9 * o:n + 9 * o + 9, n + 9 * o:n + 9 * o + 9] = f(L.Hoo[o]); have[n + 9 * o:n + 9 * o + 9, n + 9 * o:n + 9 * o + 9] = True
        b[n + 9 * o:n + 9 * o + 9] = [float(x) for x in L.bo[o]]
    ucam, uobj = sr.edge_order(g)
    for u in range(len(ucam)):
        s, o = int(L.slot[ucam[u]]), int(uobj[u])
        have[:n, n + 9 * o:n + 9 * o + 9] = True          # (a camera-ellipsoid block without an edge is zero in both)
        if s >= 0:
            H[6 * s:6 * s + 6, n + 9 * o:n + 9 * o + 9] += f(L.W[u])
    H[n:, :n] = H[:n, n:].T; have[n:, :n] = have[:n, n:].T
    return H, b, have


@pytest.mark.parametrize("name", ["minimal", "branches", "dropped"])
def test_reference_matches_checker(po, name):
    """(b) H, b and chi2 of the reference against the checker's numerically differentiated system, at the 5e-6 of the block's (vector's)
    largest entry the suite uses for the device: the conventions (orders, signs, retractions, weights) are the checker's"""
    g, c, o = lr.scene(name)
    H, b, fidx, chi2 = po.build_system(g, c, o, delta=1e-6)
    L = lr.lin_of(name, lr.MP(40))
    assert len(b) == 6 * L.nf + 9 * L.N
    Hr, br, have = as_dense(g, L)
    assert float(L.chi2) == pytest.approx(chi2, rel=1e-9)
    assert float(L.max_diag) == pytest.approx(np.abs(np.diag(H)).max(), rel=1e-5)
    np.testing.assert_allclose(br, b, rtol=0, atol=5e-6 * max(np.abs(b).max(), 1.0))
    blocks = [(6 * s, 6) for s in range(L.nf)] + [(6 * L.nf + 9 * k, 9) for k in range(L.N)]
    for i, ni in blocks:
        for j, nj in blocks:
            if have[i, j]:
                want = H[i:i + ni, j:j + nj]
                np.testing.assert_allclose(Hr[i:i + ni, j:j + nj], want, rtol=0, atol=5e-6 * np.abs(want).max(),
                                           err_msg="%s block (%d, %d)" % (name, i, j))


@pytest.mark.parametrize("name", list(lr.SCENES))
def test_reference_precision(name):
    """(c) the 40-digit evaluation against a 60-digit one: 1e-30 on every quantity, tangency included where test_gpu_lin.py runs it"""
    for mode in (0, 1) if name in lr.TANGENCY_SCENES else (0,):
        e = lr.errors(lr.MP(60), lr.lin_of(name, lr.MP(40), mode), lr.lin_of(name, lr.MP(60), mode))
        assert max(e.values()) <= 1e-30, e


def configurations():
    for name in lr.SCENES:
        for slam in (True, False):
            for mode in (0, 1) if name in lr.TANGENCY_SCENES else (0,):
                yield name, slam, mode


def test_yardsticks_are_small():
    """the float64 evaluation is never further than YARDSTICK_MAX from the reference: a larger yardstick would only widen what the
    device is allowed"""
    worst = (0.0, "")
    for name, slam, mode in configurations():
        y = lr.yardsticks(name, mode, slam)
        print(name, "slam" if slam else "mapping", "tangency" if mode else "", {k: "%.1e" % v for k, v in y.items()})
        worst = max(worst, max((v, "%s %s %d %s" % (name, slam, mode, k)) for k, v in y.items()))
    print("largest yardstick: %.2e (%s)" % worst)
    assert worst[0] <= lr.YARDSTICK_MAX


@pytest.mark.parametrize("name", list(lr.SCENES))
def test_bound_is_not_vacuous(name):
    """(d) the float64 blocks themselves with the largest entry of ONE block off by 1e-10 of itself violate test_gpu_lin.py's bound, for
    every block of every quantity of the scene"""
    mp = lr.MP(40)
    for mode in (0, 1) if name in lr.TANGENCY_SCENES else (0,):
        _bumped_blocks_violate(name, mode, mp)


def _bumped_blocks_violate(name, mode, mp):
    ref, f64, y = lr.lin_of(name, mp, mode), lr.lin_of(name, lr.F64, mode), lr.yardsticks(name, mode)
    n = 0
    for q in ("Hoo", "Hcc", "W", "bo", "bc"):
        A = np.asarray(getattr(f64, q), dtype=np.float64)
        for k in range(len(A)):
            if not A[k].any():
                continue
            B = A.copy()
            i = np.unravel_index(np.abs(B[k]).argmax(), B[k].shape)
            if q in lr.Lin.GRADS and abs(A[k][i]) < np.abs(A).max():
                continue          # (a gradient is one quantity: only its largest entry of all is 1e-10 of the scale)
            B[k][i] *= 1 + 1e-10
            err = lr.rel_err(mp, B[k], getattr(ref, q)[k]) if q in lr.Lin.BLOCKS else lr.rel_err(mp, B, getattr(ref, q))          # (a block's own error: the worst over the blocks is no smaller)
            assert err > lr.allow(lr.GROUP[q], y[q]), (name, q, k, err, y[q])
            n += 1
    for q in ("chi2", "max_diag"):
        err = lr.rel_err(mp, [float(getattr(f64, q)) * (1 + 1e-10)], [getattr(ref, q)])
        assert err > lr.allow("scalar", y[q]), (name, q, err, y[q])
    assert n >= 3


# ---- (e) esl_math.hpp compiled for the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "ubsan"])
def host_program(request, tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"          # (the default of csrc/Makefile)
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("lin_math") / ("lin_math_main_" + request.param))
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-I", os.path.join(ROOT, "object-oriented-slam_amd", "csrc"),
           os.path.join(ROOT, "tests", "lin_math_main.cpp"), "-o", exe]
    if request.param == "ubsan":
        cmd[5:5] = ["-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0 and request.param == "ubsan":
        pytest.skip("no undefined-behaviour sanitizer runtime for the host compiler: " + p.stderr[-300:])
    assert p.returncode == 0, p.stderr
    return exe


def host_lines(g, c, o, mode):
    f = lambda *arrs: " ".join("%.17g" % x for a in arrs for x in np.asarray(a, dtype=np.float64).reshape(-1))
    lines, keys = [], []
    for k in range(len(g.odom_i)):
        lines.append("odom " + f(c[g.odom_i[k]], c[g.odom_j[k]], g.odom_meas.reshape(-1, 7)[k])); keys.append(("odom", k))
    for k in range(len(g.grav_obj)):
        lines.append("grav " + f(o[g.grav_obj[k]], g.grav_normal[:3])); keys.append(("grav", k))
    for k in range(len(g.bbox_cam)):
        lines.append("bbox %d " % mode + f(c[g.bbox_cam[k]], o[g.bbox_obj[k]], g.K, g.bbox_meas.reshape(-1, 4)[k])); keys.append(("bbox", k))
    for k in range(len(g.e3d_cam)):
        lines.append("e3d " + f(c[g.e3d_cam[k]], o[g.e3d_obj[k]], g.e3d_meas.reshape(-1, 10)[k])); keys.append(("e3d", k))
    return lines, keys


@pytest.mark.parametrize("name", list(lr.SCENES))
def test_host_formulas_per_edge(host_program, name):
    """(e) r, J_a, J_b of every edge from esl_math.hpp on the host against the reference, under the rule of test_gpu_lin.py per edge"""
    mp = lr.MP(40)
    g, c, o = lr.scene(name)
    worst = {}
    for mode in (0, 1) if name in lr.TANGENCY_SCENES else (0,):
        lines, keys = host_lines(g, c, o, mode)
        p = subprocess.run([host_program], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        out = p.stdout.splitlines()
        assert len(out) == 3 * len(keys)
        ref, f64 = lr.edges_of(name, mp, mode), lr.edges_of(name, lr.F64, mode)
        for n, (cls, k) in enumerate(keys):
            got = {ln.split()[0]: np.array(ln.split()[1:], dtype=np.float64) for ln in out[3 * n:3 * n + 3]}
            er, ey = ref[cls][k], f64[cls][k]
            if er.r is None:
                assert np.isnan(got["r"]).all(), (name, cls, k)          # the dropped box: NaN in the product too
                continue
            for q in ("r", "Ja", "Jb"):
                want = getattr(er, q)
                if want is None:
                    assert got[q].size == 0
                    continue
                if q == "r" and cls == "odom" and max(abs(x) for x in want) < 1e-12:
                    assert np.abs(got[q]).max() < 1e-12          # the consistent odometry edge: its residual is the rounding of Z
                    continue
                err, y = lr.rel_err(mp, got[q], want), lr.rel_err(mp, getattr(ey, q), want)
                key = "%s %s" % (cls if cls != "bbox" else ("tangency" if mode else "bbox"), q)
                worst[key] = max(worst.get(key, (0.0, 0, 0.0, 0.0)), (lr.ratio(err, y), k, err, y))
                assert err <= HOST_MARGIN * y + lr.FLOOR, (name, cls, k, q, err, y)
    print("\n%s: worst ratios host error / float64 yardstick: " % name + ", ".join("%s %.2f (edge %d: %.1e / %.1e)" % ((k,) + v) for k, v in sorted(worst.items())))
