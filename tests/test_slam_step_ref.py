"""CPU tests of tests/slam_step_ref.py (the extended-precision SLAM trial step tests/test_gpu_slam_step.py holds the device to) and of
the premises of every graph that file runs: the reference against the checker's dense system solved whole, against mpmath where it is
importable, its retractions against oracle/np_oracle.py's, and each case's sizes and structure."""
import numpy as np
import pytest

from tests import slam_step_ref as sr

LD = sr.LD


def checker_system(pkg, po, name):
    """the checker's dense H, b (numeric Jacobians, delta = 1e-6) of a case, H made exactly symmetric (its two triangles are
    accumulated in different orders and differ in the last bit; the blocks take the upper one)"""
    g, c, o = sr.build_case(pkg, name)
    H, b, fidx, _ = po.build_system(g, c, o, delta=1e-6)
    H = np.triu(H) + np.triu(H, 1).T
    return g, c, o, H, b, fidx


@pytest.mark.parametrize("name", ["A_6c_2e", "B_23c_15e"])
def test_reference_reproduces_the_whole_system(pkg, po, name):
    """schur_ref + solve_ref + backsub_ref on the blocks of the checker's H, b against solve_ref of the whole (H + lambda I) x = b: two
    eliminations of one system, both in longdouble, must agree to 1e-15 of max|x|; numpy's float64 solves of the same system sit at
    their usual distance from it (measured on these sub-graphs: 7e-15 .. 3e-13 at the small damping)."""
    g, c, o, H, b, fidx = checker_system(pkg, po, name)
    B, hodo = sr.blocks_from_dense(g, H, b, fidx)
    n = 6 * B.nf
    md = float(np.abs(np.diag(H)).max())
    for f in (sr.LAM_SMALL, sr.LAM_BIG):
        lam = f * md
        ref = sr.reference_step(B, lam, hodo=hodo)
        x, last = sr.solve_ref(np.asarray(H, dtype=LD) + LD(lam) * np.eye(len(b), dtype=LD), b)
        xmax = float(np.abs(x).max())
        e_c = float(np.abs(ref["xc"] - x[:n]).max()) / xmax
        e_o = float(np.abs(ref["xo"].reshape(-1) - x[n:]).max()) / xmax
        y = sr.f64_yardsticks(B, lam, ref["hodo"], ref)
        print("%s lambda %.0e max_diag: reduced vs whole system x_c %.1e x_o %.1e of max|x|, last corrections %.1e / %.1e, float64 yardsticks %s"
              % (name, f, e_c, e_o, last / xmax, ref["xc_last"] / xmax, {k: "%.1e" % v for k, v in y.items()}))
        assert e_c <= 1e-15 and e_o <= 1e-15
        assert last <= 1e-3 * 1e-15 * xmax and ref["xc_last"] <= 1e-3 * 1e-15 * xmax
        for k in ("S", "bs", "xc", "xo"):
            assert y[k] <= 1e-11, (k, y[k])
            if f == sr.LAM_SMALL:      # (under the large damping the system is nearly diagonal and float64 can be exact to the last bit)
                assert y[k] >= 1e-16, (k, y[k])


def test_reference_against_mpmath_on_the_smallest_system(pkg, po):
    mp = pytest.importorskip("mpmath")
    g, c, o, H, b, fidx = checker_system(pkg, po, "A_2c_1e")
    B, hodo = sr.blocks_from_dense(g, H, b, fidx)
    assert B.nf == 1 and B.N == 1 and not hodo and len(b) == 15
    md = float(np.abs(np.diag(H)).max())
    mp.mp.dps = 40
    for f in (sr.LAM_SMALL, sr.LAM_BIG):
        lam = f * md
        ref = sr.reference_step(B, lam, hodo=hodo)
        A = mp.matrix(H.tolist()) + mp.mpf(lam) * mp.eye(15)
        x = mp.lu_solve(A, mp.matrix(b.tolist()))
        got = np.concatenate([ref["xc"], ref["xo"].reshape(-1)])
        xmax = max(abs(v) for v in x)
        hi = got.astype(np.float64)
        lo = (got - hi).astype(np.float64)                       # longdouble = hi + lo exactly
        err = max(abs(mp.mpf(float(hi[i])) + mp.mpf(float(lo[i])) - x[i]) for i in range(15)) / xmax
        print("2 cameras / 1 ellipsoid, lambda %.0e max_diag: longdouble path vs mpmath at 40 digits %.1e of max|x|" % (f, float(err)))
        assert err <= 1e-17


def inverse_hilbert(n):
    """the inverse of the n x n Hilbert matrix: integers, known in closed form"""
    from math import comb
    return np.array([[(-1) ** (i + j) * (i + j + 1) * comb(n + i, n - j - 1) * comb(n + j, n - i - 1) * comb(i + j, i) ** 2 for j in range(n)]
                     for i in range(n)], dtype=LD)


def test_inverse_and_solve_in_longdouble():
    """the two building blocks on a matrix whose entries AND whose inverse are known exactly: the inverse Hilbert matrix of order 6
    (integers up to 4.4e6, cond 1.5e7 -- a plain longdouble factorisation would leave cond * eps = 1e-12)"""
    A = inverse_hilbert(6)
    hilbert = np.array([[LD(1) / LD(i + j + 1) for j in range(6)] for i in range(6)], dtype=LD)
    X = sr.inv_spd_ld(A)
    assert float(np.abs(X - hilbert).max()) < 1e-17
    x0 = np.array([3, -1, 4, 1, -5, 9], dtype=LD)
    x, last = sr.solve_ref(A, A @ x0)                 # integers: A x0 is exact
    assert float(np.abs(x - x0).max()) < 1e-17 and last < 1e-16


def test_retractions_match_np_oracle(pkg):
    """cam_oplus_ld / obj_oplus_ld against np_oracle's float64 cam_oplus / obj_oplus to 1e-14, on both sides of se3_exp's small-angle
    threshold (|omega| < 1e-5)"""
    g, c, o = sr.base_graph(pkg)
    rng = np.random.default_rng(11)
    sizes = np.concatenate([[0.0, 1e-9, 3e-7, 5e-6, 9.9e-6, 1.01e-5, 2e-5, 1e-3], 10.0 ** rng.uniform(-8, -0.3, size=42)])
    assert len(sizes) == 50 and (sizes < sr.SMALL_ANGLE).sum() >= 5 and (sizes > sr.SMALL_ANGLE).sum() >= 5
    worst = 0.0
    for k, th in enumerate(sizes):
        w = rng.standard_normal(3); w *= th / np.linalg.norm(w)
        # np_oracle's general branch loses eps |upsilon| / |omega| of the translation to the cancellation in (1 - cos theta) / theta^2:
        # just above the threshold the translation is scaled with theta, so that loss stays under the 1e-14 compared here
        t_size = 0.1 if th < sr.SMALL_ANGLE else min(0.1, 10 * th)
        u = np.concatenate([w, t_size * rng.standard_normal(3), 0.05 * rng.standard_normal(3)])
        assert (np.linalg.norm(u[:3]) < sr.SMALL_ANGLE) == (th < sr.SMALL_ANGLE)
        cam, obj = c[1 + k % (len(c) - 1)], o[k % len(o)]
        e_c = sr.state_err(sr.cam_oplus_f64(cam, u[:6]), sr.cam_oplus_ld(cam, u[:6]))
        e_o = sr.state_err(sr.obj_oplus_f64(obj, u), sr.obj_oplus_ld(obj, u))
        worst = max(worst, e_c, e_o)
        assert e_c <= 1e-14 and e_o <= 1e-14, (th, e_c, e_o)
        q = sr.cam_oplus_ld(cam, u[:6])[3:7]
        assert abs(float(q @ q) - 1) < 1e-18 and q[3] >= 0
    # against the C checker's retractions too (quaternion form, like the device's)
    from oracle import pyoracle as po
    u = np.array([0.02, -0.01, 0.03, 0.1, 0.2, -0.1, 0.01, 0.02, -0.01])
    assert sr.state_err(po.cam_oplus(c[1], u[:6]), sr.cam_oplus_ld(c[1], u[:6])) <= 1e-14
    assert sr.state_err(po.obj_oplus(o[0], u), sr.obj_oplus_ld(o[0], u)) <= 1e-14
    print("longdouble retractions vs np_oracle's: worst %.1e over 50 updates" % worst)


def panels(n):
    return (n + 127) // 128


def touched_by_odometry(g):
    t = np.zeros(g.n_cams, dtype=bool)
    t[g.odom_i] = True; t[g.odom_j] = True
    return t


@pytest.mark.parametrize("name", list(sr.CASES))
def test_case_premises(pkg, po, name):
    """every graph of tests/test_gpu_slam_step.py is the case its row of slam_step_ref.CASES says it is"""
    prem = sr.CASES[name][3]
    g, c, o = sr.build_case(pkg, name)
    free = ~g.cam_fixed.astype(bool)
    nf = int(free.sum())
    assert g.cam_fixed[0] == 1 and nf == g.n_cams - 1 == prem["nf"]
    assert panels(6 * nf) == prem["p6"] and panels(9 * g.n_objs) == prem["p9"]
    if "seg" in prem:
        assert (nf + 15) // 16 == prem["seg"]
    pc, pob = sr.per_cam_counts(g), sr.per_obj_counts(g)
    assert ((pc > 0) | touched_by_odometry(g))[free].all()              # every free camera has an edge or an odometry neighbour
    assert len(g.odom_i) == nf and sr.odom_pairs(g) == [(i, i + 1) for i in range(nf - 1)]   # the chain is kept
    if prem.get("every_obj_seen"):
        assert pob.min() >= 1
    assert (pob.max() > 64) == (prem.get("obj_list") == "long")
    assert (pc[free].max() > 64) == (prem.get("cam_list") == "long")
    if prem.get("mixed"):
        assert sr.has_bbox_and_e3d_pair(g)
    if sr.CASES[name][0] == "sub":
        assert (g.n_cams, g.n_objs) == sr.CASES[name][1:3]
    assert 6 * nf + 9 * g.n_objs <= 1900
    # the two dampings: under the large one every camera's rotation update is on the small-angle branch of se3_exp, under the small
    # one none is (from the checker's system here; the GPU test asserts both from the reference on the device's blocks)
    H, b, fidx, _ = po.build_system(g, c, o, delta=1e-6)
    md = float(np.abs(np.diag(H)).max())
    n = 6 * nf
    for f, small in ((sr.LAM_SMALL, False), (sr.LAM_BIG, True)):
        x = np.linalg.solve(H + f * md * np.eye(len(b)), b)
        om = np.linalg.norm(x[:n].reshape(-1, 6)[:, :3], axis=1)
        assert (om.max() < 0.5 * sr.SMALL_ANGLE) if small else (om.min() > 2 * sr.SMALL_ANGLE), (f, om.min(), om.max())


def test_case_premises_shapes_named_in_the_table():
    """the sizes the cases are there for: 6 nf = 126 / 132 and 9 N = 18 / 135 (one and two panels), 258 / 261 (three), the 16-camera
    segment from both sides, the 64-lane trips"""
    c = sr.CASES
    assert [6 * c[k][3]["nf"] for k in ("B_22c_2e", "B_23c_2e", "C_44c_29e")] == [126, 132, 258]
    assert [9 * c[k][2] for k in ("B_22c_2e", "B_22c_15e", "C_44c_29e")] == [18, 135, 261]
    assert (c["C_17c_15e"][3]["nf"], c["C_18c_15e"][3]["nf"]) == (16, 17)
    assert c["D_66c_29e"][3]["obj_list"] == "long" and c["D_long_camera_list"][3]["cam_list"] == "long"
    assert [n - 1 for n in sr.F_CAMS] == [1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 65]


@pytest.mark.parametrize("odometry", [True, False])
@pytest.mark.parametrize("n_cams", sr.F_CAMS)
def test_fixed_map_case_premises(pkg, n_cams, odometry):
    g, c, o = sr.build_f_case(pkg, n_cams, odometry)
    free = ~g.cam_fixed.astype(bool)
    assert int(free.sum()) == n_cams - 1 and g.n_objs == sr.F_OBJS
    assert len(g.odom_i) == (n_cams - 1 if odometry else 0)
    assert (sr.per_cam_counts(g)[free] > 0).all()                  # every free camera sees the map: no empty block without odometry
    assert sr.odom_pairs(g) == ([(i, i + 1) for i in range(n_cams - 2)] if odometry else [])
