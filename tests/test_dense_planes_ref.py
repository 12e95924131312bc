"""The numpy statement of esl_dense_planes (tests/dense_planes_ref.py) held to closed forms, and csrc/esl_dense_planes.hpp -- the header
the kernels and the host side compile -- held to hand-computed cases and, bit for bit, to the statement (tests/dense_planes_main.cpp).
The conditions the GPU scene tests rely on are asserted here, on the statement alone.  No GPU."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as dr                # noqa: E402
import dense_planes_ref as dpr        # noqa: E402
import dense_planes_scenes as ps      # noqa: E402
from dense_prog import build_prog          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = ps.LEAF


def ext_of(keys, count=None):
    """an extract of bare keys (sorted by packed key), one sample per voxel unless count is given, no labels"""
    keys = np.asarray(keys, dtype=np.int64)
    order = np.argsort(dr.pack(keys))
    count = np.ones(len(keys), np.int32) if count is None else np.asarray(count, dtype=np.int32)
    return dict(n_voxels=len(keys), key=keys[order].astype(np.int32), count=count[order], votes=np.zeros(len(keys), np.int32))


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------------
def splitmix_by_hand(x):
    """the finaliser of x, every step written out with explicit masks"""
    m = (1 << 64) - 1
    x = (x ^ (x >> 30)) & m
    x = (x * 0xBF58476D1CE4E5B9) % (1 << 64)
    x = (x ^ (x >> 27)) & m
    x = (x * 0x94D049BB133111EB) % (1 << 64)
    return (x ^ (x >> 31)) & m


def test_mix_is_pinned():
    g = 0x9E3779B97F4A7C15
    assert dpr.mix(0, 0, 64, 0, 0) == 0xE220A8397B1DCDAF          # the counter is 1: splitmix64's first output from state 0
    assert dpr.mix(0, 0, 64, 0, 1) == splitmix_by_hand((2 * g) % (1 << 64)) == 0x6E789E6AA1B965F4          # its second output
    assert dpr.mix(0, 0, 64, 0, 2) == 0x06C45D188009454F          # and its third
    assert dpr.mix(7, 2, 100, 7, 2) == splitmix_by_hand(7 ^ ((g * (4 * 207 + 3)) % (1 << 64)))
    assert dpr.mix((1 << 64) - 1, 63, 65536, 65535, 2) == splitmix_by_hand(((1 << 64) - 1) ^ ((g * (4 * (63 * 65536 + 65535) + 3)) % (1 << 64)))
    assert dpr.index(0, 0, 64, 0, 0, 1000) == (0xE220A8397B1DCDAF >> 11) % 1000
    idx = [dpr.index(3, 1, 256, h, k, 977) for h in range(256) for k in range(3)]
    assert min(idx) >= 0 and max(idx) < 977 and len(set(idx)) > 500          # spread over the list


# ---- closed forms -------------------------------------------------------------------------------------------------------------------------------
def test_lattice_slab_every_valid_hypothesis_is_the_plane():
    e = ext_of(ps.slab_z(40, 40))
    r = dpr.planes(e, LEAF, dist_tol=0.004, n_hypotheses=256, min_inliers=50, max_planes=1)
    h = r["hyp"][0]
    valid = h[:, 0] == 1
    assert 100 < valid.sum() < 256 and (h[valid, 1] == 1600).all() and (h[valid, 2] == 1600).all() and not h[~valid].any()
    assert r["result"] == dict(status=0, n_voxels=1600, n_eligible=1600, n_planes=1, n_assigned=1600, ground_index=-1, rounds=1, stop_reason=0)
    assert r["stats"][0].tolist()[:5] == [1600, 1600, int(valid.sum()), int(np.flatnonzero(valid)[0]), 1600]
    pl = r["planes"][0]
    assert pl[0] == 0 and pl[1] == 0 and abs(pl[2]) == 1 and pl[3] == 0.005 and pl[2] == -1          # d^ > 0 decides the sign
    assert np.abs(r["centroid"][0] - [0.2, 0.2, 0.005]).max() <= 1e-15 and r["samples"].tolist() == [1600]
    # every valid hypothesis by itself
    U = e["key"].astype(np.int64)
    for hh in np.flatnonzero(valid)[:40]:
        i = [dpr.index(0, 0, 256, int(hh), k, 1600) for k in range(3)]
        p = dpr.hypothesis(i, *[[int(x) for x in U[j]] for j in i], 8, LEAF)
        assert p[0] == 0 and p[1] == 0 and abs(p[2]) == 1 and abs(p[3]) == 0.005


def test_diagonal_slab():
    e = ext_of(ps.build("diag")[0])
    r = dpr.planes(e, LEAF, dist_tol=0.004, n_hypotheses=64, min_inliers=50, max_planes=1, refine=0)
    s = np.sqrt(0.5)
    assert r["stats"][0, 0] == 900 and np.abs(r["planes"][0] - [-s, 0, -s, 0.61 * s]).max() <= 1e-15
    v = r["hyp"][0]
    assert (v[v[:, 0] == 1, 1] == 900).all()
    r1 = dpr.planes(e, LEAF, dist_tol=0.004, n_hypotheses=64, min_inliers=50, max_planes=1)
    assert r1["stats"][0].tolist()[4:6] == [900, 1] and np.abs(r1["planes"][0] - r["planes"][0]).max() <= 1e-12
    assert (r1["voxel_plane"] == 0).all()          # the refit of an exact lattice plane returns the same inlier set


def test_orientation_rules():
    assert dpr.orient_out([0.0, 0.0, 1.0, -0.5]) == [-0.0, -0.0, -1.0, 0.5] and dpr.orient_out([0.0, 0.0, -1.0, 0.5]) == [0.0, 0.0, -1.0, 0.5]
    assert dpr.orient_out([0.0, -1.0, 0.0, 0.0]) == [0.0, 1.0, 0.0, 0.0] and dpr.orient_out([0.0, 1.0, 0.0, 0.0])[1] == 1.0
    assert dpr.orient_out([-0.6, 0.8, 0.0, 0.0])[:2] == [0.6, -0.8] and dpr.orient_out([0.0, 0.0, 0.5, 0.0])[2] == 0.5


def test_ground_choice():
    up = dpr.up_unit((0, 0, 3.0))
    assert up == [0.0, 0.0, 1.0] and dpr.up_unit((0, 0, 0)) is None
    # up = +z.  The floor z = -1 (below the origin) is (0, 0, 1, 1) in planes_out and as the ground.  The floor z = +1 (above the origin)
    # is (0, 0, -1, 1) in planes_out, d^ > 0, and (0, 0, 1, -1) as the ground, n^ . up^ > 0
    below = [0.0, 0.0, 1.0, 1.0]; above = [0.0, 0.0, -1.0, 1.0]; wall = [1.0, 0.0, 0.0, 2.0]; slope = [0.0, 0.6, 0.8, 3.0]
    assert dpr.ground([wall, below], [900, 500], up, 0.7071067811865476) == (1, below)
    g, pl = dpr.ground([wall, above], [900, 500], up, 0.7071067811865476)
    assert g == 1 and pl == [-0.0, -0.0, 1.0, -1.0] and pl != above          # planes_out and ground_out differ in sign
    assert dpr.ground([wall], [900], up, 0.5) == (-1, [0.0] * 4)
    assert dpr.ground([wall, slope, below], [900, 500, 500], up, 0.7071067811865476)[0] == 1          # ties to the lowest index
    assert dpr.ground([wall, slope, below], [900, 500, 501], up, 0.7071067811865476)[0] == 2
    assert dpr.ground([wall, slope, below], [900, 500, 400], up, 0.81)[0] == 2          # 0.8 < 0.81: the slope is no candidate
    # through the whole statement: the slab kz = 30 with up = -z lies "above" the origin
    e = ext_of(ps.slab_z(20, 20, 30))
    r = dpr.planes(e, LEAF, dist_tol=0.004, n_hypotheses=32, min_inliers=50, max_planes=2, up=(0, 0, -2.0))
    assert r["result"]["ground_index"] == 0 and r["result"]["n_planes"] == 1
    assert r["planes"][0].tolist() == [0.0, 0.0, -1.0, 0.305] or r["planes"][0].tolist() == [-0.0, -0.0, -1.0, 0.305]
    assert r["ground"].tolist() == r["planes"][0].tolist()
    r = dpr.planes(e, LEAF, dist_tol=0.004, n_hypotheses=32, min_inliers=50, max_planes=2, up=(0, 0, 1.0))
    assert r["ground"][2] == 1.0 and r["ground"][3] == -0.305 and r["planes"][0][2] == -1.0          # opposite signs
    assert dpr.planes(e, LEAF, dist_tol=0.004, n_hypotheses=32, min_inliers=50, up=(0, 1.0, 0))["result"]["ground_index"] == -1


def test_guard_at_its_boundary():
    assert dpr.guard(1, 1 << 31) and not dpr.guard(1, (1 << 31) - 1) and dpr.guard(1 << 22, 1 << 20) and not dpr.guard((1 << 22) - 1, 1 << 20)
    # inside the statement: the guard depends on the winner's n and the eligible box alone; forced by shrinking the constant
    e = ext_of(ps.slab_z(40, 40))
    old = dpr.GUARD
    try:
        dpr.GUARD = 1600 * 40 * 40
        r = dpr.planes(e, LEAF, dist_tol=0.004, n_hypotheses=32, min_inliers=50, max_planes=1)
        assert r["stats"][0, 5] == 3 and r["stats"][0, 0] == 1600
        dpr.GUARD = 1600 * 40 * 40 + 1
        assert dpr.planes(e, LEAF, dist_tol=0.004, n_hypotheses=32, min_inliers=50, max_planes=1)["stats"][0, 5] == 1
    finally:
        dpr.GUARD = old


def test_jacobi_against_numpy():
    rng = np.random.default_rng(4)
    for _ in range(50):
        A = rng.normal(size=(3, 3)) * rng.uniform(0.1, 30, 3)
        S = A @ A.T
        n = dpr.jacobi_min([S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]])
        w, v = np.linalg.eigh(S)
        assert abs(np.linalg.norm(n) - 1) <= 1e-15 and np.abs(S @ n - w[0] * np.array(n)).max() <= 1e-10 * max(1.0, w[2])


@pytest.mark.parametrize("n_hyp", [64, 256])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_planted_scene(seed, n_hyp):
    """the condition the GPU scene test relies on: three planes, every planted voxel in a plane that contains it, then reason 3"""
    s = ps.scene("planted")
    e = s["ext"]
    assert e["n_voxels"] == 3047
    r = dpr.planes(e, LEAF, n_hypotheses=n_hyp, seed=seed, **ps.PLANTED)
    assert r["result"] == dict(status=0, n_voxels=3047, n_eligible=3047, n_planes=3, n_assigned=2904, ground_index=-1, rounds=4, stop_reason=3)
    assert r["stats"][:, 0].tolist() == [1600, 901, 403] and r["samples"].tolist() == [1600, 901, 403]
    assert 8 <= r["hyp"][3][:, 1].max() <= 13          # the best leftover
    truth = ps.planted_truth(e["key"].astype(np.int64))
    vp = r["voxel_plane"]
    planted = truth != 0
    assert (vp[planted] >= 0).all() and ((truth[planted] >> vp[planted]) & 1).all()
    assert ((vp == -2) | (vp >= 0)).all() and (vp == -2).sum() == 3047 - 2904
    s2 = np.sqrt(0.5)
    want = np.array([[0, 0, -1, 0.005], [-s2, 0, -s2, 0.61 * s2], [0, -1, 0, 0.455]])
    assert np.abs(r["planes"] - want).max() <= 1e-12


def test_refit_kept_and_rejected():
    """the two refit cases of the GPU tests, asserted on the statement"""
    e = ps.scene("thick")["ext"]
    kw = dict(dist_tol=1.5 * LEAF, n_hypotheses=128, min_inliers=100, max_planes=2)
    r1, r0 = dpr.planes(e, LEAF, **kw), dpr.planes(e, LEAF, refine=0, **kw)
    assert r1["stats"][0, 5] == 1 and r0["stats"][0, 5] == 0 and r1["stats"][0, 0] >= r1["stats"][0, 4] == r0["stats"][0, 0]
    n = np.array([1, 2, 5]) / np.sqrt(30)
    assert abs(abs(r1["planes"][0, :3] @ n) - 1) < abs(abs(r0["planes"][0, :3] @ n) - 1) < 1e-3          # the refit is closer to (1, 2, 5)
    e = ps.scene("rejected")["ext"]
    r = dpr.planes(e, LEAF, dist_tol=1.2 * LEAF, n_hypotheses=128, min_inliers=100, max_planes=1)
    assert r["stats"][0, 5] == 2 and r["stats"][0, 0] == r["stats"][0, 4] == 1008
    r0 = dpr.planes(e, LEAF, dist_tol=1.2 * LEAF, n_hypotheses=128, min_inliers=100, max_planes=1, refine=0)
    assert r0["planes"].tobytes() == r["planes"].tobytes() and (r0["voxel_plane"] == r["voxel_plane"]).all()


def test_ties_layers_and_gates_on_the_statement():
    L = LEAF
    kw = dict(dist_tol=0.004, n_hypotheses=128, min_inliers=50, min_baseline=4)
    r = dpr.planes(ps.scene("twins_samples")["ext"], L, **kw)
    assert r["samples"].tolist() == [800, 400] and r["stats"][:, 0].tolist() == [400, 400] and r["planes"][0, 3] == 0.305          # samples decide
    full = r["hyp"][0][:, 1] == 400
    assert set(r["hyp"][0][full, 2].tolist()) == {400, 800}          # both slabs were hit: the order decided, not luck
    r = dpr.planes(ps.scene("twins")["ext"], L, **kw)
    assert r["stats"][0, 3] == np.flatnonzero(r["hyp"][0][:, 1] == 400)[0] and r["stats"][:, 0].tolist() == [400, 400]          # the smaller h
    r = dpr.planes(ps.scene("layers")["ext"], L, dist_tol=0.4 * L, n_hypotheses=128, min_inliers=50, min_baseline=4)
    assert r["stats"][:, 0].tolist() == [900, 900] and r["result"]["stop_reason"] == 1
    r = dpr.planes(ps.scene("layers")["ext"], L, dist_tol=1.2 * L, n_hypotheses=128, min_inliers=50, min_baseline=4)
    assert r["stats"][:, 0].tolist() == [1800] and r["result"]["stop_reason"] == 1
    g = ps.scene("gates")["ext"]
    r = dpr.planes(g, L, min_count=2, **kw)
    assert r["result"]["n_eligible"] == int((g["count"] >= 2).sum()) < g["n_voxels"] and (r["voxel_plane"][g["count"] < 2] == -1).all()
    r = dpr.planes(g, L, skip_labelled=1, **kw)
    assert r["result"]["n_eligible"] == int((g["votes"] == 0).sum()) == g["n_voxels"] - 400 and (r["voxel_plane"][g["votes"] > 0] == -1).all()
    r = dpr.planes(ps.scene("gates_nolabels")["ext"], L, skip_labelled=1, **kw)
    assert r["result"]["n_eligible"] == g["n_voxels"] and r["result"]["n_planes"] == 2


def test_short_lists_on_the_statement():
    kw = dict(dist_tol=0.004, n_hypotheses=64, min_inliers=3, min_baseline=1)
    for n in (1, 2):
        r = dpr.planes(ps.scene(f"few{n}")["ext"], LEAF, **kw)
        assert r["result"] == dict(status=0, n_voxels=n, n_eligible=n, n_planes=0, n_assigned=0, ground_index=-1, rounds=0, stop_reason=1)
    r = dpr.planes(dr.DenseMap(leaf=LEAF).extract(), LEAF, **kw)
    assert r["result"] == dict(dict.fromkeys(dpr.RESULT, 0), ground_index=-1, stop_reason=1) and r["hyp"].shape == (0, 64, 3)
    r = dpr.planes(ps.scene("line3")["ext"], LEAF, **kw)
    assert r["result"]["stop_reason"] == 2 and r["result"]["rounds"] == 1 and not r["hyp"].any()
    r = dpr.planes(ps.scene("few3")["ext"], LEAF, **kw)
    assert r["result"]["n_planes"] == 1 and r["result"]["stop_reason"] == 1 and r["stats"][0, 0] == 3 and (r["voxel_plane"] == 0).all()


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_listed_exported_and_struct_sizes(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esl.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+esl_dense_planes\s*\(", txt) and re.search(r"\}\s*esl_dense_plane_params\s*;", txt)
    assert re.search(r"\}\s*esl_dense_plane_result\s*;", txt)
    assert {"esl_dense_plane_params_default", "esl_dense_planes", "esl_debug_dense_planes_layout"} <= set(pkg.lib.EXPORTS)
    L = pkg.lib.load()
    assert hasattr(L, "esl_dense_planes")
    assert ctypes.sizeof(pkg.abi.EslDensePlaneParams) == 80 and ctypes.sizeof(pkg.abi.EslDensePlaneResult) == 32
    p = pkg.abi.EslDensePlaneParams()
    L.esl_dense_plane_params_default(ctypes.byref(p))          # host code: runs without a device
    d = pkg.abi.default_dense_plane_params()
    for k, _ in pkg.abi.EslDensePlaneParams._fields_:
        if k == "up":
            assert list(p.up) == list(d.up) == list(dpr.DEFAULTS["up"])
        elif k != "pad":
            assert getattr(p, k) == getattr(d, k) == dpr.DEFAULTS[k], k
    tile, group = pkg.Context.dense_planes_layout()
    assert tile >= 64 and group >= 64 and tile % 64 == 0 and group % 64 == 0
    assert callable(pkg.Context.dense_planes)


# ---- the header against hand-computed cases and the statement, bit for bit ----------------------------------------------------------------------
def bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def run(exe, mode, text):
    return subprocess.run([exe, mode], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan_ubsan"])
def test_planes_header_matches_the_statement(tmp_path, flags):
    exe = build_prog(tmp_path, "dense_planes_main", flags)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "dense_planes ok"
    rng = np.random.default_rng(8)
    # the sampler
    cases = [(int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 64)), int(rng.integers(1, 65537)), 0, int(rng.integers(0, 3)),
              int(rng.integers(1, 1 << 26))) for _ in range(200)]
    cases = [(s, r, H, int(rng.integers(0, H)), k, n) for s, r, H, _, k, n in cases] + [(0, 0, 64, 0, 0, 1000), ((1 << 64) - 1, 63, 65536, 65535, 2, 3)]
    out = run(exe, "sample", "".join("%d %d %d %d %d %d\n" % c for c in cases))
    assert out == ["%016x %d" % (dpr.mix(*c[:5]), dpr.index(*c)) for c in cases]
    # validity and the hypothesis plane: lattice triples at several scales, repeated indices, short baselines, collinear triples
    lines, want = [], []
    mb, leaf = 4, 0.01
    for t in range(400):
        sc_ = int(rng.choice([1, 3, 10, 1000, 300000]))
        a, b, c = (rng.integers(-sc_ * 3, sc_ * 3 + 1, 3) for _ in range(3))
        if t % 7 == 0:
            c = a + 3 * (b - a)          # collinear
        i = [int(x) for x in rng.integers(0, 50, 3)]
        if t % 11 == 0:
            i[2] = i[0]
        a, b, c = ([int(x) for x in v] for v in (a, b, c))
        pl = dpr.hypothesis(i, a, b, c, mb, leaf)
        lines.append(" ".join(str(x) for x in i + a + b + c))
        want.append("0 " + " ".join([bits(0.0)] * 4) if pl is None else "1 " + " ".join(bits(x) for x in pl))
    out = run(exe, "hyp", f"{mb} {leaf!r}\n" + "\n".join(lines) + "\n")
    assert out == want and 100 < sum(w[0] == "1" for w in want) < 400
    # the Jacobi: covariances of random voxel sets, flat ones and exactly diagonal ones included
    mats = []
    for t in range(120):
        k = rng.integers(-40, 40, (int(rng.integers(3, 80)), 3)) * rng.integers(1, 4, 3)
        if t % 3 == 0:
            k[:, 2] = k[:, 0] // 2 + rng.integers(0, 2, len(k))          # nearly flat
        if t % 10 == 0:
            k[:, 2] = 5
        C = np.cov(k.T.astype(np.float64), bias=True)
        mats.append([float(C[0, 0]), float(C[0, 1]), float(C[0, 2]), float(C[1, 1]), float(C[1, 2]), float(C[2, 2])])
    mats += [[3.0, 0.0, 0.0, 1.0, 0.0, 2.0], [2.0, 0.0, 0.0, 2.0, 0.0, 2.0], [1e-300, 1e-160, 0.0, 1.0, 0.0, 2.0], [0.0] * 6]
    out = run(exe, "jacobi", "".join(" ".join(repr(x) for x in m) + "\n" for m in mats))
    assert out == [" ".join(bits(x) for x in dpr.jacobi_min(m)) for m in mats]
    # the refit and the centroid from integer moments
    lines, want = [], []
    for t in range(80):
        k = (rng.integers(-3000, 3000, (int(rng.integers(3, 200)), 3)) // rng.integers(1, 50, 3)).astype(np.int64)
        cnt = rng.integers(1, 9, len(k))
        kmin = [int(x) - int(rng.integers(0, 5)) for x in k.min(axis=0)]          # the eligible box's kmin lies at or below the members'
        mom = dpr.moments(k, cnt, kmin)
        lines.append(" ".join(str(x) for x in kmin + mom))
        want.append(" ".join(bits(x) for x in dpr.refit(mom, kmin, 0.05) + dpr.centroid(mom, kmin, 0.05)))
    assert run(exe, "refit", "0.05\n" + "\n".join(lines) + "\n") == want
    # the orientation rules and the ground choice
    pls = [[float(x) for x in rng.normal(size=4)] for _ in range(30)] + [[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 0.5, 0.0], [-0.0, 0.0, -2.0, -0.0], [0.0] * 4,
                                                                        [1.0, 0.0, 0.0, -0.0]]
    assert run(exe, "orient", "".join(" ".join(repr(x) for x in p) + "\n" for p in pls)) == [" ".join(bits(x) for x in dpr.orient_out(p)) for p in pls]
    for t in range(30):
        n = int(rng.integers(0, 9))
        P = []
        for _ in range(n):
            v = rng.normal(size=3); v /= np.linalg.norm(v)
            P.append([float(x) for x in v] + [float(rng.normal())])
        n_in = [int(x) for x in rng.integers(1, 4, n) * 100]
        up = [float(x) for x in rng.normal(size=3)]
        cosv = float(rng.choice([0.0, 0.5, 0.7071067811865476, 0.95]))
        g, pl = dpr.ground(P, n_in, dpr.up_unit(up), cosv)
        text = " ".join(repr(x) for x in up) + f" {cosv!r} {n}\n" + "".join(" ".join(repr(x) for x in p) + f" {c}\n" for p, c in zip(P, n_in))
        assert run(exe, "ground", text) == [f"{g} " + " ".join(bits(x) for x in pl)]
    # step 5, the winner over a round's (valid, inlier voxels, inlier samples), and the rows of hyp_out it writes
    rounds = {"unique best": ([(1, 40, 90), (1, 70, 10), (1, 69, 500), (0, 0, 0)], 1),
              "samples break a tie on voxels": ([(1, 70, 10), (1, 12, 900), (1, 70, 11), (1, 70, 10)], 2),
              "the index breaks a full tie": ([(0, 70, 11), (1, 5, 5), (1, 70, 11), (1, 70, 11)], 2),
              "an invalid row holds the best numbers": ([(1, 3, 3), (0, 1 << 40, 1 << 50), (1, 4, 1), (1, 3, 9)], 2),
              "the only valid row is the last": ([(0, 9, 9), (0, 0, 0), (0, 7, 70), (1, 0, 0)], 3),
              "no valid row": ([(0, 9, 9), (0, 8, 8)], None)}
    text = "".join(f"{len(rows)}\n" + "".join("%d %d %d\n" % r for r in rows) for rows, _ in rounds.values())
    for (name, (rows, want)), line in zip(rounds.items(), run(exe, "winner", text)):
        assert dpr.winner(rows) == want, name
        assert [int(x) for x in line.split()] == [-1 if want is None else want] + [v for r in rows for v in r], name
    # step 6, the refit's acceptance at its three boundaries: more voxels, as many voxels with as many / fewer samples, fewer voxels
    cases = [(71, 0, 70, 11), (70, 11, 70, 11), (70, 12, 70, 11), (70, 10, 70, 11), (69, 1 << 40, 70, 11)]
    assert [dpr.refit_kept(*c) for c in cases] == [True, True, True, False, False]
    assert run(exe, "kept", "".join("%d %d %d %d\n" % c for c in cases)) == ["1", "1", "1", "0", "0"]
