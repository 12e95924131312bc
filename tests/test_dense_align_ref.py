"""The numpy statement of esl_dense_normals / esl_dense_align_frames (tests/dense_align_ref.py) on its own: analytic known answers, the
convergence on the box room, the premises every device scene of tests/test_gpu_dense_align.py relies on, and csrc/esl_dense_align.hpp
held to the statement on the host (plain and under AddressSanitizer + UBSan, as a stand-alone program: nothing is preloaded into
Python)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_align_ref as dar          # noqa: E402
import dense_align_scenes as s         # noqa: E402
import dense_planes_ref as dpr         # noqa: E402
import dense_ref as dr                 # noqa: E402
from dense_prog import BUILDS, BUILD_IDS, NONFINITE, build_prog, check_ladder          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(name, **kw):
    c = s.case(name)
    return dar.align(s.extract(c["map"]), s.scene(c["map"])["params"]["leaf"], s.scene(c["map"])["params"], c["cams"], c["K"], c["rows"],
                     c["cols"], c["depth"], **dict(c["params"], **kw))


def index_of(ext, key):
    return [list(k) for k in ext["key"].tolist()].index(list(key))


# ---- known answers: normals ----------------------------------------------------------------------------------------------------------------
def test_lattice_plane_normal():
    e = s.extract("plane")
    n = dar.normals(e)
    assert n["result"] == dict(status=0, n_voxels=81, n_eligible=81, n_valid=77)          # the four corners have 4 neighbours
    for i in range(81):
        kx, ky, _ = e["key"][i]
        inner = int(0 < kx < 8) + int(0 < ky < 8)
        assert n["neighbors"][i] == (9, 6, 4)[2 - inner]
        if inner == 2:
            assert n["normal"][i].tolist() == [0.0, 0.0, 1.0] and n["curvature"][i] == 0.0 and n["valid"][i] == 1
        if inner == 0:
            assert n["valid"][i] == 0 and n["normal"][i].tolist() == [0.0, 0.0, 0.0] and np.isnan(n["curvature"][i])
    # min_count 2: no voxel is eligible, none has a neighbour
    n2 = dar.normals(e, min_count=2)
    assert n2["result"]["n_eligible"] == 0 and (n2["neighbors"] == 0).all() and (n2["valid"] == 0).all() and np.isnan(n2["curvature"]).all()
    assert len(dar.normals(e, cap=10)["normal"]) == 10


def test_tilted_plane_normal():
    e = s.extract("tilted")
    assert e["n_voxels"] == 81 and e["xyz"].tolist() == sorted([list(p) for p in s.lattice_points("tilted")])          # the centroids are the samples
    n = dar.normals(e)
    want = np.array([1.0, 0.0, -2.0]) / math.sqrt(5.0)
    inner = [i for i in range(81) if 0 < e["key"][i][0] < 8 and 0 < e["key"][i][1] < 8]
    assert len(inner) == 49 and (n["neighbors"][inner] == 9).all() and (n["valid"][inner] == 1).all()
    assert np.abs(n["normal"][inner] - want).max() < 1e-12 and np.abs(n["curvature"][inner]).max() < 1e-12
    assert (n["normal"][inner][:, 0] > 0).all()          # the first non-zero component is positive


def test_edge_and_corner_are_invalid():
    n = dar.normals(s.extract("edge"))
    assert n["neighbors"].tolist() == [2, 2] and n["valid"].tolist() == [0, 0] and (n["normal"] == 0).all() and np.isnan(n["curvature"]).all()
    e = s.extract("corner")
    n = dar.normals(e)
    i = index_of(e, (0, 0, 0))
    assert n["neighbors"][i] == 7 and n["valid"][i] == 0 and np.isnan(n["curvature"][i])          # m is enough, the curvature is not
    C, tr = n["C"][i], n["trace"][i]
    w = np.array(dpr.jacobi_min(C))
    lam = w @ np.array([[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]]) @ w
    assert lam / tr > 0.05
    j = index_of(e, (2, 2, 0))          # inside a face
    assert n["valid"][j] == 1 and n["normal"][j].tolist() == [0.0, 0.0, 1.0] and n["neighbors"][j] == 9


def test_vectorised_jacobi_is_the_planes_jacobi():
    rng = np.random.default_rng(5)
    A = rng.normal(size=(200, 3, 3)); A = A @ A.transpose(0, 2, 1)
    C = np.stack([A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]], axis=-1)
    C[:50, 1] = 0.0; C[50:60, [1, 2, 4]] = 0.0          # skipped pivots, diagonal matrices
    got = dar.jacobi_min(C)
    for i in range(len(C)):
        assert got[i].tobytes() == np.array(dpr.jacobi_min(C[i])).tobytes(), i


# ---- known answers: a step ------------------------------------------------------------------------------------------------------------------
def three_planes(v):
    """samples on the lattice planes x = 1/2, y = 1/2, z = 1/2 (a 4 x 4 dyadic patch each), all moved by v; the camera centre at the origin"""
    g = [(a / 8, b / 8) for a in range(1, 5) for b in range(1, 5)]
    c = np.array([(0.5, a, b) for a, b in g] + [(a, 0.5, b) for a, b in g] + [(a, b, 0.5) for a, b in g])
    n = np.array([(1.0, 0, 0)] * 16 + [(0, 1.0, 0)] * 16 + [(0, 0, 1.0)] * 16)
    return c + np.asarray(v), c, n


def test_one_step_gives_back_the_shift():
    v = np.array([1 / 64, -1 / 128, 3 / 256])
    pw, c, n = three_planes(v)
    T = dar.terms(pw, [0.0, 0.0, 0.0], c, n)
    assert (T[:, 27] == np.rint((n * v).sum(axis=1) ** 2 * dar.FIX)).all()          # e = n . v, exact in the fixed point
    row = np.zeros(dar.ROW, np.int64); row[:28] = T.sum(axis=0); row[28] = row[36] = len(pw)
    H, g = dar.system(row)
    st, delta = dar.solve(H, g, len(pw), dict(dar.ALIGN_DEFAULTS, min_inliers=3))
    assert st == 0
    # every term is a dyadic number with fewer than 30 fractional bits, so the sums are exact and H delta = -g has the exact solution
    # (-v, 0); what is left is the double Cholesky of a well-conditioned 6 x 6: far below one fixed-point unit
    assert np.abs(np.array(delta) - np.concatenate([-v, np.zeros(3)])).max() <= 2.0 ** -30
    new = dar.update([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0], delta)          # an unnormalised identity
    assert np.abs(np.array(dar.centre(new)) + v).max() <= 2.0 ** -30 and np.abs(np.array(new[3:]) - [0, 0, 0, 1]).max() <= 2.0 ** -30


def test_one_plane_is_degenerate_and_few_are_too_few():
    pw, c, n = three_planes([0.0, 0.0, 1 / 64])
    T = dar.terms(pw[32:], [0.0, 0.0, 0.0], c[32:], n[32:])          # the plane z = 1/2 alone
    row = np.zeros(dar.ROW, np.int64); row[:28] = T.sum(axis=0)
    H, g = dar.system(row)
    assert dar.solve(H, g, 16, dict(dar.ALIGN_DEFAULTS, min_inliers=3)) == (dar.DEGENERATE, [0.0] * 6)
    assert dar.solve(H, g, 16, dar.ALIGN_DEFAULTS) == (dar.TOO_FEW, [0.0] * 6)          # min_inliers 100 is asked first


def test_tie_goes_to_the_smaller_key():
    # centroids at x = 1/4 (key 0) and x = 3/4 (key 1) with leaf 1/2; the sample at x = 1/2 is equidistant
    keys = dr.pack(np.array([[0, 0, 0], [1, 0, 0]]))
    xyz = np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25]])
    pw = np.array([[0.5, 0.25, 0.25], [0.5 + 2.0 ** -40, 0.25, 0.25]])
    best, d2 = dar.match(pw, np.array([[1, 0, 0], [1, 0, 0]]), keys, xyz, np.array([1, 1], np.uint8), 1)
    assert best.tolist() == [0, 1] and d2[0] == 0.0625
    best, _ = dar.match(pw, np.array([[1, 0, 0], [1, 0, 0]]), keys, xyz, np.array([0, 1], np.uint8), 1)          # an invalid voxel is no candidate
    assert best.tolist() == [1, 1]
    best, _ = dar.match(pw[:1], np.array([[1, 0, 0]]), keys, xyz, np.array([1, 1], np.uint8), 0)          # reach 0: the sample's own voxel
    assert best.tolist() == [1]
    best, _ = dar.match(pw[:1], np.array([[3, 0, 0]]), keys, xyz, np.array([1, 1], np.uint8), 1)
    assert best.tolist() == [-1]


def test_pose_update_is_a_rotation_about_the_centre():
    cam = s.views()["true"][0]
    new = dar.update(cam, [0.0, 0.0, 0.0, 0.0, 0.0, 0.01])
    assert np.abs(np.array(dar.centre(new)) - np.array(dar.centre(cam))).max() < 1e-15
    Ra, Rb = dr.pose(cam)[0], dr.pose(new)[0]
    W = Rb.T @ Ra          # R_wc_new R_wc^T = Exp(omega): a turn about the world's z by +0.01
    assert abs(math.atan2(W[1, 0], W[0, 0]) - 2 * math.atan(0.005)) < 1e-15 and abs(W[2, 2] - 1) < 1e-15


# ---- convergence on the box room ----------------------------------------------------------------------------------------------------------
def test_convergence_on_the_room():
    c = s.case("corner")
    assert (c["rows"], c["cols"]) == (120, 160) and s.LEAF == 0.05 and len(s.scene("room")["frames"]["cams"]) == 6
    e0 = dar.pose_error(c["cams"][0], c["true"][0])
    assert abs(e0[0] - 0.030) < 1e-4 and abs(e0[1] - 0.010) < 1e-4
    r = run("corner", iters=3)
    e3 = dar.pose_error(r["cams"][0], c["true"][0])
    print("start", e0, "after", int(r["iters"][0]), "steps", e3, "rms", math.sqrt(r["sum_e2"][0] / r["counts"][0, 7]))
    assert r["iters"][0] <= 3 and e3[0] * 10 <= e0[0] and e3[1] * 10 <= e0[1]
    assert math.sqrt(r["sum_e2"][0] / r["counts"][0, 7]) < 0.005


# ---- the premises of the device scenes ----------------------------------------------------------------------------------------------------
def test_room_premises():
    e = s.extract("room")
    n = dar.normals(e)
    assert 5000 < e["n_voxels"] < 20000 and n["result"]["n_valid"] > e["n_voxels"] // 2 and n["result"]["n_valid"] < e["n_voxels"]
    assert s.extract("removed")["n_voxels"] < e["n_voxels"] and s.scene("removed")["map"].status == 0
    wo = s.extract("without")
    assert wo["n_voxels"] == s.extract("removed")["n_voxels"] and wo["xyz"].tobytes() == s.extract("removed")["xyz"].tobytes()
    assert s.scene("full")["map"].status == 3
    r2 = dar.normals(e, radius=2, min_neighbors=12)
    assert 0 < r2["result"]["n_valid"] != n["result"]["n_valid"]


@pytest.mark.parametrize("name", s.CASES)
def test_case_premises(name):
    c = s.case(name)
    r = run(name)
    cnt = {k: r["counts"][0, i] for i, k in enumerate(dar.COUNTS)}
    print(name, r["result"], r["status"].tolist(), r["iters"].tolist(), r["counts"].tolist())
    assert r["status"][0] == dar.CONVERGED and cnt["n_inlier"] > 300 and cnt["n_nomatch"] > 0 and cnt["n_sampled"] == -(-c["rows"] // r_stride(c)) * -(-c["cols"] // r_stride(c))
    assert cnt["n_used"] == cnt["n_nomatch"] + cnt["n_far"] + cnt["n_inlier"] and r["sums"][0, 0, 28] == r["sums"][0, 0, 36]
    e1 = dar.pose_error(r["cams"][0], c["true"][0])
    assert e1[0] < 0.003 and e1[1] < 0.001
    if name == "far":
        assert (r["sums"][0, 0, 34:37] > 0).all()          # no match, far and inlier in the first pass
    if name == "small":
        assert cnt["n_sampled"] == 768
    if name == "small_odd":
        assert cnt["n_sampled"] == 713 and 713 % 64 and 713 % 256
    if name == "mixed":
        assert r["status"].tolist() == [dar.CONVERGED, dar.DEGENERATE, dar.TOO_FEW] and r["iters"].tolist()[1:] == [0, 0]
        assert r["counts"][1, 7] > 1000 and r["counts"][2, 1] == r["counts"][2, 0] and r["counts"][2, 7] == 0
        assert r["cams"][1:].tobytes() == c["cams"][1:].tobytes()          # a stopped frame keeps its pose
        alone = run("corner")
        for k in ("cams", "status", "iters", "counts", "sum_e2", "H", "step"):
            assert r[k][:1].tobytes() == alone[k].tobytes(), k
        assert (r["sums"][1, 1:] == 0).all() and (r["sums"][2, 1:] == 0).all()


def r_stride(c):
    return c["params"].get("stride", dar.ALIGN_DEFAULTS["stride"])


def test_removed_equals_the_map_without_the_frame():
    a, b = run("removed"), run("without")
    for k in ("cams", "status", "iters", "counts", "sum_e2", "H", "step", "sums"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["result"] == b["result"] and a["cams"].tobytes() != run("corner")["cams"].tobytes()


def test_refusals_of_the_statement():
    c = s.case("corner")
    assert dar.align(s.extract("full"), s.PLEAF, s.scene("full")["params"], c["cams"], c["K"], 120, 160, c["depth"]) == dict(
        result=dict(status=3, n_voxels=-1, n_valid=0, n_passes=0))
    with pytest.raises(dr.InvalidPose):
        dar.align(s.extract("room"), s.LEAF, s.MAP_PARAMS, [[0.0] * 7], c["K"], 120, 160, c["depth"])
    # the bound of step c: 16384 x 16384 pixels at 6 m reach 2^62, 120 x 160 do not
    Q = dar.bound(c["K"], 120, 160, 6.0, 0.01)
    assert 6.0 < Q < 12.0 and dar.sums_fit(4800, Q) and not dar.sums_fit(16384 * 16384, dar.bound(c["K"], 16384, 16384, 6.0, 0.01))
    r0 = run("corner", iters=0)
    assert r0["result"]["n_passes"] == 1 and r0["status"].tolist() == [0] and r0["cams"].tobytes() == c["cams"].tobytes() and r0["counts"][0, 7] > 0


# ---- the header against the statement -----------------------------------------------------------------------------------------------------
def bits(x):
    return [str(int(b)) for b in np.asarray(x, dtype=np.float64).reshape(-1).view(np.uint64)]


def call(exe, mode, lines):
    out = subprocess.run([exe, mode], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[-1] == ""
    return out[:-1]


def neighbour_lists(ext, reach, eligible):
    """per voxel the indices of its neighbours in visit order"""
    n = ext["n_voxels"]
    key = np.asarray(ext["key"], dtype=np.int64).reshape(n, 3)
    packed = dr.pack(key)
    cols = [dar.lookup(packed, key + np.asarray(off, dtype=np.int64)) for off in dar.offsets(reach)]
    J = np.stack(cols, axis=-1)
    return [[int(j) for j in J[i] if j >= 0 and eligible[j]] if eligible[i] else [] for i in range(n)]


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan_ubsan"])
def test_align_header_matches_the_statement(tmp_path, flags):
    exe = build_prog(tmp_path, "dense_align_main", flags)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "dense_align ok"
    # the normals: the moments in visit order, the Jacobi, the orientation, the curvature and the gates
    n_valid = n_invalid = 0
    for name, radius, min_nb, step in (("plane", 1, 5, 1), ("tilted", 1, 5, 1), ("corner", 1, 5, 1), ("edge", 1, 5, 1), ("room", 1, 5, 3), ("room", 2, 12, 7)):
        ext = s.extract(name)
        ref = dar.normals(ext, radius=radius, min_neighbors=min_nb)
        nb = neighbour_lists(ext, radius, np.ones(ext["n_voxels"], bool))
        pick = list(range(0, ext["n_voxels"], step))
        lines = [f"{len(pick)} {min_nb} {bits(0.05)[0]}"]
        for i in pick:
            lines.append(f"{len(nb[i])} " + " ".join(bits(ext["xyz"][i])))
            lines += [" ".join(bits(ext["xyz"][j])) for j in nb[i]]
        out = call(exe, "normal", lines)
        assert len(out) == len(pick)
        for i, got in zip(pick, out):
            g = got.split()
            assert g[:2] == [str(int(ref["neighbors"][i])), str(int(ref["valid"][i]))] and g[2:5] == bits(ref["normal"][i]), (name, radius, i)
            if ref["valid"][i]:
                n_valid += 1
                assert g[5] == bits(ref["curvature"][i])[0], (name, radius, i)
            else:
                n_invalid += 1
                assert np.isnan(np.array([int(g[5])], np.uint64).view(np.float64)[0]) and np.isnan(ref["curvature"][i])
    assert n_valid > 3000 and n_invalid > 100
    # the match, the terms and the step, pass after pass
    n_steps = {0: 0, dar.TOO_FEW: 0, dar.DEGENERATE: 0}
    for name, over in (("corner", {}), ("corner", dict(damping=0.5, reach=2)), ("far", {}), ("one_wall", {}), ("empty", {}), ("small_odd", {})):
        c = s.case(name)
        p = dict(dar.ALIGN_DEFAULTS, **{k: v for k, v in dict(c["params"], **over).items() if k in dar.ALIGN_DEFAULTS})
        ext, mp = s.extract(c["map"]), dict(dr.DEFAULTS, **s.scene(c["map"])["params"])
        nrm = dar.normals(ext)
        cam = [float(x) for x in c["cams"][0]]
        keys = dr.pack(np.asarray(ext["key"], dtype=np.int64))
        for _ in range(3):
            row, det = dar.accumulate(ext, nrm, s.LEAF, mp, cam, c["K"], c["rows"], c["cols"], c["depth"][0], p, detail=True)
            sm = det["samples"]
            pick = list(range(0, len(sm["pw"]), 5))
            cand = np.stack([dar.lookup(keys, sm["k"] + np.asarray(off, dtype=np.int64)) for off in dar.offsets(p["reach"])], axis=-1) if len(sm["pw"]) else None
            lines = [str(len(pick))]
            lists = []
            for i in pick:
                lst = [int(j) for j in cand[i] if j >= 0 and nrm["valid"][j]]
                lists.append(lst)
                lines.append(f"{len(lst)} " + " ".join(bits(sm["pw"][i])))
                lines += [" ".join(bits(ext["xyz"][j])) for j in lst]
            out = call(exe, "match", lines)
            for i, lst, got in zip(pick, lists, out):
                b, d2 = got.split()
                assert (lst[int(b)] if int(b) >= 0 else -1) == det["best"][i] and (int(b) < 0 or d2 == bits(det["d2"][i])[0]), (name, i)
            inl = np.flatnonzero(det["inlier"])
            o = dar.centre(cam)
            lines = [f"{len(inl)} " + " ".join(bits(o))]
            lines += [" ".join(bits(sm["pw"][i]) + bits(ext["xyz"][det["best"][i]]) + bits(nrm["normal"][det["best"][i]])) for i in inl]
            out = call(exe, "terms", lines)
            assert [[int(x) for x in ln.split()] for ln in out] == det["terms"].tolist(), name
            H, g = dar.system(row)
            st, delta = dar.solve(H, g, int(row[36]), p)
            nxt = dar.update(cam, delta)
            line = " ".join([str(int(x)) for x in row[:28]] + [str(int(row[36])), str(p["min_inliers"])] + bits(p["damping"]) + bits(p["min_pivot_ratio"]) + bits(cam))
            got = call(exe, "step", ["1", line])[0].split()
            conv = dar.norm3(delta[:3]) <= 1e-5 and dar.norm3(delta[3:]) <= 1e-5
            want = ([str(st)] + bits(H) + bits(g) + bits(delta) + ["1"] + bits(nxt) + bits(dar.norm3(delta[:3])) + bits(dar.norm3(delta[3:]))
                    + [str(int(conv))])
            assert got == want, (name, st)
            n_steps[st] += 1
            if st != 0:
                break
            cam = nxt
    assert n_steps[0] >= 9 and n_steps[dar.TOO_FEW] == 1 and n_steps[dar.DEGENERATE] == 1


# ---- what esl_dense_normals and esl_dense_align_frames refuse for their parameters (csrc/esl_dense_check.hpp), text by text and in order ----
TINY = 5e-324          # the smallest positive double: the first value above 0, its negative the first below
NORMAL_RUNGS = [
    ("max_curvature not finite or negative", [dict(max_curvature=0.0)], [dict(max_curvature=-TINY)] + [dict(max_curvature=v) for v in NONFINITE]),
    ("radius outside 1 .. 2", [dict(radius=1), dict(radius=2)], [dict(radius=0), dict(radius=3)]),
    ("min_count < 1", [dict(min_count=1)], [dict(min_count=0)]),
    ("min_neighbors < 1", [dict(min_neighbors=1)], [dict(min_neighbors=0)]),
]


@pytest.mark.parametrize("flags", BUILDS, ids=BUILD_IDS)
def test_align_params_check_texts_and_order(tmp_path, flags):
    """dal_params_check, and dnr_params_check which ends it and which esl_dense_normals calls alone: every rung at its last accepted and
    first refused value, NaN and the infinities in every double, and the earlier rung's text when two fail."""
    exe = build_prog(tmp_path, "dense_align_main", flags)
    normals = dict(max_curvature=0.05, radius=1, min_count=1, min_neighbors=5)
    defaults = dict(max_dist=0.0, damping=0.0, min_pivot_ratio=1e-6, tol_t=1e-5, tol_r=1e-5, iters=4, stride=2, reach=1, min_inliers=100, **normals)
    rungs = [
        ("max_dist not finite or negative", [dict(max_dist=0.0)], [dict(max_dist=-TINY)] + [dict(max_dist=v) for v in NONFINITE]),
        ("damping not finite or negative", [dict(damping=0.0)], [dict(damping=-TINY)] + [dict(damping=v) for v in NONFINITE]),
        ("min_pivot_ratio not finite or negative", [dict(min_pivot_ratio=0.0)], [dict(min_pivot_ratio=-TINY)] + [dict(min_pivot_ratio=v) for v in NONFINITE]),
        ("tol_t not finite or negative", [dict(tol_t=0.0)], [dict(tol_t=-TINY)] + [dict(tol_t=v) for v in NONFINITE]),
        ("tol_r not finite or negative", [dict(tol_r=0.0)], [dict(tol_r=-TINY)] + [dict(tol_r=v) for v in NONFINITE]),
        ("iters outside 0 .. 64", [dict(iters=0), dict(iters=64)], [dict(iters=-1), dict(iters=65)]),
        ("stride < 1", [dict(stride=1)], [dict(stride=0)]),
        ("reach outside 0 .. 2", [dict(reach=0), dict(reach=2)], [dict(reach=-1), dict(reach=3)]),
        ("min_inliers < 1", [dict(min_inliers=1)], [dict(min_inliers=0)]),
    ] + NORMAL_RUNGS
    nfields = ["max_curvature", "radius", "min_count", "min_neighbors"]
    fields = ["max_dist", "damping", "min_pivot_ratio", "tol_t", "tol_r", "iters", "stride", "reach", "min_inliers"] + nfields
    check_ladder(exe, fields, defaults, rungs)
    check_ladder(exe, nfields, normals, NORMAL_RUNGS, mode="check_normals")
