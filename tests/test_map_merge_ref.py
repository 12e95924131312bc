"""esl_map_overlaps / esl_map_merge without a device: the lattice estimator of the numpy statement (tests/map_merge_ref.py) against
closed forms and against a dense lattice, N_ball, the planted-duplicates scene, a hand-made edge list with conflicts, the permutation
property, csrc/esl_merge_lattice.hpp in a stand-alone program (plain and under AddressSanitizer / UBSan) against the Python statement,
and the exported symbols."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_merge_ref as mr          # noqa: E402
import map_merge_scenes as sc       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the lattice --------------------------------------------------------------------------------------------------------------------------------
def test_n_ball():
    assert [mr.n_ball(n) for n in (4, 8, 16, 32)] == [32, 280, 2176, 17256]
    assert mr.n_ball(16) == 34 * 64
    for n in range(4, 33):          # no triple on the sphere, for any n
        k = mr.lattice(n)
        assert not ((k * k).sum(1) == n * n).any()
        assert np.array_equal(k, -k[::-1])          # the lexicographic order is point-symmetric


def build_lattice_prog(tmp, flags):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/merge_lattice_main.cpp"
    exe = str(tmp / "merge_lattice_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", *flags, "-o", exe, os.path.join(ROOT, "tests", "merge_lattice_main.cpp")])
    return exe


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan_ubsan"])
def test_lattice_header_matches_python(tmp_path, flags):
    exe = build_lattice_prog(tmp_path, flags)
    ns = [4, 5, 7, 8, 9, 16, 31, 32]
    keys = [(0, 0), (0, 65535), (1, 0), (2 ** 31 - 1, 0), (2 ** 31 - 1, 65535), (7, 12), (7, 13), (8, 12)]
    text = f"{len(ns)}\n" + " ".join(map(str, ns)) + f"\n{len(keys)}\n" + "".join(f"{w} {i}\n" for w, i in keys)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    want = []
    for n in ns:
        p, inside = mr.lattice_cells(n)
        want.append(f"count {n} {mr.n_ball(n)}")
        for t, (c, inb) in enumerate(zip(p, inside)):
            k = 2 * c + 1 - n
            want.append(f"cell {n} {t} {c[0]} {c[1]} {c[2]} {k[0]} {k[1]} {k[2]} {int(inb)}")
        rounds = (n ** 3 + 63) // 64
        for lane in range(64):      # the walk of a lane: the cells lane, lane + 64, ...
            ts = [lane + 64 * it if lane + 64 * it < n ** 3 else -1 for it in range(rounds)]
            want.append(f"walk {n} {lane} " + " ".join(map(str, ts)))
    for w, i in keys:
        ck, rk = ((2 ** 31 - 1 - w) << 32) | i, (w << 32) | (2 ** 31 - 1 - i)
        want.append(f"key {w} {i} {ck} {rk} {i} {i}")
    assert r.stdout.splitlines() == want
    # the keys order as step 6 and step 7 say: smaller conflict key = larger weight, then lower index; larger representative key likewise
    conflict = sorted(keys, key=lambda k: ((2 ** 31 - 1 - k[0]) << 32) | k[1])
    assert conflict == sorted(keys, key=lambda k: (-k[0], k[1]))
    rep = sorted(keys, key=lambda k: -((k[0] << 32) | (2 ** 31 - 1 - k[1])))
    assert rep == conflict


# ---- the estimator against closed forms -------------------------------------------------------------------------------------------------------------
def test_two_spheres_against_the_lens_formula():
    worst = 0.0
    for r1, r2, d in ((1.0, 1.0, 0.52), (1.0, 1.0, 1.04), (0.5, 0.8, 0.7), (0.3, 0.9, 0.75), (1.0, 0.6, 1.37)):
        pair = np.stack([sc.sphere([0.11, -0.2, 0.3], r1), sc.sphere(np.array([0.11, -0.2, 0.3]) + d * np.array([0.6, 0.48, 0.64]), r2)])
        iou, con = sc.pair_iou(pair, 16)
        want_iou, want_con = sc.sphere_lens_iou(r1, r2, d)
        worst = max(worst, abs(iou - want_iou))
        assert abs(iou - want_iou) <= 2 * sc.IOU_ERR_N16 and abs(con - want_con) <= 0.05, (r1, r2, d, iou, want_iou, con, want_con)
    assert worst > 0          # an estimate, not the formula restated


def test_nested_and_disjoint():
    big = sc.ell([0.3, 0.1, -0.2], [0.9, 0.7, 0.8], yaw=0.4)
    small = sc.ell([0.3, 0.1, -0.2], [0.45, 0.35, 0.4], yaw=0.4)
    ov = mr.overlaps(np.stack([big, small]), [0, 0])
    nb = mr.n_ball(16)
    assert ov["n_pairs"] == 1 and ov["counts"][0, 1] == nb         # every sample of the small one lies in the large one
    assert ov["contain"][0] <= 1.0
    # concentric, same axes, half the size: V_small / V_large = 1/8; the estimate of the intersection is the mean of two estimates of it
    assert abs(ov["iou"][0] - 0.125) <= 2 * sc.IOU_ERR_N16 and ov["contain"][0] >= 1 - 8 * 2 * sc.IOU_ERR_N16
    ov = mr.overlaps(np.stack([big, small]), [0, 0], lattice=32)
    assert abs(ov["iou"][0] - 0.125) <= sc.IOU_ERR_N16
    far = sc.ell([3.0, 0.1, -0.2], [0.9, 0.7, 0.8])
    ov = mr.overlaps(np.stack([big, far]), [0, 0])
    assert ov["n_candidates"] == 0 and ov["n_pairs"] == 0
    # bounding spheres meet, bodies do not: a candidate, not an overlapping pair
    flat_a, flat_b = sc.ell([0, 0, 0], [0.9, 0.9, 0.1]), sc.ell([0, 0, 0.8], [0.9, 0.9, 0.1])
    ov = mr.overlaps(np.stack([flat_a, flat_b]), [0, 0])
    assert ov["n_candidates"] == 1 and ov["n_pairs"] == 0
    # an exact copy
    ov = mr.overlaps(np.stack([big, big]), [0, 0])
    assert list(ov["counts"][0]) == [nb, nb] and abs(ov["iou"][0] - 1) <= sc.TOL and ov["contain"][0] == 1.0


def test_lattice_16_against_64():
    """the named constant of map_merge_scenes.py is what this measures; asserted against twice the constant"""
    worst = 0.0
    pairs = sc.estimator_pairs()
    assert len(pairs) == 300
    for pr in pairs:
        a, b = sc.pair_iou(pr, 16), sc.pair_iou(pr, 64)
        worst = max(worst, abs(a[0] - b[0]))
    print(f"largest |iou(16) - iou(64)| over {len(pairs)} pairs: {worst:.5f}")
    assert worst <= 2 * sc.IOU_ERR_N16
    assert worst >= 0.5 * sc.IOU_ERR_N16, "the constant no longer states what is measured"


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------
def test_planted_duplicates_are_recovered_exactly():
    s = sc.planted_scene()
    assert len(s["objs"]) == sc.N_PLANTED + sc.N_COPIES
    for over in (dict(), dict(match_labels=0)):
        r = mr.merge(s["objs"], s["labels"], None, s["obs_cam"], s["obs_obj"], **over)
        sc.check_conditions(r["overlaps"])
        assert np.array_equal(r["group"], s["group"])                     # exactly the planted groups, no false one
        res = r["result"]
        assert (res["status"], res["n_groups"], res["n_merged_groups"], res["largest_group"]) == (0, sc.N_PLANTED, sc.N_COPIES, 2)
        assert res["n_conflicts"] == 2 * sc.N_COPIES and res["n_links"] == sc.N_COPIES and res["n_pairs"] > res["n_links"]
        # the thresholds stand at least ten times the estimator's error away from every pair, planted or not
        ov, p = r["overlaps"], r["overlaps"]["params"]
        planted = np.array([s["group"][i] == s["group"][j] for i, j in ov["pairs"]])
        assert ov["iou"][planted].min() >= p["min_iou"] + 10 * sc.IOU_ERR_N16
        assert ov["iou"][~planted].max() <= p["min_iou"] - 10 * sc.IOU_ERR_N16
        assert ov["contain"][~planted].max() <= p["min_contain"] - 10 * sc.IOU_ERR_N16
        # every surviving entry points at the merged object of its original, one entry per (frame, object)
        out = r["obs_obj"]
        live = out >= 0
        assert np.array_equal(out[live], r["new_index"][s["obs_obj"][live]])
        pairs = list(zip(s["obs_cam"][live], out[live]))
        assert len(pairs) == len(set(pairs)) and (out[s["obs_obj"] < 0] == -1).all()
        assert r["weights"].sum() == (s["obs_obj"] >= 0).sum()


def test_hand_made_list_with_conflicts():
    a = sc.ell([0, 0, 0], [0.5, 0.4, 0.3], yaw=0.2)
    b = sc.ell([0.01, 0, 0], [0.5, 0.4, 0.3], yaw=0.25)
    c = sc.ell([5, 0, 0], [0.5, 0.4, 0.3])
    objs, labels = np.stack([a, c, b]), np.array([4, 4, 4], np.int32)          # 0 ~ 2, 1 alone
    cam = np.array([0, 0, 1, 1, 2, 2, 2, 3, 3, 0], np.int32)
    obj = np.array([0, 2, 2, 1, 2, 2, 0, -1, 1, 1], np.int32)
    # weights from the list: object 0: 2 entries, 1: 3, 2: 4 -> the representative of {0, 2} is 2
    r = mr.merge(objs, labels, None, cam, obj)
    assert list(r["group"]) == [0, 1, 0] and list(r["new_index"]) == [0, 1, 0]
    assert r["objs"][0].tobytes() == b.tobytes() and r["objs"][1].tobytes() == c.tobytes()
    assert list(r["weights"]) == [6, 3] and list(r["labels"]) == [4, 4]
    # frame 0: entries 0 (object 0, weight 2) and 1 (object 2, weight 4) -> entry 1; frame 2: entries 4, 5 (object 2), 6 (object 0) -> 4
    assert list(r["obs_obj"]) == [-1, 0, 0, 1, 0, -1, -1, -1, 1, 1]
    assert r["result"]["n_conflicts"] == 3
    # equal weights: the lower original index wins
    r = mr.merge(objs, labels, [5, 1, 5], cam, obj)
    assert r["objs"][0].tobytes() == a.tobytes() and list(r["weights"]) == [10, 1]
    assert list(r["obs_obj"]) == [0, -1, 0, 1, -1, -1, 0, -1, 1, 1]
    # no list: every weight 1
    r = mr.merge(objs, labels)
    assert list(r["weights"]) == [2, 1] and r["obs_obj"] is None and r["objs"][0].tobytes() == a.tobytes()


def test_permuting_the_map_permutes_the_groups():
    s = sc.clutter_scene(1)
    M = len(s["objs"])
    base = mr.merge(s["objs"], s["labels"], s["weights"], s["obs_cam"], s["obs_obj"])
    assert base["result"]["n_merged_groups"] > 0
    perm = np.random.default_rng(5).permutation(M)          # new position k holds old object perm[k]
    inv = np.argsort(perm)
    obs = np.where(s["obs_obj"] >= 0, inv[np.maximum(s["obs_obj"], 0)], -1)
    r = mr.merge(s["objs"][perm], s["labels"][perm], s["weights"][perm], s["obs_cam"], obs)
    same_base = base["group"][:, None] == base["group"][None, :]
    same_perm = r["group"][inv][:, None] == r["group"][inv][None, :]
    assert np.array_equal(same_base, same_perm)
    for k in ("n_valid", "n_groups", "n_merged_groups", "largest_group", "n_candidates", "n_pairs", "n_links"):
        assert r["result"][k] == base["result"][k], k
    assert sorted(r["weights"]) == sorted(base["weights"])


def test_chains_and_invalid_ellipsoids():
    r = mr.merge(sc.chain(3), np.zeros(3, np.int32))
    ov = r["overlaps"]
    assert [tuple(p) for p in ov["pairs"]] == [(0, 1), (0, 2), (1, 2)] and list(ov["link"]) == [True, False, True]
    assert list(r["group"]) == [0, 0, 0]
    r = mr.merge(sc.chain(33), np.zeros(33, np.int32))
    assert r["result"]["n_groups"] == 1 and r["result"]["largest_group"] == 33 and r["result"]["n_links"] == 32
    objs = sc.chain(4, spacing=0.1)
    objs[1, 4] = np.nan
    objs[2, 7] = -1.0          # a negative half-axis counts by its absolute value
    objs[3, 3:7] *= 3.0        # an unnormalised quaternion is normalised
    r = mr.merge(objs, np.zeros(4, np.int32))
    assert list(r["overlaps"]["valid"]) == [True, False, True, True] and list(r["group"]) == [0, 1, 0, 0]
    assert r["objs"][1].tobytes() == objs[1].tobytes()


# ---- the symbols --------------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_listed_exported_and_struct_sizes(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esl.h")).read(), flags=re.S)
    for name in ("esl_map_overlaps", "esl_map_merge"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt)
    assert re.search(r"\}\s*esl_merge_params\s*;", txt) and re.search(r"\}\s*esl_merge_result\s*;", txt)
    assert {"esl_merge_params_default", "esl_map_overlaps", "esl_map_merge"} <= set(pkg.lib.EXPORTS)
    L = pkg.lib.load()
    assert ctypes.sizeof(pkg.abi.EslMergeParams) == 32 and ctypes.sizeof(pkg.abi.EslMergeResult) == 48
    p = pkg.abi.EslMergeParams()
    L.esl_merge_params_default(ctypes.byref(p))          # host code: runs without a device
    d = pkg.abi.default_merge_params()
    for k, _ in pkg.abi.EslMergeParams._fields_:
        assert getattr(p, k) == getattr(d, k) == mr.DEFAULTS[k], k
    assert L.esl_abi_version() == 5
