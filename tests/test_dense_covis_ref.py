"""The numpy statement of esl_dense_covis_frames (tests/dense_covis_ref.py) on its own: the premises every device scene of
tests/test_gpu_dense_covis.py relies on, the hand-made scene's literals, and csrc/esl_dense_covis.hpp held to the statement on the
host (plain and under AddressSanitizer + UBSan, as a stand-alone program: nothing is preloaded into Python).

The statement's numbers on `ghost` (48 x 64, leaf 0.05, its six views, defaults: window 1, min_others 3, 9 / 10): 7376 voxels;
seen 4010, 4725, 4093, 4836, 3755, 5537; pair[0][1] = 3479; voxels by k = 0 .. 6: 0, 1245, 1356, 1071, 621, 1196, 1887; covered
3579, 3396, 3088, 3348, 3133, 3242; unique 0, 21, 362, 228, 29, 605; no frame redundant at 9 / 10."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_carve_scenes as cs        # noqa: E402
import dense_covis_ref as dco          # noqa: E402
import dense_covis_scenes as vs        # noqa: E402
from dense_prog import BUILDS, BUILD_IDS, NONFINITE, build_prog, check_ladder          # noqa: E402
from test_dense_carve_ref import GATE_RUNGS          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(sc, m, frames=None, keep=None, **kw):
    f = list(range(len(sc["cams"]))) if frames is None else list(frames)
    return dco.covis(m, sc["cams"][f], sc["depth"][f], sc["K"], sc["rows"], sc["cols"], keep=keep, **kw)


def identities(r):
    k = r["vox"].astype(np.int64)
    assert r["result"]["sum_seen"] == int(k.sum()) == int(r["frame"][:, 3].sum())
    assert r["result"]["sum_pairs"] == int((k * (k - 1) // 2).sum())
    assert np.array_equal(np.diag(r["pair"]), r["frame"][:, 3]) and np.array_equal(r["pair"], r["pair"].T)
    assert (r["frame"][:, :3].sum(axis=1) == r["result"]["n_voxels"]).all() and (r["frame"][:, 7] == 0).all()
    assert (r["frame"][:, 3] <= r["frame"][:, 0]).all() and (r["frame"][:, 4] <= r["frame"][:, 3]).all()
    assert r["result"]["n_seen"] == int((k >= 1).sum()) and r["result"]["n_culled"] == int((r["frame"][:, 6] >= 0).sum())


def test_ghost_numbers():
    sc = cs.ghost_scene("ghost")
    r = run(sc, cs.build(sc))
    identities(r)
    assert r["result"]["n_voxels"] == 7376
    assert r["frame"][:, 3].tolist() == [4010, 4725, 4093, 4836, 3755, 5537] and r["pair"][0][1] == 3479
    assert np.bincount(r["vox"], minlength=7).tolist() == [0, 1245, 1356, 1071, 621, 1196, 1887]
    assert r["frame"][:, 4].tolist() == [3579, 3396, 3088, 3348, 3133, 3242] and r["frame"][:, 5].tolist() == [0, 21, 362, 228, 29, 605]
    assert not any(dco.redundant(s, c, 9, 10) for s, c in zip(r["frame"][:, 3].tolist(), r["frame"][:, 4].tolist()))
    assert run(sc, cs.build(sc), max_cull=6)["order"] == [] and (r["frame"][:, 6] == -1).all()
    assert (7376 + 63) // 64 == 116          # the words of a row: they cross the pair kernel's slab of 64


CULLS = [          # (params, protected frames, the order of leaving as (frame, uncovered))
    (dict(min_others=3, cover_num=4, cover_den=5), (), [(0, 431)]),
    (dict(min_others=1, cover_num=4, cover_den=5), (), [(0, 0), (1, 21), (4, 122), (3, 256)]),
    (dict(min_others=1, cover_num=4, cover_den=5), (0,), [(1, 21), (4, 98), (3, 242), (2, 594)]),
    (dict(min_others=2, cover_num=7, cover_den=10), (), [(0, 50), (4, 377), (1, 1141)]),
]


@pytest.mark.parametrize("case", range(len(CULLS)))
def test_ghost_cull_orders(case):
    p, prot, order = CULLS[case]
    sc = cs.ghost_scene("ghost")
    keep = np.array([f in prot for f in range(6)], np.uint8) if prot else None
    r = run(sc, cs.build(sc), keep=keep, max_cull=6, **p)
    identities(r)
    assert r["order"] == order and r["result"]["n_culled"] == len(order)
    want = [-1] * 6
    for i, (f, _) in enumerate(order):
        want[f] = i
    assert r["frame"][:, 6].tolist() == want
    # the run stopped before max_cull: no alive unprotected frame is redundant under the alive frames' counts
    alive = [f for f in range(6) if want[f] < 0]
    k = r["B"][alive].sum(axis=0)
    for f in alive:
        cov = int((r["B"][f] & (k - 1 >= p["min_others"])).sum())
        assert (f in prot) or not dco.redundant(int(r["B"][f].sum()), cov, p["cover_num"], p["cover_den"])
    # max_cull below the number of candidates: the order's prefix
    short = run(sc, cs.build(sc), keep=keep, max_cull=1, **p)
    assert short["order"] == order[:1] and np.array_equal(short["pair"], r["pair"]) and np.array_equal(short["vox"], r["vox"])


@pytest.mark.parametrize("name", vs.ROOMS)
def test_identities_and_full_cover(name):
    sc = vs.scene(name)
    m = cs.build(sc)
    r = run(sc, m)
    identities(r)
    assert r["result"]["n_seen"] > 1000
    # at 1 / 1 a frame leaves only when every voxel it sees stays covered: each voxel keeps min(k_i, min_others) alive observers
    for mo in (1, 2):
        c = run(sc, m, max_cull=len(sc["cams"]), min_others=mo, cover_num=1, cover_den=1)
        identities(c)
        alive = c["frame"][:, 6] < 0
        k_left = c["B"][alive].sum(axis=0)
        assert (k_left >= np.minimum(c["vox"], mo)).all()
        for r_ in range(c["result"]["n_culled"]):          # and after any number of rounds
            k_r = c["B"][(c["frame"][:, 6] < 0) | (c["frame"][:, 6] > r_)].sum(axis=0)
            assert (k_r >= np.minimum(c["vox"], mo)).all()


def test_away_views_share_nothing_with_some():
    sc = vs.away()
    r = run(sc, cs.build(sc))
    identities(r)
    zero = [(a, b) for a in range(9) for b in range(a + 1, 9) if r["pair"][a][b] == 0]
    print("away: seen", r["frame"][:, 3].tolist(), "zero pairs", zero)
    assert len(zero) >= 2 and all(b >= 6 for _, b in zero) and (r["frame"][:, 3] > 500).all()
    assert r["result"]["n_voxels"] % 64 and (r["pair"][6:, 6:] > 0).all()


def test_hand_scene():
    h = vs.hand()
    m = cs.build(h["map"])
    r = dco.covis(m, h["cams"], h["depth"], h["K"], h["rows"], h["cols"], **h["params"])
    identities(r)
    o = vs.hand_order(m)
    assert r["B"][:, o].astype(int).tolist() == vs.HAND_B and r["vox"][o].tolist() == vs.HAND_K_COUNT
    assert r["pair"].tolist() == vs.HAND_PAIR and r["frame"].tolist() == vs.HAND_FRAME
    assert r["result"] == dict(status=0, n_voxels=3, n_seen=3, n_culled=0, sum_seen=7, sum_pairs=5)
    # 1 / 2 of what a frame sees covered by two others: frames 0 and 1 qualify (1 of 2), frame 2 does not (1 of 3); 0 leaves first, then
    # the middle voxel has k = 2 and nothing is covered any more
    c = dco.covis(m, h["cams"], h["depth"], h["K"], h["rows"], h["cols"], max_cull=4, cover_num=1, cover_den=2, **h["params"])
    assert c["order"] == [(0, 1)] and c["frame"][:, 6].tolist() == [0, -1, -1, -1]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_point_rows(n):
    e = vs.points(n)
    m = cs.build(e["map"])
    r = dco.covis(m, e["cams"], e["depth"], e["K"], e["rows"], e["cols"], **e["params"])
    identities(r)
    assert r["result"]["n_voxels"] == n and np.array_equal(r["B"], e["B"])          # voxel j is bit j: the tail of the last word is known
    assert r["frame"][:, 0].tolist() == [n, n, n]


def test_cycled_duplicates():
    sc = cs.ghost_scene("ghost_odd")
    cams, depth = vs.cycled(sc, 19)
    r = dco.covis(cs.build(sc), cams, depth, sc["K"], sc["rows"], sc["cols"])
    identities(r)
    for j in range(6, 12):          # an exact duplicate pair: every voxel one of them sees, both see
        assert r["pair"][j][j - 6] == r["frame"][j, 3] == r["frame"][j - 6, 3] and np.array_equal(cams[j], cams[j - 6])
    assert not np.array_equal(cams[12], cams[0]) and r["pair"][12][0] < r["frame"][0, 3] and (r["frame"][:, 5] == 0).all()


def test_invalid_map_and_pose():
    sc = cs.full_scene()
    m = cs.build(sc)
    assert m.status == 3
    h = vs.hand()
    r = dco.covis(m, h["cams"], h["depth"], h["K"], 1, 3)
    assert r == dict(result=dict(status=3, n_voxels=-1, n_seen=0, n_culled=0, sum_seen=0, sum_pairs=0))
    import dense_ref as dr
    with pytest.raises(dr.InvalidPose):
        dco.covis(cs.build(h["map"]), [[0, 0, 0, 0, 0, 0, 0]], h["depth"][:1], h["K"], 1, 3)
    empty = dco.covis(cs.build(h["map"], frames=[]), h["cams"], h["depth"], h["K"], 1, 3, max_cull=3)
    assert empty["result"] == dict(status=0, n_voxels=0, n_seen=0, n_culled=0, sum_seen=0, sum_pairs=0) and (empty["pair"] == 0).all()
    none = dco.covis(cs.build(h["map"]), np.zeros((0, 7)), np.zeros((0, 1, 3), np.uint16), h["K"], 1, 3)
    assert none["pair"].shape == (0, 0) and none["vox"].tolist() == [0, 0, 0] and none["frame"].shape == (0, 8)


# ---- the header against the statement -----------------------------------------------------------------------------------------------------
def words_of(B):
    """the rows of the boolean matrix as 64-bit words: bit i % 64 of word i / 64 = column i"""
    F, n = B.shape
    W = (n + 63) // 64
    pad = np.zeros((F, W * 64), bool); pad[:, :n] = B
    return (pad.reshape(F, W, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)


@pytest.mark.parametrize("flags", BUILDS, ids=BUILD_IDS)
def test_covis_header_matches_the_statement(tmp_path, flags):
    exe = build_prog(tmp_path, "dense_covis_main", flags)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "dense_covis ok"
    # the predicate and the order on the values of the scenes and at the edges of the integer ranges
    big = 2 ** 31 - 1
    preds = [(s, c, n, d) for s in (0, 1, 2, 10, 4010, big) for c in (0, 1, 9, 3579, big) if c <= s
             for n, d in ((9, 10), (4, 5), (0, 1), (1, 1), (2 ** 20, 2 ** 20), (2 ** 20 - 1, 2 ** 20), (1, 2 ** 20))]
    sc = cs.ghost_scene("ghost")
    r = run(sc, cs.build(sc))
    preds += [(int(s), int(c), n, d) for s, c in zip(r["frame"][:, 3], r["frame"][:, 4]) for n, d in ((4, 5), (7, 10), (9, 10), (89, 100))]
    out = subprocess.run([exe, "pred"], input="\n".join(" ".join(map(str, q)) for q in preds) + "\n", capture_output=True, text=True, check=True)
    assert [int(v) for v in out.stdout.split()] == [int(dco.redundant(*q)) for q in preds]
    assert {int(dco.redundant(*q)) for q in preds} == {0, 1}
    cands = [(ua, fa, ub, fb) for ua in (0, 1, 431, big) for ub in (0, 1, 431, big) for fa in (0, 3, 4095) for fb in (0, 3, 4095) if fa != fb]
    out = subprocess.run([exe, "order"], input="\n".join(" ".join(map(str, q)) for q in cands) + "\n", capture_output=True, text=True, check=True)
    assert [int(v) for v in out.stdout.split()] == [int(dco.before(*q)) for q in cands]
    # the pair count of two word rows: every pair of frames of two scenes, the rows written as hexadecimal words
    for name, B in (("ghost", r["B"]), ("points129", vs.points(129)["B"]), ("points64", vs.points(64)["B"])):
        Wd = words_of(B)
        F, W = Wd.shape
        path = tmp_path / f"{name}.txt"
        with open(path, "w") as fh:
            fh.write(f"{F} {W}\n" + "\n".join(" ".join(f"{int(v):x}" for v in row) for row in Wd) + "\n")
        out = subprocess.run([exe, "pairs", str(path)], capture_output=True, text=True, check=True).stdout.split()
        Bi = B.astype(np.int64)
        assert np.array_equal(np.array([int(v) for v in out], np.int64).reshape(F, F), Bi @ Bi.T), name
        assert all(dco.pair_count(Wd[a], Wd[b]) == int((Bi @ Bi.T)[a, b]) for a in range(F) for b in range(F))


# ---- what esl_dense_covis_frames refuses for its parameters (csrc/esl_dense_check.hpp), text by text and in order -------------------------
@pytest.mark.parametrize("flags", BUILDS, ids=BUILD_IDS)
def test_covis_params_check_texts_and_order(tmp_path, flags):
    exe = build_prog(tmp_path, "dense_covis_main", flags)
    defaults = dict(dco.DEFAULTS)
    rungs = GATE_RUNGS + [
        ("window outside 0 .. 4", [dict(window=0), dict(window=4)], [dict(window=-1), dict(window=5)]),
        ("min_others < 1", [dict(min_others=1)], [dict(min_others=0)]),
        ("cover_den outside 1 .. 2^20", [dict(cover_den=2 ** 20), dict(cover_den=1, cover_num=1)], [dict(cover_den=0, cover_num=0), dict(cover_den=2 ** 20 + 1)]),
        ("cover_num outside 0 .. cover_den", [dict(cover_num=0), dict(cover_num=10)], [dict(cover_num=-1), dict(cover_num=11)]),
        ("negative max_cull", [dict(max_cull=0), dict(max_cull=2 ** 31 - 1)], [dict(max_cull=-1)]),
        ("reserved not 0", [], [dict(reserved=1), dict(reserved=-1)]),
    ]
    fields = ["depth_scale", "depth_min", "depth_max", "depth_tol", "window", "min_others", "cover_num", "cover_den", "max_cull", "reserved"]
    check_ladder(exe, fields, defaults, rungs)
    assert NONFINITE
