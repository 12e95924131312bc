"""The numpy statement of esl_dense_* (tests/dense_ref.py) pinned by itself, and csrc/esl_dense_key.hpp -- the header the kernels
compile -- held to it on the host (tests/dense_key_main.cpp).  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as dr          # noqa: E402
import dense_scenes as sc       # noqa: E402
from dense_prog import BUILDS, BUILD_IDS, NONFINITE, build_prog, check_ladder          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ID = [0, 0, 0, 0, 0, 0, 1.0]
TWO30 = 1 << 30


def same_map(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def hand_map():
    """two identity frames of 2 x 2 pixels, leaf 1, depth_scale 2, fx = fy = 2, cx = cy = 0.5: z = 3, 2, none, 200 m; then 3.5 m"""
    m = dr.DenseMap(leaf=1.0, depth_scale=2.0, depth_min=0.5, depth_max=100.0)
    depth = np.array([[[6, 4], [0, 400]], [[7, 0], [0, 0]]], np.uint16)
    bgr = np.zeros((2, 2, 2, 3), np.uint8); inst = np.full((2, 2, 2), -1, np.int32)
    bgr[0, 0, 0] = (10, 0, 255); bgr[0, 0, 1] = (7, 8, 9); inst[0, 0, 0] = 5
    bgr[1, 0, 0] = (11, 0, 254); inst[1, 0, 0] = 2
    r0 = m.add_frames([ID], (2.0, 2.0, 0.5, 0.5), 2, 2, depth[:1], bgr[:1], inst[:1])
    r1 = m.add_frames([ID], (2.0, 2.0, 0.5, 0.5), 2, 2, depth[1:], bgr[1:], inst[1:])
    return m, r0, r1


def test_hand_computed_case():
    m, r0, r1 = hand_map()
    assert r0 == dict(n_sampled=4, n_zero=1, n_depth_out=1, n_key_out=0, n_used=2, status=0)
    assert r1 == dict(n_sampled=4, n_zero=3, n_depth_out=0, n_key_out=0, n_used=1, status=0)
    e = m.extract()
    # pixel (0, 0): x = y = (0 - 0.5) z / 2 = -0.75 at z = 3, -0.875 at z = 3.5: floor gives -1 where truncation gives 0
    # pixel (1, 0): x = 0.5, y = -0.5 at z = 2
    assert e["n_voxels"] == 2 and e["key"].tolist() == [[-1, -1, 3], [0, -1, 2]]
    assert e["count"].tolist() == [2, 1]
    fx = -805306368 + -939524096          # -0.75 2^30 + -0.875 2^30
    assert fx == -1744830464
    assert e["xyz"].tolist() == [[fx / TWO30 / 2, fx / TWO30 / 2, 6979321856 / TWO30 / 2], [0.5, -0.5, 2.0]]
    assert e["xyz"][0].tolist() == [-0.8125, -0.8125, 3.25]
    # B: (10 + 11) / 2 = 10.5 rounds half up to 11; R: (255 + 254) / 2 = 254.5 -> 255
    assert e["bgr"].tolist() == [[11, 0, 255], [7, 8, 9]]
    # ids 5 and 2 with one vote each: the lower id; the second voxel has no labelled sample
    assert e["inst"].tolist() == [2, -1] and e["votes"].tolist() == [1, 0]
    assert m.info() == dict(n_samples=3, n_voxels=2, n_pairs=2, status=0, with_color=1, with_inst=1)
    # the fixed-point sums themselves
    keys, inv = np.unique(m.key, return_inverse=True)
    S = np.zeros((2, 3), np.int64); np.add.at(S, inv, m.fix)
    assert S.tolist() == [[fx, fx, 6979321856], [536870912, -536870912, 2147483648]]
    assert keys.tolist() == [((-1 + 2**20) << 42) | ((-1 + 2**20) << 21) | (3 + 2**20), ((0 + 2**20) << 42) | ((-1 + 2**20) << 21) | (2 + 2**20)]


def test_pack_order_and_round_trip():
    rng = np.random.default_rng(0)
    k = rng.integers(-dr.KEY_MAX, dr.KEY_MAX + 1, (2000, 3))
    k[:4] = [[-dr.KEY_MAX] * 3, [dr.KEY_MAX] * 3, [0, 0, 0], [-1, -1, -1]]
    key = dr.pack(k)
    assert np.array_equal(dr.unpack(key), k) and (key != np.uint64(2**64 - 1)).all()
    assert np.array_equal(np.argsort(key, kind="stable"), np.lexsort((k[:, 2], k[:, 1], k[:, 0])))


@pytest.mark.parametrize("seed", sc.ROOM_SEEDS)
@pytest.mark.parametrize("leaf,stride", [(0.05, 1), (0.2, 1), (0.01, 1), (0.05, 3), (0.2, 3), (0.01, 3)])
def test_room_conditions(seed, leaf, stride):
    s = sc.room_scene(seed)
    m, adds = sc.reference(s, leaf=leaf, stride=stride)
    sc.check_conditions(m, min_largest=100 if leaf == 0.2 and stride == 1 else 0)
    a = adds[0]
    assert a["n_sampled"] == 3 * -(-48 // stride) * -(-64 // stride) and a["n_key_out"] == 0 and a["n_depth_out"] == 0
    assert a["n_zero"] + a["n_used"] == a["n_sampled"] and 0.03 < a["n_zero"] / a["n_sampled"] < 0.08
    e = m.extract()
    assert e["count"].sum() == a["n_used"] and (e["votes"] <= e["count"]).all()
    assert ((e["inst"] >= 0) == (e["votes"] > 0)).all()
    if stride == 1:
        assert {0, 1, 2, 10, 11, 12} <= set(e["inst"].tolist())          # the three bodies and the wall's patches
    if leaf == 0.2 and stride == 1:          # voxels on the outlines get mixed votes
        assert ((e["votes"] > 0) & (e["votes"] < e["count"])).sum() >= 5


def test_permutations_change_no_bit():
    s = sc.room_scene(0)
    base = sc.reference(s, leaf=0.05)[0].extract()
    rev = dict(s, cams=s["cams"][::-1], depth=s["depth"][::-1], bgr=s["bgr"][::-1], inst=s["inst"][::-1])
    same_map(base, sc.reference(rev, leaf=0.05)[0].extract())
    m = sc.reference(s, leaf=0.05)[0]
    perm = np.random.default_rng(1).permutation(len(m.key))          # the samples in any order
    for name in ("key", "fix", "bgr", "id", "frame", "pw"):
        setattr(m, name, getattr(m, name)[perm])
    same_map(base, m.extract())


def test_incremental_equals_batch():
    s = sc.room_scene(1)
    batch, _ = sc.reference(s, leaf=0.05)
    inc, adds = sc.reference(s, calls=[[0], [1], [2]], leaf=0.05)
    same_map(batch.extract(), inc.extract())
    assert batch.info() == inc.info() and sum(a["n_used"] for a in adds) == batch.info()["n_samples"]
    assert batch.extract(cap=10)["key"].tolist() == batch.extract()["key"][:10].tolist() and batch.extract(cap=0)["n_voxels"] == batch.n_voxels()


def test_vote_ties_and_majorities():
    m = dr.DenseMap(leaf=10.0, depth_scale=1000.0)          # one voxel
    depth = np.full((1, 1, 6), 2000, np.uint16); bgr = np.zeros((1, 1, 6, 3), np.uint8)
    for ids, want in (([4, 4, 9, 9, -1, -1], (4, 2)), ([9, 9, 4, 4, -1, 7], (4, 2)), ([3, 8, 8, 8, 3, 3], (3, 3)), ([-1] * 6, (-1, 0)),
                      ([0, 1, 1, -1, -1, -1], (1, 2))):
        m = dr.DenseMap(leaf=10.0, depth_scale=1000.0)
        m.add_frames([ID], (60.0, 60.0, -1.0, -1.0), 1, 6, depth, bgr, np.array(ids, np.int32).reshape(1, 1, 6))
        e = m.extract()
        assert e["n_voxels"] == 1 and (int(e["inst"][0]), int(e["votes"][0])) == want, ids


def test_capacity_and_errors():
    s = sc.room_scene(0)
    V = sc.reference(s, leaf=0.2)[0].n_voxels()
    assert sc.reference(s, leaf=0.2, max_voxels=V)[0].status == 0
    m, adds = sc.reference(s, leaf=0.2, max_voxels=V - 1)
    assert m.status == 3 and adds[0]["status"] == 3 and m.extract() == dict(n_voxels=-1) and m.info()["n_voxels"] == -1
    again = m.add_frames(s["cams"], s["K"], s["rows"], s["cols"], s["depth"], s["bgr"], s["inst"])
    assert again["n_used"] == 0 and again["status"] == 3
    for bad in ([0, 0, 0, 0, 0, 0, 0], [0, 0, np.nan, 0, 0, 0, 1], [0, 0, 0, np.inf, 0, 0, 1], [0, 0, 0, 1e200, 1e200, 0, 0]):
        with pytest.raises(dr.InvalidPose):
            dr.pose(bad)


# ---- the header against the statement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan_ubsan"])
def test_key_header_matches_the_statement(tmp_path, flags):
    exe = build_prog(tmp_path, "dense_key_main", flags)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "dense_key ok"
    for leaf, stride, shift in ((0.05, 1, None), (0.01, 3, None), (1e-6, 1, None), (0.05, 1, sc.NEGATIVE_SHIFT)):
        s = sc.room_scene(0, shift=shift)
        p = dict(dr.DEFAULTS, leaf=leaf, stride=stride, depth_min=1.6)          # some samples fall below depth_min
        lines, expect = [], []
        for f, cam in enumerate(s["cams"]):
            rows_, cols_ = np.meshgrid(np.arange(0, s["rows"], stride), np.arange(0, s["cols"], stride), indexing="ij")
            smp = dr.samples(cam, s["K"], s["rows"], s["cols"], s["depth"][f], p)
            used = {(r, c): i for i, (r, c) in enumerate(zip(smp["row"].tolist(), smp["col"].tolist()))}
            fix = np.rint(smp["pw"] * dr.FIX).astype(np.int64); key = dr.pack(smp["k"])
            n_other = 0
            for r, c in zip(rows_.reshape(-1).tolist(), cols_.reshape(-1).tolist()):
                raw = int(s["depth"][f, r, c])
                lines.append(" ".join(repr(float(v)) for v in cam) + f" {raw} {c} {r}")
                if (r, c) in used:
                    i = used[(r, c)]
                    expect.append(f"0 {int(key[i])} {fix[i, 0]} {fix[i, 1]} {fix[i, 2]}")
                else:
                    expect.append(None); n_other += 1
            assert n_other == smp["counts"]["n_zero"] + smp["counts"]["n_depth_out"] + smp["counts"]["n_key_out"]
            if leaf == 1e-6:
                assert smp["counts"]["n_used"] == 0 and smp["counts"]["n_key_out"] > 1000
            if shift is not None:
                assert (smp["k"] < 0).all()
        head = f"{leaf!r} {p['depth_scale']!r} {p['depth_min']!r} {p['depth_max']!r} " + " ".join(repr(float(v)) for v in s["K"]) + f" {len(lines)}\n"
        out = subprocess.run([exe, "samples"], input=head + "\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == len(lines) + 1
        n_used = 0
        for got, want in zip(out, expect):
            if want is None:
                assert got.split()[0] in ("1", "2", "3") and got.split()[1:] == ["0"] * 4
            else:
                assert got == want; n_used += 1
        assert n_used > 500 or leaf == 1e-6


# ---- what the entries refuse for the image geometry (csrc/esl_dense_check.hpp), text by text and in order ---------------------------------
TINY = 5e-324          # the smallest positive double: the first value above 0, its negative the first below


@pytest.mark.parametrize("flags", BUILDS, ids=BUILD_IDS)
def test_image_check_texts_and_order(tmp_path, flags):
    """dense_image_check, which esl_dense_add / _remove / _move_frames, esl_dense_render, esl_dense_align_frames and esl_dense_carve_frames
    call: every rung at its last accepted and first refused value, NaN and the infinities, and the earlier rung's text when two fail."""
    exe = build_prog(tmp_path, "dense_key_main", flags)
    defaults = dict(null_K=0, rows=480, cols=640, fx=525.0, fy=525.0, cx=319.5, cy=239.5)
    rungs = [
        ("null K", [], [dict(null_K=1)]),
        ("rows < 1 or > 16384", [dict(rows=1), dict(rows=16384)], [dict(rows=0), dict(rows=16385), dict(rows=-1)]),
        ("cols < 1 or > 16384", [dict(cols=1), dict(cols=16384)], [dict(cols=0), dict(cols=16385), dict(cols=-1)]),
        ("fx not finite or <= 0", [dict(fx=TINY), dict(fx=1e308)], [dict(fx=0.0), dict(fx=-TINY)] + [dict(fx=v) for v in NONFINITE]),
        # cx and cy are free here: esl_dense_align_frames alone asks them to be finite, in its entry
        ("fy not finite or <= 0", [dict(fy=TINY), dict(fy=1e308)] + [dict(cx=v) for v in NONFINITE] + [dict(cy=v) for v in NONFINITE],
         [dict(fy=0.0), dict(fy=-TINY)] + [dict(fy=v) for v in NONFINITE]),
    ]
    check_ladder(exe, ["null_K", "rows", "cols", "fx", "fy", "cx", "cy"], defaults, rungs)
