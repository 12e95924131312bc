"""The numpy statement of the 2-D association (tests/assoc2d_ref.py) against known answers, and its projection against the C oracle.

Measured on the CPU, room_scene(0 .. 5): the statement's unclipped boxes differ from oracle.pyoracle.project_bbox by at most 1.02e-9 px
(seed 0, frame 2, object 19; 4.4e-10 to 7.6e-10 px on the other seeds) -- the oracle walks the reference's route through the inverse
conic and the ellipse's angle, the statement takes the tangent lines of the dual conic.  assoc2d_scenes.TOL = 10 x that = 1.02e-8 px is
what the device tests allow between the device and the statement; assoc2d_scenes.CONDITION stays 100 times above it."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc2d_ref as ar        # noqa: E402
import assoc2d_scenes as sc     # noqa: E402

K, ROWS, COLS = sc.K, sc.ROWS, sc.COLS


@functools.lru_cache(maxsize=None)
def room(seed):
    s = sc.room_scene(seed)
    return s, sc.reference(s)


def test_sphere_on_the_axis():
    r, z = 0.4, 3.0
    pr = ar.predict(sc.IDENTITY_CAM, sc.sphere([0, 0, z], r)[None], K, ROWS, COLS)
    h = r / np.sqrt(z * z - r * r)
    want = [K[2] - K[0] * h, K[3] - K[1] * h, K[2] + K[0] * h, K[3] + K[1] * h]
    assert pr["flags"][0] == 1 and pr["depth"][0] == z
    assert np.abs(pr["boxes"][0] - want).max() < 1e-10
    assert np.abs(pr["raw"][0] - want).max() < 1e-10


def test_iou_of_hand_made_boxes():
    a = np.array([0.0, 0, 10, 10])
    assert ar.iou(a, a) == 1.0
    assert ar.iou(a, np.array([5.0, 0, 15, 10])) == pytest.approx(50 / 150)
    assert ar.iou(a, np.array([5.0, 5, 15, 15])) == pytest.approx(25 / 175)
    assert ar.iou(a, np.array([10.0, 0, 20, 10])) == 0.0          # touching
    assert ar.iou(a, np.array([20.0, 20, 30, 30])) == 0.0
    assert ar.iou(a, np.array([2.0, 2, 4, 4])) == pytest.approx(4 / 100)


def test_two_spheres_on_one_ray():
    objs = np.stack([sc.sphere([0, 0, 6.0], 0.5), sc.sphere([0, 0, 3.0], 0.5)])
    pr = ar.predict(sc.IDENTITY_CAM, objs, K, ROWS, COLS)
    assert list(pr["flags"]) == [3, 1]                              # the far one is covered entirely
    assert list(ar.predict(sc.IDENTITY_CAM, objs, K, ROWS, COLS, dict(occlusion=0))["flags"]) == [1, 1]
    # 0.7 is the threshold: a near sphere shifted so that it covers about half of the far box hides nothing
    objs[1, 0] = 0.5
    cover = ar.overlap(pr["boxes"][0], ar.predict(sc.IDENTITY_CAM, objs, K, ROWS, COLS)["boxes"][1]) / ar.area(pr["boxes"][0])
    assert 0.3 < cover < 0.7
    assert list(ar.predict(sc.IDENTITY_CAM, objs, K, ROWS, COLS)["flags"]) == [1, 1]
    assert list(ar.predict(sc.IDENTITY_CAM, objs, K, ROWS, COLS, dict(occl_ratio=0.3))["flags"]) == [3, 1]


def test_behind_and_inside_are_ineligible():
    objs = np.stack([sc.sphere([0, 0, -3.0], 0.4), sc.sphere([0.1, 0, 0.2], 1.0), sc.sphere([0, 0, 3.0], 0.4)])
    pr = ar.predict(sc.IDENTITY_CAM, objs, K, ROWS, COLS)
    assert list(pr["flags"]) == [0, 0, 1]
    assert np.isnan(pr["boxes"][:2]).all() and np.isnan(pr["depth"][:2]).all()
    # too small a box: 2 fx r / z below min_box_px
    assert ar.predict(sc.IDENTITY_CAM, sc.sphere([0, 0, 30.0], 0.2)[None], K, ROWS, COLS)["flags"][0] == 0


def test_row_order_greedy():
    objs = sc.sphere([0, 0, 3.0], 0.4)[None]
    box = ar.predict(sc.IDENTITY_CAM, objs, K, ROWS, COLS)["boxes"][0]
    det = np.stack([box + [3, 0, 3, 0], box])                       # the second fits better, the first comes first
    r = ar.associate(sc.IDENTITY_CAM[None], objs, [2], K, ROWS, COLS, [0, 2], det, [2, 2])
    assert list(r["assoc"]) == [0, -1] and r["iou"][1] == 0 and 0.3 < r["iou"][0] < 1
    assert list(r["frame_stats"][0]) == [1, 0, 1, 0]
    r = ar.associate(sc.IDENTITY_CAM[None], objs, [2], K, ROWS, COLS, [0, 2], det, [1, 2])     # labels: the first has no candidate
    assert list(r["assoc"]) == [-1, 0] and r["iou"][1] == 1.0
    r = ar.associate(sc.IDENTITY_CAM[None], objs, [2], K, ROWS, COLS, [0, 2], det, [1, 2], dict(match_labels=0))
    assert list(r["assoc"]) == [0, -1]
    bad = np.stack([[10, 10, 10, 50.0], [np.nan, 0, 5, 5], box])    # degenerate boxes claim nothing
    r = ar.associate(sc.IDENTITY_CAM[None], objs, [2], K, ROWS, COLS, [0, 3], bad, [2, 2, 2])
    assert list(r["assoc"]) == [-1, -1, 0]


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_generated_scenes(seed):
    s, ref = room(seed)
    sc.check_conditions(ref)
    st = ref["frame_stats"]
    assert st[:, 0].min() >= 10 and st[:, 1].min() >= 1 and (st[:, 3] == 0).all()
    assert np.array_equal(ref["assoc"], s["true_obj"])              # every detection recovers its own object
    assert np.array_equal(st[:, 2], np.diff(s["det_offsets"]))
    sc.check_conditions(sc.reference(s, min_iou=0.6))


def test_projection_against_the_oracle(po):
    """largest disagreement of the unclipped boxes over every eligible prediction of the six scenes: 1.02e-9 px (module docstring)"""
    worst = 0.0
    for seed in sc.SEEDS:
        s, ref = room(seed)
        for f, pr in enumerate(ref["frames"]):
            for m in np.nonzero(pr["flags"] & 1)[0]:
                worst = max(worst, np.abs(po.project_bbox(s["cams"][f], s["objs"][m], np.array(K)) - pr["raw"][m]).max())
    print(f"numpy statement against the oracle: {worst:.3e} px")
    assert 0 < worst < sc.TOL
    assert sc.CONDITION >= 100 * sc.TOL
