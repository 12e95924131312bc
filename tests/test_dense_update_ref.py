"""The numpy statement of the dense map's removal, move and purge (tests/dense_update_ref.py) and the scenes of its GPU tests
(tests/dense_update_scenes.py), on the CPU: the scenes' conditions, the statement against from-scratch maps, and its bookkeeping on
cases small enough to count by hand."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_objects_ref as dor       # noqa: E402
import dense_update_ref as ur         # noqa: E402
import dense_update_scenes as us      # noqa: E402

OUTS = ("key", "xyz", "count", "bgr", "inst", "votes")
ZERO_REMOVE = dict(n_sampled=0, n_zero=0, n_depth_out=0, n_key_out=0, n_used=0, n_missing=0, n_emptied=0)


def same_map(a, b):
    ea, eb = a.extract(), b.extract()
    assert ea["n_voxels"] == eb["n_voxels"]
    for k in OUTS:
        assert ea[k].tobytes() == eb[k].tobytes(), k
    assert a.info() == b.info()


@pytest.mark.parametrize("stride", us.STRIDES)
@pytest.mark.parametrize("leaf", us.LEAVES)
def test_scene_conditions(leaf, stride):
    us.removal_conditions(leaf, stride)
    us.move_conditions(leaf, stride)


def test_bridge_conditions():
    assert us.bridge_conditions() == dict(full=1, kept=2)


def test_remove_equals_from_scratch():
    s = us.room()
    mp = us.room_maps(0.05, 1)
    m, _ = us.build(s, range(us.N_CAMS), leaf=0.05)
    res = m.remove_frames(*us.frames_of(s, us.REMOVED))
    cond = us.removal_conditions(0.05, 1)
    assert res["status"] == 0 and res["n_missing"] == 0 and res["n_emptied"] == cond["emptied"]
    assert res["n_used"] == mp["full"].info()["n_samples"] - mp["kept"].info()["n_samples"] > 0
    same_map(m, mp["kept"])
    sl = m.slots()
    assert sl["voxel_slots"] == mp["full"].info()["n_voxels"] and sl["dead_voxels"] == cond["emptied"] and sl["dead_pairs"] > 0
    before, after = m.purge()
    assert before == sl and after == dict(voxel_slots=mp["kept"].info()["n_voxels"], dead_voxels=0, pair_slots=mp["kept"].info()["n_pairs"],
                                          dead_pairs=0)
    same_map(m, mp["kept"])
    # adding the frames again gives the full map back
    m.add_frames(*us.frames_of(s, us.REMOVED))
    same_map(m, mp["full"])


def test_move_equals_from_scratch():
    s = us.with_moved(us.room())
    mp = us.room_maps(0.01, 1)
    cond = us.move_conditions(0.01, 1)
    m, _ = us.build(s, range(us.N_CAMS), leaf=0.01)
    res = m.move_frames(s["cams"], s["cams_moved"], s["K"], s["rows"], s["cols"], s["depth"], s["bgr"], s["inst"])
    assert res["n_frames_moved"] == len(us.MOVED) and res["n_frames_same"] == us.N_CAMS - len(us.MOVED)
    assert res["removed"]["n_emptied"] == cond["revived"] + cond["dead"] and res["removed"]["n_used"] == res["added"]["n_used"] > 0
    same_map(m, mp["moved"])
    sl = m.slots()
    assert sl["dead_voxels"] == cond["dead"] and sl["voxel_slots"] == mp["full"].info()["n_voxels"] + cond["claimed"]
    same = m.move_frames(s["cams_moved"], s["cams_moved"], s["K"], s["rows"], s["cols"], s["depth"], s["bgr"], s["inst"])
    assert same["n_frames_same"] == us.N_CAMS and same["n_frames_moved"] == 0 and same["removed"] == dict(ZERO_REMOVE, status=0)
    same_map(m, mp["moved"])


def two_frames_one_voxel():
    """two 1 x 1 frames on the voxel (0, 0, 0): labels 0 and 1, colours 10 and 30"""
    s = dor.voxel_frames(np.array([[0, 0, 0]]), 0.05, [[0, 1]], None)
    s["bgr"][0] = 10; s["bgr"][1] = 30
    return s


def test_one_voxel_by_hand():
    s = two_frames_one_voxel()
    m, add = us.build(s, [0, 1], leaf=0.05)
    assert add["n_used"] == 2 and m.info()["n_voxels"] == 1 and m.info()["n_pairs"] == 2 and m.extract()["bgr"].tolist() == [[20, 20, 20]]
    r = m.remove_frames(*us.frames_of(s, [0]))
    assert r == dict(ZERO_REMOVE, n_sampled=1, n_used=1, status=0)
    e = m.extract()
    assert e["count"].tolist() == [1] and e["inst"].tolist() == [1] and e["votes"].tolist() == [1] and e["bgr"].tolist() == [[30, 30, 30]]
    assert m.info()["n_samples"] == 1 and m.info()["n_pairs"] == 1
    assert m.slots() == dict(voxel_slots=1, dead_voxels=0, pair_slots=2, dead_pairs=1)
    r = m.remove_frames(*us.frames_of(s, [1]))
    assert r == dict(ZERO_REMOVE, n_sampled=1, n_used=1, n_emptied=1, status=0)
    assert m.info()["n_voxels"] == 0 and m.info()["n_pairs"] == 0 and m.info()["n_samples"] == 0 and m.extract()["n_voxels"] == 0
    assert m.slots() == dict(voxel_slots=1, dead_voxels=1, pair_slots=2, dead_pairs=2)
    assert m.purge()[1] == dict(voxel_slots=0, dead_voxels=0, pair_slots=0, dead_pairs=0)
    # a revived voxel: the slot is no new claim
    m, _ = us.build(s, [0], leaf=0.05)
    m.remove_frames(*us.frames_of(s, [0]))
    m.add_frames(*us.frames_of(s, [1]))
    assert m.slots() == dict(voxel_slots=1, dead_voxels=0, pair_slots=2, dead_pairs=1) and m.extract()["inst"].tolist() == [1]


def test_status_4_routes():
    s = two_frames_one_voxel()
    other = dor.voxel_frames(np.array([[5, 5, 5]]), 0.05, [0], None)
    # a frame that was never added: its voxel is not in the table
    m, _ = us.build(s, [0, 1], leaf=0.05)
    r = m.remove_frames(*us.frames_of(other, [0]))
    assert r["n_missing"] == 1 and r["status"] == 4 and m.info()["n_voxels"] == -1 and m.extract() == dict(n_voxels=-1)
    assert m.slots() == dict(voxel_slots=-1, dead_voxels=-1, pair_slots=-1, dead_pairs=-1)
    assert m.remove_frames(*us.frames_of(s, [0])) == dict(ZERO_REMOVE, status=4)          # nothing more is removed or added
    assert m.add_frames(*us.frames_of(s, [0]))["n_used"] == 0 and m.status == 4
    # ... or its voxel is, but not its pair
    m, _ = us.build(s, [0], leaf=0.05)
    r = m.remove_frames(*us.frames_of(s, [1]))
    assert r["n_missing"] == 1 and r["status"] == 4
    # the same frame twice: a negative count
    m, _ = us.build(s, [0, 1], leaf=0.05)
    assert m.remove_frames(*us.frames_of(s, [0]))["status"] == 0
    r = m.remove_frames(*us.frames_of(s, [0, 1]))
    assert r["n_missing"] == 0 and r["status"] == 4 and m.tables()["cnt"].tolist() == [-1]
    # the only frame with another colour: a dead voxel with a colour sum left
    m, _ = us.build(s, [0], leaf=0.05)
    t = dict(s, bgr=s["bgr"] + 1)
    r = m.remove_frames(*us.frames_of(t, [0]))
    assert r["n_missing"] == 0 and r["n_emptied"] == 1 and r["status"] == 4
    assert m.tables()["cnt"].tolist() == [0] and m.tables()["C"].tolist() == [[-1, -1, -1]]
    # a map at status 3 stays at 3
    m, _ = us.build(dict(s, cams=np.concatenate([s["cams"][:1], other["cams"]])), [0, 1], leaf=0.05, max_voxels=1)
    assert m.status == 3 and m.remove_frames(*us.frames_of(s, [0])) == dict(ZERO_REMOVE, status=3)


def capacity_scene():
    """the room with MOVED at their second poses (the map that fits exactly), and what moving them to the first poses claims"""
    s = us.with_moved(us.room())
    mp = us.room_maps(0.05, 1)
    V = mp["moved"].info()["n_voxels"]
    assert mp["full"].info()["n_voxels"] <= V and mp["full"].info()["n_pairs"] <= 2 * V
    return s, mp, V


def test_capacity_counts_claimed_slots():
    s, mp, V = capacity_scene()
    moved = list(us.MOVED)
    for purge in (False, True):
        m, add = us.build(s, range(us.N_CAMS), "cams_moved", leaf=0.05, max_voxels=V)
        assert add["status"] == 0
        r = m.remove_frames(*us.frames_of(s, moved, "cams_moved"))
        assert r["status"] == 0 and r["n_emptied"] > 0
        if purge:
            before, after = m.purge()
            assert before["voxel_slots"] == V and after["voxel_slots"] == V - r["n_emptied"] and after["dead_voxels"] == 0
        a = m.add_frames(*us.frames_of(s, moved, "cams"))
        if purge:
            assert a["status"] == 0
            same_map(m, us.build(s, range(us.N_CAMS), leaf=0.05, max_voxels=V)[0])
        else:
            assert a["status"] == 3 and len(m.claim_v) > V and m.info()["n_voxels"] == -1
