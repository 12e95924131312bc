"""Scenes of the esl_dense_remove_frames / _move_frames / _purge tests, and the conditions, asserted on the numpy statement alone
(tests/dense_update_ref.py), under which the tests test something: a removal that empties voxels, thins others and changes labels, a
move that revives, claims and leaves dead slots, a bridge whose removal splits a component.  Built on tests/dense_scenes.py; everything
is generated from fixed seeds.  Nothing here is imported by the package."""
import functools

import numpy as np

import dense_objects_ref as dor
import dense_ref as dr
import dense_scenes as sc
import dense_update_ref as ur
import render_scenes as rs

SEED, N_CAMS = 2, 4
REMOVED = (1,)                      # the frames the removal tests take out; the others are kept
MOVED = (1, 3)                      # the frames the move tests move from the first pose set to the second
MAXV = 65536
LEAVES, STRIDES = (0.01, 0.05), (1, 3)
BRIDGE_LEAF, BRIDGE_REACH = 0.05, 2


def quat_mul(a, b):
    """Hamilton product of (x, y, z, w) quaternions"""
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def second_poses(cams, seed=0):
    """every pose a few millimetres and milliradians off"""
    rng = np.random.default_rng(9000 + seed)
    out = np.array(cams, dtype=np.float64)
    for f in range(len(out)):
        out[f, :3] += rng.uniform(-0.004, 0.004, 3)
        out[f, 3:] = quat_mul(out[f, 3:], rs.quat(rng.normal(size=3), rng.uniform(0.002, 0.005)))
    return out


@functools.lru_cache(maxsize=None)
def room():
    """dense_scenes.room_scene with four frames, and its second pose set as cams2"""
    s = sc.room_scene(SEED, n_cams=N_CAMS)
    return dict(s, cams2=second_poses(s["cams"]))


def kept(F=N_CAMS, removed=REMOVED):
    return [f for f in range(F) if f not in removed]


def frames_of(s, idx, cams="cams"):
    """the arguments of an add / remove call for the frames idx of a scene, after K, rows and cols"""
    idx = list(idx)
    return (s[cams][idx], s["K"], s["rows"], s["cols"], s["depth"][idx], s["bgr"][idx], s["inst"][idx])


def build(s, idx, cams="cams", cls=ur.DenseUpdateMap, with_color=True, with_inst=True, **over):
    over.setdefault("max_voxels", MAXV)
    m = cls(with_color, with_inst, **over)
    res = m.add_frames(*frames_of(s, idx, cams))
    return m, res


def with_moved(s, moved=MOVED):
    """the scene's poses with the frames `moved` at their second pose"""
    c = s["cams"].copy()
    c[list(moved)] = s["cams2"][list(moved)]
    return dict(s, cams_moved=c)


@functools.lru_cache(maxsize=None)
def room_maps(leaf, stride):
    """the statement's maps of the room at one leaf and stride, each checked for the conditions of exact equality:
    full (all frames, first poses), kept (from scratch), moved (from scratch, MOVED at the second poses)"""
    s = with_moved(room())
    out = {}
    for name, idx, cams in (("full", range(N_CAMS), "cams"), ("kept", kept(), "cams"), ("moved", range(N_CAMS), "cams_moved"),
                            ("second", range(N_CAMS), "cams2")):
        m, _ = build(s, idx, cams, leaf=leaf, stride=stride)
        sc.check_conditions(m)
        out[name] = m
    return out


def removal_conditions(leaf, stride):
    """on the statement alone: the removal of REMOVED empties a voxel, thins a shared one and changes a winning label"""
    mp = room_maps(leaf, stride)
    full, rest = mp["full"], mp["kept"]
    gone = np.isin(full.frame, REMOVED)
    k_gone, k_kept = np.unique(full.key[gone]), np.unique(full.key[~gone])
    emptied = np.setdiff1d(k_gone, k_kept)
    shared = np.intersect1d(k_gone, k_kept)
    assert len(emptied) > 0, "the removal empties no voxel"
    assert len(shared) > 0, "no voxel holds samples of a removed and of a kept frame"
    ef, ek = full.extract(), rest.extract()
    pf = dr.pack(ef["key"]); pk = dr.pack(ek["key"])
    both = np.isin(pf, pk)
    assert np.array_equal(pf[both], pk)
    changed = int((ef["inst"][both] != ek["inst"]).sum())
    assert changed > 0, "the removal changes no winning label"
    return dict(emptied=len(emptied), shared=len(shared), relabelled=changed)


def move_conditions(leaf, stride):
    """on the statement alone: moving MOVED revives a dead voxel, claims a new one and leaves one dead"""
    mp = room_maps(leaf, stride)
    full, new = mp["full"], mp["moved"]
    gone = np.isin(full.frame, MOVED)
    emptied = np.setdiff1d(np.unique(full.key[gone]), np.unique(full.key[~gone]))
    after = np.unique(new.key)
    revived = np.intersect1d(emptied, after)
    claimed = np.setdiff1d(after, np.unique(full.key))
    dead = np.setdiff1d(emptied, after)
    assert len(revived) > 0, "the move revives no dead voxel"
    assert len(claimed) > 0, "the move claims no new voxel"
    assert len(dead) > 0, "the move leaves no dead voxel"
    return dict(revived=len(revived), claimed=len(claimed), dead=len(dead))


# ---- the bridge: two blobs of one label, joined only through the voxel of one extra frame ----------------------------------------------
@functools.lru_cache(maxsize=None)
def bridge():
    """-> dict(frames: 1 x 1 frames, one per voxel, the bridge's LAST; n_blob: the frames of the two blobs).  Two 3 x 3 x 3 blobs of label
    0 whose nearest voxels are 4 apart along x, and one voxel half way: within reach 2 of both"""
    a = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    keys = np.concatenate([a + np.array([-1, 0, 2]), a + np.array([5, 0, 2]), np.array([[3, 1, 3]])])
    s = dor.voxel_frames(keys, BRIDGE_LEAF, np.zeros(len(keys), int), None)
    assert len(s["cams"]) == len(keys)
    return dict(frames=s, n_blob=len(keys) - 1)


def bridge_conditions():
    """on the statement alone: the full map has one component of label 0, the map of the blobs' frames has two"""
    b = bridge()
    s, n = b["frames"], b["n_blob"]
    out = {}
    for name, idx in (("full", range(n + 1)), ("kept", range(n))):
        m, _ = build(s, idx, leaf=BRIDGE_LEAF)
        sc.check_conditions(m, two_frames=False)
        r = dor.objects(m.extract(), BRIDGE_LEAF, 1, (0.0, 0.0, 1.0, 0.0), reach=BRIDGE_REACH, min_component=1)
        out[name] = r["result"]["n_components"]
    assert out == dict(full=1, kept=2), out
    return out
