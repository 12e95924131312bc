"""Scenes of the esl_map_overlaps / esl_map_merge tests, and the conditions under which exact agreement between the numpy statement
(tests/map_merge_ref.py) and the device is a fair demand.

Comparison rule: counts, pair lists, n_*, groups, indices, merged rows and the rewritten list are exact; iou and contain agree within
TOL = 1e-12 absolute (from equal integers they are a dozen FP64 operations on values in [0, 1]).  check_conditions asserts, on the
reference alone and before any device call, that no sample has |q - 1| < Q_MARGIN (the device may contract to FMA, numpy does not), no
gate quantity lies within GATE_MARGIN relative of its threshold and no iou / contain within THR_MARGIN of min_iou / min_contain.  The
seeds below were picked on the CPU so that every scene satisfies them."""
import functools

import numpy as np

import map_merge_ref as mr

TOL = 1e-12
Q_MARGIN = 1e-9
GATE_MARGIN = 1e-6
THR_MARGIN = 1e-6
# the largest |iou(n = 16) - iou(n = 64)| over the 300 random oriented overlapping pairs of estimator_pairs(), measured by
# tests/test_map_merge_ref.py::test_lattice_16_against_64, which asserts twice this value
IOU_ERR_N16 = 0.0076
CLUTTER_SEEDS = (0, 1, 2)          # lattice 16
CLUTTER_SEED_BY_LATTICE = {4: 3, 5: 4, 32: 5}


def ell(c, s, yaw=0.0, q=None):
    """the 10-vector: centre, quaternion (x, y, z, w), half-axes"""
    if q is None:
        q = [0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)]
    return np.concatenate([np.asarray(c, float), np.asarray(q, float), np.asarray(s, float)])


def sphere(c, r):
    return ell(c, [r, r, r])


def random_ell(rng, lo, hi, smin=0.2, smax=0.6):
    q = rng.normal(size=4)
    return ell(rng.uniform(lo, hi, 3), rng.uniform(smin, smax, 3), q=q / np.linalg.norm(q))


def check_conditions(ov):
    """ov: the dict of map_merge_ref.overlaps (or merge()['overlaps'])"""
    m = ov["margins"]
    assert m["q"] >= Q_MARGIN, f"a sample has |q - 1| = {m['q']:.3g}"
    assert m["gate"] >= GATE_MARGIN, f"a gate quantity is within {m['gate']:.3g} of its threshold"
    assert m["thr"] >= THR_MARGIN, f"an iou / contain is within {m['thr']:.3g} of its threshold"


# ---- the estimator ----------------------------------------------------------------------------------------------------------------------------
def estimator_pairs(count=300, seed=7):
    """random oriented pairs that overlap: (count, 2, 10)"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        a = random_ell(rng, -0.1, 0.1)
        b = random_ell(rng, -0.35, 0.35)
        out.append(np.stack([a, b]))
    return np.array(out)


def pair_iou(pair, n):
    ov = mr.overlaps(pair, [0, 0], lattice=n) if n <= 32 else None
    if ov is not None:
        return (float(ov["iou"][0]), float(ov["contain"][0])) if ov["n_pairs"] else (0.0, 0.0)
    pre = mr.prepare(pair)                      # a lattice finer than the interface admits: the same statement, called directly
    k = mr.lattice(n).astype(np.float64)
    ca, cb = int((mr.q_values(pre, 0, 1, k, n) <= 1).sum()), int((mr.q_values(pre, 1, 0, k, n) <= 1).sum())
    return mr.measures(ca, cb, pre["V"][0], pre["V"][1], len(k))


# ---- cluttered random scenes ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clutter_scene(seed, M=40, box=1.2, n_labels=2):
    rng = np.random.default_rng(1000 + seed)
    objs = np.array([random_ell(rng, 0, box) for _ in range(M)])
    labels = rng.integers(0, n_labels, M).astype(np.int32)
    F = 12
    n_obs = 6 * M
    obs_obj = rng.integers(-1, M, n_obs).astype(np.int32)      # -1: skipped entries among them
    obs_cam = rng.integers(0, F, n_obs).astype(np.int32)
    weights = rng.integers(0, 5, M).astype(np.int32)           # small: ties, so that the lowest index decides too
    return dict(objs=objs, labels=labels, obs_cam=obs_cam, obs_obj=obs_obj, weights=weights)


@functools.lru_cache(maxsize=None)
def dense_cluster(M=300, seed=0):
    """every pair a candidate: M (M - 1) / 2 of them, one label"""
    rng = np.random.default_rng(2000 + seed)
    objs = np.array([random_ell(rng, 0, 0.25, 0.3, 0.5) for _ in range(M)])
    return dict(objs=objs, labels=np.zeros(M, np.int32))


# ---- planted duplicates -----------------------------------------------------------------------------------------------------------------------
N_PLANTED, N_COPIES, PLANTED_FRAMES = 60, 25, 30


@functools.lru_cache(maxsize=None)
def planted_scene(seed=0):
    """60 separated objects on a jittered grid, 25 of them a second time: centre moved by up to 10 % of the smallest half-axis, axes
    changed by +-10 %, yaw by +-10 degrees.  The copies stand behind the originals (index 60 + k is the copy of copy_of[k]).  The edge
    list gives every object 8 - 20 frames; a duplicated object's frames are split between the two copies, two more frames box both
    (the conflicts of step 7), a few entries are skipped, and the list is shuffled."""
    rng = np.random.default_rng(3000 + seed)
    objs, labels = [], []
    for g in range(N_PLANTED):
        c = np.array([g % 8, (g // 8) % 8, 0.0]) * 0.9 + rng.uniform(-0.1, 0.1, 3)
        objs.append(ell(c, rng.uniform(0.25, 0.6, 3), yaw=rng.uniform(-np.pi, np.pi)))
        labels.append(int(rng.integers(0, 4)))
    copy_of = np.sort(rng.choice(N_PLANTED, N_COPIES, replace=False))
    for o in copy_of:
        v = objs[o]
        yaw = 2 * np.arctan2(v[5], v[6]) + np.deg2rad(rng.uniform(-10, 10))
        c = v[:3] + rng.uniform(-1, 1, 3) / np.sqrt(3) * 0.1 * v[7:].min()
        objs.append(ell(c, v[7:] * rng.uniform(0.9, 1.1, 3), yaw=yaw))
        labels.append(labels[o])
    objs, labels = np.array(objs), np.array(labels, np.int32)
    M = len(objs)
    cam, obj = [], []
    for o in range(N_PLANTED):
        frames = rng.choice(PLANTED_FRAMES, int(rng.integers(8, 21)), replace=False)
        k = np.nonzero(copy_of == o)[0]
        if len(k) == 0:
            cam += list(frames); obj += [o] * len(frames)
            continue
        dup = N_PLANTED + int(k[0])
        for f in frames[:-2]:
            cam.append(f); obj.append(o if rng.random() < 0.5 else dup)
        for f in frames[-2:]:
            cam += [f, f]; obj += [o, dup]
    cam += list(rng.integers(0, PLANTED_FRAMES, 15)); obj += [-1] * 10 + [-7] * 5
    order = rng.permutation(len(cam))
    group = np.arange(M); group[N_PLANTED:] = copy_of
    return dict(objs=objs, labels=labels, obs_cam=np.array(cam, np.int32)[order], obs_obj=np.array(obj, np.int32)[order],
                copy_of=copy_of, group=group.astype(np.int32), weights=rng.integers(1, 50, M).astype(np.int32))


# ---- hand-made geometry -------------------------------------------------------------------------------------------------------------------------
def chain(n, spacing=0.52, tilt=0.37):
    """n unit spheres on a tilted line: neighbours (0.52 apart: iou 0.45) link, next-but-one (1.04: iou 0.17, contain 0.29) do not"""
    d = np.array([np.cos(tilt), np.sin(tilt) * 0.8, np.sin(tilt) * 0.6])
    return np.array([sphere(0.013 + d * spacing * i, 1.0) for i in range(n)])


def sphere_lens_iou(r1, r2, d):
    """closed form: two spheres at distance d, |r1 - r2| < d < r1 + r2"""
    lens = np.pi * (r1 + r2 - d) ** 2 * (d * d + 2 * d * (r1 + r2) - 3 * (r1 - r2) ** 2) / (12 * d)
    v1, v2 = 4 / 3 * np.pi * r1 ** 3, 4 / 3 * np.pi * r2 ** 3
    return lens / (v1 + v2 - lens), lens / min(v1, v2)
