"""The numpy statement of esl_init_quadrics_robust (include/esl.h, "consensus SVD initialisation", steps 1-7): the sampler in Python
integers, the hypothesis fits through the C oracle's single-object path (pyoracle.init_quadric), the boxes through
pyoracle.project_bbox, the bbox edge's visibility predicate as tests/assoc2d_ref.py states it (restated over all entries of an object at
once; tests/test_init_robust_ref.py holds the two together), the refit through init_batch_ref.reference on the masked list.

Also the planted scenes the tests share: the scenes of init_batch_ref with some boxes of every object of >= 15 observations moved
40-80 px, and one long list whose refit goes through the slab."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_batch_ref as ib     # noqa: E402

M64 = (1 << 64) - 1
DEFAULTS = dict(sample_size=5, n_hypotheses=64, inlier_px=10.0, min_inliers=8, refine=1, seed=0)
NEAR_PX = 1e-3      # a residual this close to inlier_px makes the flag a coin toss between two correct implementations
LONG_LIST = ("L600", 3, 300)   # scene, object, entries: more than 248 inliers, so the refit's plane matrix goes to the slab


def params(**over):
    p = dict(DEFAULTS)
    for k, v in over.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


# ---- step 2: the sampler ------------------------------------------------------------------------------------------------------------
def mix(seed, h, k):
    """the splitmix64 finaliser of seed ^ (0x9E3779B97F4A7C15 * (32 h + k + 1)), mod 2^64"""
    seed, h, k = int(seed), int(h), int(k)     # Python integers: a numpy integer would overflow
    z = (seed ^ ((0x9E3779B97F4A7C15 * (32 * h + k + 1)) & M64)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def n_hypotheses(n, sample_size, H):
    return 1 if n <= sample_size else H


def sample(seed, h, n, sample_size):
    """the ascending local indices of hypothesis h of an object with n entries (Floyd's sampling)"""
    s = min(sample_size, n)
    if n <= sample_size:
        return list(range(n))
    out = []
    for k in range(s):
        j = n - s + k
        t = (mix(seed, h, k) >> 11) % (j + 1)
        out.append(j if t in out else t)
    return sorted(out)


# ---- the planted scenes ----------------------------------------------------------------------------------------------------------------
def plant(s, rng):
    """s with max(1, int(0.15 n)) boxes of every object of n >= 15 entries moved by 40-80 px in x and in y; 'planted' marks them"""
    boxes = np.array(s["obs_boxes"], dtype=np.float64)
    planted = np.zeros(len(boxes), bool)
    for sel in ib.group(s["obs_obj"], s["N"]):
        n = len(sel)
        if n < 15:
            continue
        nout = max(1, int(0.15 * n))
        bad = rng.choice(n, nout, replace=False)
        sign = rng.choice([-1, 1], (nout, 2))
        mag = rng.uniform(40, 80, (nout, 2))
        boxes[sel[bad], 0] += sign[:, 0] * mag[:, 0]; boxes[sel[bad], 2] += sign[:, 0] * mag[:, 0]
        boxes[sel[bad], 1] += sign[:, 1] * mag[:, 1]; boxes[sel[bad], 3] += sign[:, 1] * mag[:, 1]
        planted[sel[bad]] = True
    out = dict(s, obs_boxes=boxes, planted=planted)
    boxes.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def planted_scene(name):
    """init_batch_ref.scene(name) planted with default_rng(0); "LONG": the long list, one object"""
    if name == "LONG":
        base, o, n = LONG_LIST
        s = ib.scene(base)
        sel = ib.group(s["obs_obj"], s["N"])[o][:n]
        assert len(sel) == n
        one = dict(cams=s["cams"], N=1, obs_cam=s["obs_cam"][sel], obs_obj=np.zeros(n, np.int32), obs_boxes=s["obs_boxes"][sel], K=s["K"])
        return plant(one, np.random.default_rng(0))
    return plant(ib.scene(name), np.random.default_rng(0))


# ---- steps 3 and 4 ---------------------------------------------------------------------------------------------------------------------
def kept_lines(boxes, rows=ib.ROWS, cols=ib.COLS):
    """(n, 4) bool: the lines init_batch_ref.plane_rows keeps; none for a detection with all four coordinates < 1"""
    d = np.asarray(boxes, float).reshape(-1, 4)
    lim = np.array([cols, rows, cols, rows], float)
    return (d > 0) & (d < lim - 1) & ~(d < 1).all(axis=1, keepdims=True)


def _rot(q):
    x, y, z, w = np.moveaxis(q, -1, 0)
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1).reshape(q.shape[:-1] + (3, 3))


def visible(Tcw, ell, K, bb, rows=ib.ROWS, cols=ib.COLS):
    """assoc2d_ref.visible for every row of Tcw (n, 7) against one ellipsoid, bb (n, 4) the raw boxes (NaN rows: no real outline)"""
    R, t = _rot(Tcw[:, 3:7]), Tcw[:, :3]
    pc = R @ ell[:3] + t
    front = ~(pc[:, 2] < 0)
    cam_w = -np.einsum("nji,nj->ni", R, t)
    xo = ((cam_w - ell[:3]) @ _rot(ell[3:7])) / ell[7:10]
    outside = ~((xo * xo).sum(axis=1) - 1.0 < 0)
    with np.errstate(all="ignore"):
        u, v = K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]
        inside = lambda a, b: (0 < a) & (a < cols) & (0 < b) & (b < rows)   # noqa: E731
        corner = ~np.isnan(bb[:, 0]) & (inside(bb[:, 0], bb[:, 1]) | inside(bb[:, 2], bb[:, 3]))
        return front & outside & (inside(u, v) | corner)


def residuals(Tcw, boxes, ell, K, rows=ib.ROWS, cols=ib.COLS):
    """r_i of step 4 for every entry of one object under one ellipsoid"""
    po = ib._po()
    Tcw = np.asarray(Tcw, float).reshape(-1, 7)
    Tcw = np.concatenate([Tcw[:, :3], Tcw[:, 3:] / np.linalg.norm(Tcw[:, 3:], axis=1, keepdims=True)], axis=1)
    d = np.asarray(boxes, float).reshape(-1, 4)
    keep = kept_lines(d, rows, cols)
    bb = np.array([po.project_bbox(T, ell, K) for T in Tcw]).reshape(-1, 4)
    with np.errstate(all="ignore"):
        r = np.where(keep, np.abs(bb - d), 0.0).max(axis=1)
    bad = ~keep.any(axis=1) | ~np.isfinite(bb).all(axis=1) | ~visible(Tcw, np.asarray(ell, float), K, bb, rows, cols)
    return np.where(bad, np.inf, r)


def score(r, inlier_px):
    inl = r <= inlier_px
    return inl, int(inl.sum()), float((r[inl] ** 2).sum())


def fit(Tcw, boxes, K, rows, cols, faithful):
    """(valid, planes, ellipsoid, Q*) of the plain SVD initialisation over these entries"""
    po = ib._po()
    planes = int(kept_lines(boxes, rows, cols).sum())
    if planes < 9:
        return False, planes, np.zeros(10), np.zeros((4, 4))
    Twc = np.array([po.se3_inv(T) for T in Tcw])
    e, Q, ok = po.init_quadric(Twc, boxes, K, rows, cols, faithful=faithful)
    return bool(ok), planes, e, Q


def better(a, b):
    """(n_in, cost) a is not worse than b"""
    return a[0] > b[0] or (a[0] == b[0] and a[1] <= b[1])


def reference(cams, N, obs_cam, obs_obj, obs_boxes, K, rows=ib.ROWS, cols=ib.COLS, faithful=0, min_observations=0, p=None, **_):
    """dict(ellipsoids (N, 10), qstar (N, 4, 4), plane_error (N,), stats (N, 8), inliers (n_obs,), residuals (n_obs,),
    hyp (N, H, 4), hyp_ell (N, H, 10), hyp_q (N, H, 4, 4), hyp_res: per object the (H_o, n) residuals; winner_res: per object the
    winner's residuals; runner_up: per object (n_in, cost) of the second-best valid hypothesis or None)"""
    p = params(**(p or {}))
    cams = np.asarray(cams, float).reshape(-1, 7)
    obs_cam, obs_obj, obs_boxes = np.asarray(obs_cam), np.asarray(obs_obj), np.asarray(obs_boxes, float).reshape(-1, 4)
    H, px = p["n_hypotheses"], p["inlier_px"]
    out = dict(ellipsoids=np.zeros((N, 10)), qstar=np.zeros((N, 4, 4)), plane_error=np.zeros(N), stats=np.zeros((N, 8), np.int32),
               inliers=np.zeros(len(obs_obj), np.int32), residuals=np.full(len(obs_obj), np.nan), hyp=np.zeros((N, H, 4)),
               hyp_ell=np.zeros((N, H, 10)), hyp_q=np.zeros((N, H, 4, 4)), hyp_res=[None] * N, winner_res=[None] * N, runner_up=[None] * N)
    st = out["stats"]
    st[:, 6] = -1
    for o, sel in enumerate(ib.group(obs_obj, N)):
        n = len(sel)
        st[o, 1] = n
        if n < min_observations:
            st[o, 0] = 1
            continue
        Tcw, boxes = cams[obs_cam[sel]], obs_boxes[sel]
        st[o, 2] = int(kept_lines(boxes, rows, cols).sum())
        if st[o, 2] < 9:
            st[o, 0] = 2
            continue
        best, ranked, allres = None, [], []
        for h in range(n_hypotheses(n, p["sample_size"], H)):
            loc = sample(p["seed"], h, n, p["sample_size"])
            ok, planes, e, Q = fit(Tcw[loc], boxes[loc], K, rows, cols, faithful)
            out["hyp"][o, h, :2] = ok, planes
            out["hyp_q"][o, h] = Q
            if not ok:
                allres.append(np.full(n, np.inf))
                continue
            r = residuals(Tcw, boxes, e, K, rows, cols)
            allres.append(r)
            inl, n_in, cost = score(r, px)
            out["hyp"][o, h, 2:] = n_in, cost
            out["hyp_ell"][o, h] = e
            ranked.append((-n_in, cost, h))
            if best is None or (-n_in, cost, h) < best[0]:
                best = ((-n_in, cost, h), e, Q, r, inl)
        out["hyp_res"][o] = np.array(allres)
        st[o, 5] = len(ranked)
        if best is None:
            st[o, 0] = 4
            continue
        (neg, cost, h), e, Q, r, inl = best
        ranked.sort()
        out["runner_up"][o] = (-ranked[1][0], ranked[1][1]) if len(ranked) > 1 else None
        out["winner_res"][o] = r
        st[o, 6], st[o, 4] = h, -neg
        if -neg < p["min_inliers"]:
            st[o, 0] = 5
            continue
        if p["refine"]:
            masked = np.where(inl, 0, -1)
            e2, Q2, _, st2 = ib.reference(Tcw, 1, np.arange(n), masked, boxes, K, rows, cols, faithful=faithful)
            st[o, 3] = int(inl.sum() > ib.TILE)
            if st2[0, 0] == 0:
                r2 = residuals(Tcw, boxes, e2[0], K, rows, cols)
                inl2, n2, cost2 = score(r2, px)
                if better((n2, cost2), (-neg, cost)):
                    e, Q, r, inl = e2[0], Q2[0], r2, inl2
                    st[o, 4], st[o, 7] = n2, 1
        out["ellipsoids"][o], out["qstar"][o] = e, Q
        out["plane_error"][o] = ib.plane_error(ib.plane_rows(Tcw[inl], boxes[inl], K, rows, cols), e)
        out["inliers"][sel], out["residuals"][sel] = inl, r
    return out


@functools.lru_cache(maxsize=None)
def scene_reference(name, faithful=0):
    s = planted_scene(name)
    return reference(s["cams"], s["N"], s["obs_cam"], s["obs_obj"], s["obs_boxes"], s["K"], faithful=faithful)


def cost_tolerance(s, ref):
    """How far a cost and a residual may move when the ellipsoid moves within what init_batch_ref.assert_values grants the device
    (centre 1e-8, half-axes 1e-6 relative).  Every object's winning hypothesis (the one with the most inliers, so the longest sum) is
    moved four ways -- the centre by +-1e-8 in all three coordinates, the half-axes by a factor 1 +- 1e-6 --; the largest change of
    its cost, and of any finite residual, over the scene, times 10.  Returns (cost tolerance px^2, residual tolerance px)."""
    worst_c, worst_r = 0.0, 0.0
    px = DEFAULTS["inlier_px"]
    for o, sel in enumerate(ib.group(s["obs_obj"], s["N"])):
        h = ref["stats"][o, 6]
        if h < 0:
            continue
        Tcw, boxes, e = s["cams"][s["obs_cam"][sel]], s["obs_boxes"][sel], ref["hyp_ell"][o, h]
        r0 = ref["hyp_res"][o][h]
        inl = r0 <= px
        for sc, sa in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            e2 = e.copy(); e2[:3] += sc * 1e-8; e2[7:] *= 1 + sa * 1e-6
            r = residuals(Tcw, boxes, e2, s["K"])
            fin = np.isfinite(r) & np.isfinite(r0)
            worst_r = max(worst_r, float(np.abs(r[fin] - r0[fin]).max()))
            worst_c = max(worst_c, abs(float((r[inl] ** 2).sum()) - float((r0[inl] ** 2).sum())))
    return 10 * worst_c, 10 * worst_r
