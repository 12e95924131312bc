"""esl_relocalize restated in numpy: the reference the device is compared with (tests/test_reloc_ref.py, tests/test_gpu_reloc.py).

Camera pose and detection -> map association of one frame against a fixed map, with no pose prior: both sides are moved into
their gravity frames (ground plane = z 0), every pair of gated (detection, map object) candidates is a planar-motion hypothesis,
every hypothesis is scored against every detection, the winner of the total order (inliers, cost, key) is re-fitted in closed
form and the detections are associated one to one under the final pose.  Loops are fine here; only the pair gate is vectorised.

Every quantity that is compared against a threshold also records how close it came (`margin`: smallest relative distance to
a threshold), and the winner records its distance to the runner-up (`runner_gap`): an implementation in other arithmetic can be
expected to return the same integers only where both are far above rounding."""
import numpy as np

DEFAULTS = dict(center_tol=0.25, height_tol=0.25, size_ratio=1.5, min_baseline=0.5, min_inliers=3, max_candidates=4096,
                match_labels=1, refine=1)


def gravity_frame(plane):
    """(A, d): G(x) = A x + (0, 0, d) with rows u, v, n of A; third coordinate = height above the plane."""
    plane = np.asarray(plane, dtype=np.float64)
    nn = np.sqrt(plane[0] * plane[0] + plane[1] * plane[1] + plane[2] * plane[2])
    n = plane[:3] / nn
    d = plane[3] / nn
    k = int(np.argmin(np.abs(n)))          # first smallest |n_k|
    e = np.zeros(3); e[k] = 1.0
    u = np.cross(e, n)
    u = u / np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    v = np.cross(n, u)
    return np.stack([u, v, n]), d


def prep(objs, A, d):
    """gravity-frame (x, y, height) of the centres and the half-axes sorted ascending"""
    objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    g = objs[:, :3] @ A.T
    g[:, 2] += d
    return g, np.sort(objs[:, 7:10], axis=1)


def rot_to_quat(R):
    """x y z w with w >= 0 (largest-component branch)"""
    ww = 1 + R[0, 0] + R[1, 1] + R[2, 2]
    xx = 1 + R[0, 0] - R[1, 1] - R[2, 2]
    yy = 1 - R[0, 0] + R[1, 1] - R[2, 2]
    zz = 1 - R[0, 0] - R[1, 1] + R[2, 2]
    k = int(np.argmax([ww, xx, yy, zz]))
    if k == 0:
        s = 2 * np.sqrt(ww); q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, s / 4]
    elif k == 1:
        s = 2 * np.sqrt(xx); q = [s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif k == 2:
        s = 2 * np.sqrt(yy); q = [(R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = 2 * np.sqrt(zz); q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4, (R[1, 0] - R[0, 1]) / s]
    q = np.array(q)
    if q[3] < 0:
        q = -q
    return q / np.sqrt((q * q).sum())


def pose_from_planar(Aw, dw, Ac, dc, yaw, tx, ty):
    """Twc (x y z qx qy qz qw) of x_w = G_w^-1(Z(yaw, t) G_c(x_c))"""
    c, s = np.cos(yaw), np.sin(yaw)
    Z = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    R = Aw.T @ Z @ Ac
    t = Aw.T @ np.array([tx, ty, dc - dw])
    return np.concatenate([t, rot_to_quat(R)])


class _Margin:
    def __init__(self):
        self.v = np.inf

    def note(self, x, thr):
        x = np.asarray(x, dtype=np.float64)
        if x.size:
            with np.errstate(invalid="ignore"):
                r = np.abs(x - thr) / max(abs(thr), 1e-300)
            r = r[np.isfinite(r)]
            if r.size:
                self.v = min(self.v, float(r.min()))


def _better(a, b):
    """(n, cost, key) total order: more inliers, then lower cost, then lower key"""
    if a[0] != b[0]:
        return a[0] > b[0]
    if a[1] != b[1]:
        return a[1] < b[1]
    return a[2] < b[2]


def relocalize(map_objs, map_labels, ground_world, det_objs, det_labels, ground_cam, params=None):
    P_ = dict(DEFAULTS)
    if params:
        P_.update(params)
    tol, tol2 = float(P_["center_tol"]), float(P_["center_tol"]) ** 2
    map_objs = np.asarray(map_objs, dtype=np.float64).reshape(-1, 10)
    det_objs = np.asarray(det_objs, dtype=np.float64).reshape(-1, 10)
    map_labels = np.asarray(map_labels, dtype=np.int64).reshape(-1)
    det_labels = np.asarray(det_labels, dtype=np.int64).reshape(-1)
    M, D = len(map_objs), len(det_objs)
    Aw, dw = gravity_frame(ground_world)
    Ac, dc = gravity_frame(ground_cam)
    pm, sm = prep(map_objs, Aw, dw)
    qd, sd = prep(det_objs, Ac, dc)
    mg = _Margin()
    out = dict(status=1, n_candidates=0, n_hypotheses=0, best_key=-1, n_inliers=0, refined=0, cost=0.0, yaw=0.0, tx=0.0, ty=0.0,
               Twc=np.array([0, 0, 0, 0, 0, 0, 1.0]), assoc=-np.ones(D, dtype=np.int32), margin=np.inf, runner_gap=np.inf,
               refine_gap=np.inf)

    # ---- 2. candidates, (d, m) lexicographic, CSR by detection
    cd, cm = [], []
    row = [0]
    for d in range(D):
        if M:
            ok = np.ones(M, dtype=bool)
            if P_["match_labels"]:
                ok &= map_labels == det_labels[d]
            dh = np.abs(qd[d, 2] - pm[:, 2])
            mg.note(dh, P_["height_tol"])
            ok &= dh <= P_["height_tol"]
            if P_["size_ratio"] > 1:
                with np.errstate(invalid="ignore", divide="ignore"):
                    lr = np.abs(np.log(sd[d][None, :] / sm)).max(axis=1)
                thr = np.log(P_["size_ratio"])
                mg.note(lr, thr)
                ok &= (lr <= thr) & (sd[d, 0] > 0) & (sm[:, 0] > 0)   # a non-positive or NaN half-axis fails
            for m in np.nonzero(ok)[0]:
                cd.append(d); cm.append(int(m))
        row.append(len(cd))
    cd, cm = np.array(cd, dtype=np.int64), np.array(cm, dtype=np.int64)
    P = len(cd)
    out["n_candidates"] = P
    out["margin"] = mg.v
    if P > P_["max_candidates"]:
        out["status"] = 3
        return out
    if P < 2:
        return out
    cq = qd[cd, :2]          # detection side of every candidate
    cp = pm[cm, :2]          # map side

    # ---- 3. hypotheses: i < j, different detections, different map objects, baseline and length consistency
    ii, jj = np.triu_indices(P, 1)
    keep = (cd[ii] != cd[jj]) & (cm[ii] != cm[jj])
    ii, jj = ii[keep], jj[keep]
    dq = cq[jj] - cq[ii]
    dp = cp[jj] - cp[ii]
    lq = np.sqrt(dq[:, 0] * dq[:, 0] + dq[:, 1] * dq[:, 1])
    lp = np.sqrt(dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1])
    mg.note(lq, P_["min_baseline"])
    mg.note(np.abs(lq - lp), 2 * tol)
    keep = (lq >= P_["min_baseline"]) & (np.abs(lq - lp) <= 2 * tol)
    ii, jj, dq, dp = ii[keep], jj[keep], dq[keep], dp[keep]
    out["n_hypotheses"] = int(len(ii))
    out["margin"] = mg.v
    if len(ii) == 0:
        return out

    def motion(i, j):
        psi = np.arctan2(cp[j, 1] - cp[i, 1], cp[j, 0] - cp[i, 0]) - np.arctan2(cq[j, 1] - cq[i, 1], cq[j, 0] - cq[i, 0])
        c, s = np.cos(psi), np.sin(psi)
        mqx, mqy = 0.5 * (cq[i, 0] + cq[j, 0]), 0.5 * (cq[i, 1] + cq[j, 1])
        mpx, mpy = 0.5 * (cp[i, 0] + cp[j, 0]), 0.5 * (cp[i, 1] + cp[j, 1])
        return psi, mpx - (c * mqx - s * mqy), mpy - (s * mqx + c * mqy)

    def dist2(psi, tx, ty):
        """squared planar distance of every candidate's moved detection centre to its map centre"""
        c, s = np.cos(psi), np.sin(psi)
        ex = c * cq[:, 0] - s * cq[:, 1] + tx - cp[:, 0]
        ey = s * cq[:, 0] + c * cq[:, 1] + ty - cp[:, 1]
        return ex * ex + ey * ey

    def score(psi, tx, ty, note=True):
        """(n, cost, nearest candidate per detection or -1)"""
        d2 = dist2(psi, tx, ty)
        n, cost, near = 0, 0.0, -np.ones(D, dtype=np.int64)
        for d in range(D):
            if row[d + 1] > row[d]:
                k = row[d] + int(np.argmin(d2[row[d]:row[d + 1]]))
                if note:
                    mg.note(d2[k], tol2)
                if d2[k] <= tol2:
                    n += 1; cost += d2[k]; near[d] = k
        return n, cost, near

    # ---- 4. score; winner = max n, min cost, min key
    best, second = None, None
    for i, j in zip(ii, jj):
        psi, tx, ty = motion(i, j)
        n, cost, _ = score(psi, tx, ty)
        cur = (n, cost, int(i) * P + int(j))
        if best is None or _better(cur, best):
            best, second = cur, best
        elif second is None or _better(cur, second):
            second = cur
    out["margin"] = mg.v
    if second is not None and second[0] == best[0]:
        out["runner_gap"] = abs(second[1] - best[1]) / max(best[1], second[1], 1e-300)
    out["best_key"] = best[2]
    bi, bj = best[2] // P, best[2] % P
    psi, tx, ty = motion(bi, bj)
    n0, cost0, near = score(psi, tx, ty, note=False)
    if n0 < P_["min_inliers"]:
        out.update(status=2, n_inliers=n0, cost=cost0)
        return out

    # ---- 5. closed-form planar re-fit over the winner's inlier pairs (two pairs already are their own fit: nothing to do below 3)
    if P_["refine"] and n0 >= 3:
        ks = near[near >= 0]
        mq, mp = cq[ks].mean(axis=0), cp[ks].mean(axis=0)
        a, b = cq[ks] - mq, cp[ks] - mp
        sc = (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]).sum()
        sdot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).sum()
        psi1 = np.arctan2(sc, sdot)
        c, s = np.cos(psi1), np.sin(psi1)
        tx1, ty1 = mp[0] - (c * mq[0] - s * mq[1]), mp[1] - (s * mq[0] + c * mq[1])
        n1, cost1, _ = score(psi1, tx1, ty1)
        out["margin"] = mg.v
        if n1 == n0:
            out["refine_gap"] = abs(cost1 - cost0) / max(cost0, cost1, 1e-300)
        if n1 > n0 or (n1 == n0 and cost1 <= cost0):
            psi, tx, ty = psi1, tx1, ty1
            out["refined"] = 1

    # ---- 6. association under the final pose: detections in index order, nearest unclaimed candidate within center_tol
    d2 = dist2(psi, tx, ty)
    claimed = set()
    n, cost = 0, 0.0
    for d in range(D):
        bk, bd = -1, np.inf
        for k in range(row[d], row[d + 1]):
            if int(cm[k]) not in claimed and d2[k] < bd:
                bk, bd = k, d2[k]
        if bk >= 0:
            mg.note(bd, tol2)
            if bd <= tol2:
                claimed.add(int(cm[bk])); out["assoc"][d] = cm[bk]; n += 1; cost += bd
    out["margin"] = mg.v
    yaw = np.arctan2(np.sin(psi), np.cos(psi))
    out.update(status=0, n_inliers=n, cost=cost, yaw=float(yaw), tx=float(tx), ty=float(ty),
               Twc=pose_from_planar(Aw, dw, Ac, dc, yaw, tx, ty))
    return out
