"""The numpy statement of esl_dense_normals and esl_dense_align_frames (include/esl.h, "normals of the dense map" steps N1 to N5 and
"aligning frames to the dense map" steps a to e), on top of tests/dense_ref.py: the map is what DenseMap.extract() lists (live voxels in
ascending packed-key order).  The arithmetic follows csrc/esl_dense_align.hpp operation by operation -- the device is compared with it
byte for byte -- so nothing here may be "simplified": sums run in the header's order, one product and one add at a time; the 6 x 6
solve and the pose update are plain Python floats (IEEE doubles, no contraction).  Test infrastructure only: nothing here is imported
by the package."""
import math

import numpy as np

import dense_ref as dr

FIX = dr.FIX
SWEEPS = 8
NORMAL_DEFAULTS = dict(max_curvature=0.05, radius=1, min_count=1, min_neighbors=5)
ALIGN_DEFAULTS = dict(max_dist=0.0, damping=0.0, min_pivot_ratio=1e-6, tol_t=1e-5, tol_r=1e-5, iters=4, stride=2, reach=1, min_inliers=100)
COUNTS = ("n_sampled", "n_zero", "n_depth_out", "n_key_out", "n_used", "n_nomatch", "n_far", "n_inlier")
ROW = 37
MAX_ITERS, CONVERGED, TOO_FEW, DEGENERATE = 0, 1, 2, 3


def offsets(reach):
    """the (2 reach + 1)^3 key offsets in ascending (kx, ky, kz), i.e. ascending packed-key order"""
    r = range(-reach, reach + 1)
    return [(dx, dy, dz) for dx in r for dy in r for dz in r]


def lookup(keys_sorted, k):
    """(n, 3) integer keys -> index into the ascending packed keys, -1 where absent or out of range"""
    k = np.asarray(k, dtype=np.int64)
    inr = (np.abs(k) <= dr.KEY_MAX).all(axis=-1)
    pk = dr.pack(np.where(inr[:, None], k, 0))
    if not len(keys_sorted):
        return np.full(len(k), -1, np.int64)
    pos = np.minimum(np.searchsorted(keys_sorted, pk), len(keys_sorted) - 1)
    return np.where(inr & (keys_sorted[pos] == pk), pos, -1).astype(np.int64)


def jacobi_min(C):
    """dense_planes_ref.jacobi_min over rows: C (n, 6) -> (n, 3), the same operations in the same order (a skipped pivot keeps its
    values)"""
    C = np.asarray(C, dtype=np.float64)
    n = len(C)
    idx = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
    a = [[C[:, idx[r][c]].copy() for c in range(3)] for r in range(3)]
    v = [[np.full(n, 1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = a[p][q]
                on = apq != 0
                theta = (a[q][q] - a[p][p]) / (2 * apq)
                t = 1 / (np.abs(theta) + np.sqrt(theta * theta + 1))
                t = np.where(theta < 0, -t, t)
                c = 1 / np.sqrt(t * t + 1); s = t * c
                for k in range(3):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p] = np.where(on, c * akp - s * akq, akp); a[k][q] = np.where(on, s * akp + c * akq, akq)
                for k in range(3):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k] = np.where(on, c * apk - s * aqk, apk); a[q][k] = np.where(on, s * apk + c * aqk, aqk)
                for k in range(3):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = np.where(on, c * vkp - s * vkq, vkp); v[k][q] = np.where(on, s * vkp + c * vkq, vkq)
        lo = a[0][0].copy()
        w = [v[0][0].copy(), v[1][0].copy(), v[2][0].copy()]
        for e in (1, 2):
            less = a[e][e] < lo
            lo = np.where(less, a[e][e], lo)
            w = [np.where(less, v[r][e], w[r]) for r in range(3)]
        nn = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        return np.stack([w[0] / nn, w[1] / nn, w[2] / nn], axis=-1)


def normals(ext, cap=None, **over):
    """steps N1 to N5 on an extract (key, xyz, count of the live voxels in ascending key order) -> dict(result, normal, curvature,
    neighbors, valid, and C (n, 6) / trace for the tests)"""
    p = dict(NORMAL_DEFAULTS); p.update(over)
    if ext["n_voxels"] < 0:
        return dict(result=dict(status=ext.get("status", 3), n_voxels=-1, n_eligible=0, n_valid=0))
    n = ext["n_voxels"]
    key = np.asarray(ext["key"], dtype=np.int64).reshape(n, 3)
    c = np.asarray(ext["xyz"], dtype=np.float64).reshape(n, 3)
    packed = dr.pack(key) if n else np.zeros(0, np.uint64)
    elig = np.asarray(ext["count"]).reshape(n) >= p["min_count"]
    m = np.zeros(n, np.int64)
    s = [np.zeros(n) for _ in range(3)]
    M = [np.zeros(n) for _ in range(6)]
    for off in offsets(p["radius"]):
        j = lookup(packed, key + np.asarray(off, dtype=np.int64))
        has = elig & (j >= 0) & elig[np.maximum(j, 0)]
        cj = c[np.maximum(j, 0)]
        d = [cj[:, a] - c[:, a] for a in range(3)]
        for a in range(3):
            s[a] = np.where(has, s[a] + d[a], s[a])
        e = 0
        for a in range(3):
            for b in range(a, 3):
                M[e] = np.where(has, M[e] + d[a] * d[b], M[e])
                e += 1
        m += has
    with np.errstate(all="ignore"):
        dm = m.astype(np.float64)
        u = [s[a] / dm for a in range(3)]
        C = np.stack([M[0] / dm - u[0] * u[0], M[1] / dm - u[0] * u[1], M[2] / dm - u[0] * u[2],
                      M[3] / dm - u[1] * u[1], M[4] / dm - u[1] * u[2], M[5] / dm - u[2] * u[2]], axis=-1)
        trace = (C[:, 0] + C[:, 3]) + C[:, 5]
        run = elig & (m >= 1) & (m >= p["min_neighbors"]) & (trace > 0)
        w = jacobi_min(np.where(run[:, None], C, np.array([1.0, 0, 0, 2.0, 0, 3.0])))
        first = np.where(w[:, 0] != 0, w[:, 0], np.where(w[:, 1] != 0, w[:, 1], w[:, 2]))
        w = np.where((first < 0)[:, None], -w, w)
        c0 = (C[:, 0] * w[:, 0] + C[:, 1] * w[:, 1]) + C[:, 2] * w[:, 2]
        c1 = (C[:, 1] * w[:, 0] + C[:, 3] * w[:, 1]) + C[:, 4] * w[:, 2]
        c2 = (C[:, 2] * w[:, 0] + C[:, 4] * w[:, 1]) + C[:, 5] * w[:, 2]
        lam = (w[:, 0] * c0 + w[:, 1] * c1) + w[:, 2] * c2
        cv = lam / trace
        valid = run & (cv <= p["max_curvature"])
    normal = np.where(valid[:, None], w, 0.0)
    curv = np.where(valid, cv, np.nan)
    k = n if cap is None else min(int(cap), n)
    return dict(result=dict(status=0, n_voxels=n, n_eligible=int(elig.sum()), n_valid=int(valid.sum())),
                normal=normal[:k], curvature=curv[:k], neighbors=m.astype(np.int32)[:k], valid=valid.astype(np.uint8)[:k], C=C, trace=trace)


def max_dist2(p, leaf):
    d = p["max_dist"] if p["max_dist"] > 0 else float(p["reach"] + 1) * leaf
    return d * d


def bound(K, rows, cols, depth_max, md2):
    """step c: Q"""
    fx, fy, cx, cy = (float(v) for v in K)
    x = max(abs(0.0 - cx), abs(float(cols - 1) - cx)) / fx
    y = max(abs(0.0 - cy), abs(float(rows - 1) - cy)) / fy
    far = abs(depth_max) * math.sqrt((1.0 + x * x) + y * y)
    return max(max(1.0, far), math.sqrt(md2)) * (1.0 + 1.0 / 1048576.0)


def sums_fit(n_sampled, Q):
    return float(n_sampled) * (Q * Q * FIX + 1.0) < 4611686018427387904.0


def centre(cam):
    """step c: o = R^T (0 - t), dense_world's operations"""
    R, t = dr.pose(cam)
    d = [0.0 - float(t[0]), 0.0 - float(t[1]), 0.0 - float(t[2])]
    return [(float(R[0, a]) * d[0] + float(R[1, a]) * d[1]) + float(R[2, a]) * d[2] for a in range(3)]


def match(pw, k, ext_keys, xyz, valid, reach):
    """step b -> (best index or -1, best d2)"""
    n = len(pw)
    best = np.full(n, -1, np.int64); best_d2 = np.zeros(n)
    for off in offsets(reach):
        j = lookup(ext_keys, k + np.asarray(off, dtype=np.int64))
        cand = (j >= 0) & (valid[np.maximum(j, 0)] != 0) if len(valid) else np.zeros(n, bool)
        cj = xyz[np.maximum(j, 0)] if len(xyz) else np.zeros((n, 3))
        r = [pw[:, a] - cj[:, a] for a in range(3)]
        d2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
        take = cand & ((best < 0) | (d2 < best_d2))
        best = np.where(take, j, best); best_d2 = np.where(take, d2, best_d2)
    return best, best_d2


def terms(pw, o, c, n):
    """step c: the 28 fixed-point terms of every inlier, (n, 28) int64"""
    q = [pw[:, a] - o[a] for a in range(3)]
    r = [pw[:, a] - c[:, a] for a in range(3)]
    e = (n[:, 0] * r[0] + n[:, 1] * r[1]) + n[:, 2] * r[2]
    J = [n[:, 0], n[:, 1], n[:, 2], q[1] * n[:, 2] - q[2] * n[:, 1], q[2] * n[:, 0] - q[0] * n[:, 2], q[0] * n[:, 1] - q[1] * n[:, 0]]
    cols = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * e for a in range(6)] + [e * e]
    return np.stack([np.rint(x * FIX).astype(np.int64) for x in cols], axis=-1) if len(pw) else np.zeros((0, 28), np.int64)


def accumulate(ext, nrm, leaf, mp, cam, K, rows, cols, depth, p, detail=False):
    """steps a to c of one frame at one pose -> the row of 37 int64"""
    s = dr.samples(cam, K, rows, cols, depth, dict(mp, stride=p["stride"], leaf=leaf))
    row = np.zeros(ROW, np.int64)
    cn = s["counts"]
    row[29:34] = [cn["n_sampled"], cn["n_zero"], cn["n_depth_out"], cn["n_key_out"], cn["n_used"]]
    n = ext["n_voxels"]
    keys = dr.pack(np.asarray(ext["key"], dtype=np.int64).reshape(n, 3)) if n else np.zeros(0, np.uint64)
    xyz = np.asarray(ext["xyz"], dtype=np.float64).reshape(n, 3)
    best, d2 = match(s["pw"], s["k"], keys, xyz, nrm["valid"], p["reach"])
    far = (best >= 0) & (d2 > max_dist2(p, leaf))
    inl = (best >= 0) & ~far
    row[34:37] = [int((best < 0).sum()), int(far.sum()), int(inl.sum())]
    T = terms(s["pw"][inl], centre(cam), xyz[best[inl]], nrm["normal"][best[inl]])
    row[:28] = T.sum(axis=0, dtype=np.int64)
    row[28] = int(inl.sum())
    if detail:
        return row, dict(samples=s, best=best, d2=d2, inlier=inl, terms=T)
    return row


def system(row):
    """step d: H (6 x 6 lists) and g"""
    H = [[0.0] * 6 for _ in range(6)]
    k = 0
    for a in range(6):
        for b in range(a, 6):
            v = float(int(row[k])) / FIX
            H[a][b] = v; H[b][a] = v
            k += 1
    return H, [float(int(row[21 + a])) / FIX for a in range(6)]


def solve(H, g, n_inlier, p):
    """step d -> (0 / TOO_FEW / DEGENERATE, delta)"""
    delta = [0.0] * 6
    if n_inlier < p["min_inliers"]:
        return TOO_FEW, delta
    A = [list(r) for r in H]
    L = [[0.0] * 6 for _ in range(6)]
    dmax = 0.0
    for a in range(6):
        A[a][a] = H[a][a] + p["damping"] * H[a][a]
        if a == 0 or A[a][a] > dmax:
            dmax = A[a][a]
    floor_ = p["min_pivot_ratio"] * dmax
    for j in range(6):
        piv = A[j][j]
        for k in range(j):
            piv = piv - L[j][k] * L[j][k]
        if not piv > 0 or not piv >= floor_:
            return DEGENERATE, delta
        ljj = math.sqrt(piv)
        L[j][j] = ljj
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / ljj
    y = [0.0] * 6
    for i in range(6):
        v = -g[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * delta[k]
        delta[i] = v / L[i][i]
    if not all(math.isfinite(x) for x in delta):
        return DEGENERATE, [0.0] * 6
    return 0, delta


def norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def update(cam, delta):
    """step d: the pose after delta = (v, omega), or None when it is not a valid pose"""
    cam = [float(x) for x in cam]
    try:
        o = centre(cam)
    except dr.InvalidPose:
        return None
    nrm = math.sqrt(cam[3] * cam[3] + cam[4] * cam[4] + cam[5] * cam[5] + cam[6] * cam[6])
    ax, ay, az, aw = cam[3] / nrm, cam[4] / nrm, cam[5] / nrm, cam[6] / nrm
    hx, hy, hz = delta[3] / 2, delta[4] / 2, delta[5] / 2
    dn = math.sqrt(((hx * hx + hy * hy) + hz * hz) + 1.0)
    bx, by, bz, bw = -(hx / dn), -(hy / dn), -(hz / dn), 1.0 / dn
    c = [0.0] * 7
    c[3] = ((aw * bx + ax * bw) + ay * bz) - az * by
    c[4] = ((aw * by - ax * bz) + ay * bw) + az * bx
    c[5] = ((aw * bz + ax * by) - ay * bx) + az * bw
    c[6] = ((aw * bw - ax * bx) - ay * by) - az * bz
    try:
        R, _ = dr.pose(c)
    except dr.InvalidPose:
        return None
    R = [[float(R[i, j]) for j in range(3)] for i in range(3)]
    o0, o1, o2 = o[0] + delta[0], o[1] + delta[1], o[2] + delta[2]
    for a in range(3):
        c[a] = -((R[a][0] * o0 + R[a][1] * o1) + R[a][2] * o2)
    if not all(math.isfinite(x) for x in c):
        return None
    return c


def align(ext, leaf, map_params, cams, K, rows, cols, depth, **over):
    """esl_dense_align_frames on an extract of the map -> dict(result, cams, status, iters, counts, sum_e2, H, step, sums)"""
    p = dict(ALIGN_DEFAULTS); p.update({k: v for k, v in over.items() if k in ALIGN_DEFAULTS})
    np_over = {k: v for k, v in over.items() if k in NORMAL_DEFAULTS}
    unknown = set(over) - set(ALIGN_DEFAULTS) - set(NORMAL_DEFAULTS)
    if unknown:
        raise KeyError(sorted(unknown))
    if ext["n_voxels"] < 0:
        return dict(result=dict(status=ext.get("status", 3), n_voxels=-1, n_valid=0, n_passes=0))
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    F = len(cams)
    for c in cams:
        dr.pose(c)
    mp = dict(dr.DEFAULTS); mp.update(map_params)
    srows, scols = (rows + p["stride"] - 1) // p["stride"], (cols + p["stride"] - 1) // p["stride"]
    if srows * scols * F >= 1 << 31 or not sums_fit(srows * scols, bound(K, rows, cols, mp["depth_max"], max_dist2(p, leaf))):
        raise ValueError("the call is refused: ESL_ERR_INVALID")
    nrm = normals(ext, **np_over)
    iters = p["iters"]
    out = dict(cams=np.zeros((F, 7)), status=np.zeros(F, np.int32), iters=np.zeros(F, np.int32), counts=np.zeros((F, 8), np.int64),
               sum_e2=np.zeros(F), H=np.zeros((F, 6, 6)), step=np.zeros((F, 2)), sums=np.zeros((F, iters + 1, ROW), np.int64))
    passes = 0
    for f in range(F):
        cam = [float(x) for x in cams[f]]
        last = False
        for it in range(iters + 1):
            row = accumulate(ext, nrm, leaf, mp, cam, K, rows, cols, np.asarray(depth)[f], p)
            passes = max(passes, it + 1)
            out["sums"][f, it] = row
            H, g = system(row)
            stop = last or it == iters
            if not stop:
                st, delta = solve(H, g, int(row[36]), p)
                nxt = update(cam, delta) if st == 0 else None
                if st == 0 and nxt is None:
                    st = DEGENERATE
                if st != 0:
                    out["status"][f] = st; stop = True
                else:
                    cam = nxt
                    out["iters"][f] += 1
                    out["step"][f] = [norm3(delta[:3]), norm3(delta[3:])]
                    if norm3(delta[:3]) <= p["tol_t"] and norm3(delta[3:]) <= p["tol_r"]:
                        out["status"][f] = CONVERGED; last = True
            if stop:
                out["counts"][f] = row[29:37]
                out["sum_e2"][f] = float(int(row[27])) / FIX
                out["H"][f] = np.array(H)
                break
        out["cams"][f] = cam
    out["result"] = dict(status=0, n_voxels=ext["n_voxels"], n_valid=nrm["result"]["n_valid"], n_passes=passes)
    return out


def pose_error(cam, cam_true):
    """(distance of the camera centres, rotation angle between the two poses) -- for the convergence test, ordinary float maths"""
    Ra, _ = dr.pose(cam); Rb, _ = dr.pose(cam_true)
    oa, ob = np.array(centre(cam)), np.array(centre(cam_true))
    cosang = (np.trace(Ra @ Rb.T) - 1) / 2
    return float(np.linalg.norm(oa - ob)), float(np.arccos(np.clip(cosang, -1, 1)))
