"""The numpy statement of esl_dense_planes (include/esl.h, "dominant planes and the ground from the dense map", steps 1-9) on top of
dense_ref.DenseMap.extract().  Where the library runs on the host (the hypotheses' planes, the Jacobi, the refit, the orientations, the
ground) the arithmetic is in Python floats, operation by operation as csrc/esl_dense_planes.hpp has it, so the bits agree; the score
over the list is vectorised with the same parenthesisation.  Test infrastructure only: nothing here is imported by the package."""
import math

import numpy as np

import dense_ref as dr

DEFAULTS = dict(dist_tol=0.02, up=(0.0, 0.0, 0.0), up_min_cos=0.7071067811865476, n_hypotheses=1024, max_planes=8, min_inliers=1000,
                min_baseline=8, min_count=1, skip_labelled=0, refine=1, seed=0)
RESULT = ("status", "n_voxels", "n_eligible", "n_planes", "n_assigned", "ground_index", "rounds", "stop_reason")
GUARD = 1 << 62
SWEEPS = 8
M64 = (1 << 64) - 1


def mix(seed, r, n_hyp, h, k):
    """step 3: the splitmix64 finaliser of seed ^ (golden ratio * (4 (r n_hyp + h) + k + 1)), in Python integers mod 2^64"""
    z = (seed ^ (0x9E3779B97F4A7C15 * ((4 * (r * n_hyp + h) + k + 1) & M64))) & M64
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def index(seed, r, n_hyp, h, k, n_r):
    return (mix(seed, r, n_hyp, h, k) >> 11) % n_r


def proj(a, x):
    return (a[0] * x[0] + a[1] * x[1]) + a[2] * x[2]


def hypothesis(i, a, b, c, min_baseline, leaf):
    """step 3 -> [n^0, n^1, n^2, d^] or None; i = the three indices, a, b, c = the three keys (Python integers)"""
    if i[0] == i[1] or i[0] == i[2] or i[1] == i[2]:
        return None
    cheb = lambda p, q: max(abs(p[0] - q[0]), abs(p[1] - q[1]), abs(p[2] - q[2]))          # noqa: E731
    if cheb(a, b) < min_baseline or cheb(a, c) < min_baseline or cheb(b, c) < min_baseline:
        return None
    u = [b[e] - a[e] for e in range(3)]; v = [c[e] - a[e] for e in range(3)]
    N = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    n0, n1, n2 = float(N[0]), float(N[1]), float(N[2])
    norm = math.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    if norm < 0.5 * (float(min_baseline) * float(min_baseline)):
        return None
    n = [n0 / norm, n1 / norm, n2 / norm]
    x = [(float(a[e]) + 0.5) * leaf for e in range(3)]
    return n + [-proj(n, x)]


def heights(pl, X):
    """step 4 over the centres X (m, 3)"""
    return (pl[0] * X[:, 0] + pl[1] * X[:, 1]) + pl[2] * X[:, 2] + pl[3]


def score(pl, X, count, tol):
    inl = np.abs(heights(pl, X)) <= tol
    return inl, int(inl.sum()), int(count[inl].sum())


def guard(n, span):
    return n * span * span >= GUARD


def jacobi_min(C):
    """step 6: the re-normalised eigenvector of the smallest eigenvalue of the symmetric C = [c00, c01, c02, c11, c12, c22]"""
    C = [float(x) for x in C]          # Python floats: an overflowing theta^2 is an infinity without a warning, as in C
    a = [[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = a[p][q]
            if apq == 0:
                continue
            theta = (a[q][q] - a[p][p]) / (2 * apq)
            t = 1 / (abs(theta) + math.sqrt(theta * theta + 1))
            if theta < 0:
                t = -t
            c = 1 / math.sqrt(t * t + 1); s = t * c
            for k in range(3):
                akp, akq = a[k][p], a[k][q]
                a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq
            for k in range(3):
                apk, aqk = a[p][k], a[q][k]
                a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk
            for k in range(3):
                vkp, vkq = v[k][p], v[k][q]
                v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq
    k = 0
    for e in (1, 2):
        if a[e][e] < a[k][k]:
            k = e
    w = [v[0][k], v[1][k], v[2][k]]
    nn = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    return [w[0] / nn, w[1] / nn, w[2] / nn]


def moments(keys, count, kmin):
    """the eleven integers n, samples, s (3), M (xx xy xz yy yz zz) of the voxels `keys` relative to kmin, Python integers"""
    d = (np.asarray(keys, dtype=np.int64) - np.asarray(kmin, dtype=np.int64)).astype(object)
    mom = [len(d), int(np.asarray(count, dtype=np.int64).astype(object).sum())] + [int(d[:, a].sum()) for a in range(3)]
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        mom.append(int((d[:, a] * d[:, b]).sum()))
    return mom


def centroid(mom, kmin, leaf):
    dn = float(mom[0])
    return [(float(kmin[a]) + float(mom[2 + a]) / dn + 0.5) * leaf for a in range(3)]


def refit(mom, kmin, leaf):
    dn = float(mom[0])
    m = [float(mom[2]) / dn, float(mom[3]) / dn, float(mom[4]) / dn]
    C = [float(mom[5]) / dn - m[0] * m[0], float(mom[6]) / dn - m[0] * m[1], float(mom[7]) / dn - m[0] * m[2],
         float(mom[8]) / dn - m[1] * m[1], float(mom[9]) / dn - m[1] * m[2], float(mom[10]) / dn - m[2] * m[2]]
    n = jacobi_min(C)
    return n + [-proj(n, centroid(mom, kmin, leaf))]


def orient_out(pl):
    """step 8"""
    flip = pl[3] < 0
    if pl[3] == 0:
        for a in range(3):
            if pl[a] != 0:
                flip = pl[a] < 0
                break
    return [-x for x in pl] if flip else list(pl)


def up_unit(up):
    up = [float(x) for x in up]
    if up[0] == 0 and up[1] == 0 and up[2] == 0:
        return None
    nn = math.sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2])
    return [up[0] / nn, up[1] / nn, up[2] / nn]


def ground(planes, n_in, uh, up_min_cos):
    """step 9 -> (ground_index, ground plane (4 floats, zero without one))"""
    g = -1
    for p, pl in enumerate(planes):
        if not abs(proj(pl, uh)) >= up_min_cos:
            continue
        if g < 0 or n_in[p] > n_in[g]:
            g = p
    if g < 0:
        return -1, [0.0] * 4
    pl = list(planes[g])
    return g, ([-x for x in pl] if proj(pl, uh) < 0 else pl)


def winner(rows):
    """step 5 on a round's rows (valid, inlier voxels, inlier samples): the valid row with the most voxels, then the most samples, then
    the smallest index; None when no row is valid"""
    best = None
    for h, (valid, n_in, smp) in enumerate(rows):
        if valid and (best is None or (n_in, smp) > (rows[best][1], rows[best][2])):          # ascending h: a tie keeps the smaller h
            best = h
    return best


def refit_kept(n2, s2, win_n, win_s):
    """step 6: the refit is kept with no fewer inlier voxels, and with as many no fewer samples"""
    return (n2, s2) >= (win_n, win_s)


def planes(ext, leaf, voxel_cap=None, **over):
    """ext = DenseMap.extract() (all voxels).  Returns what Context.dense_planes(hyp=True) returns."""
    p = dict(DEFAULTS); p.update(over)
    Hn, P = p["n_hypotheses"], p["max_planes"]
    res = dict.fromkeys(RESULT, 0)
    if ext["n_voxels"] < 0:
        res.update(status=3, n_voxels=-1)
        return dict(result=res, planes=np.zeros((0, 4)), centroid=np.zeros((0, 3)), stats=np.zeros((0, 8), np.int32), samples=np.zeros(0, np.int64),
                    ground=np.zeros(4), voxel_plane=np.zeros(0, np.int32), hyp=np.zeros((0, Hn, 3), np.int64))
    V = ext["n_voxels"]
    res.update(n_voxels=V, ground_index=-1, stop_reason=1)
    voxel_cap = V if voxel_cap is None else voxel_cap
    out_pl, out_c, out_st, out_s, hyp = [], [], [], [], []
    state = np.full(V, -1, np.int64)
    if V:
        keys = ext["key"].astype(np.int64); count = ext["count"].astype(np.int64); votes = ext["votes"].astype(np.int64)
        el = count >= p["min_count"]
        if p["skip_labelled"]:
            el &= votes == 0
        state[el] = -2
        res["n_eligible"] = int(el.sum())
        X = (keys.astype(np.float64) + 0.5) * leaf
        if el.any():
            kmin = [int(x) for x in keys[el].min(axis=0)]
            span = int((keys[el].max(axis=0) - keys[el].min(axis=0) + 1).max())
        stop = 0
        for r in range(P):
            U = np.flatnonzero(state == -2)
            n_r = len(U)
            if n_r < 3:
                stop = 1
                break
            res["rounds"] = r + 1
            XU, cU, kU = X[U], count[U], keys[U]
            rows = np.zeros((Hn, 3), np.int64)
            hyp.append(rows)
            pls = {}
            for h in range(Hn):
                i = [index(p["seed"], r, Hn, h, k, n_r) for k in range(3)]
                a, b, c = ([int(x) for x in kU[j]] for j in i)
                pl = hypothesis(i, a, b, c, p["min_baseline"], leaf)
                if pl is None:
                    continue
                _, n_in, smp = score(pl, XU, cU, p["dist_tol"])
                rows[h] = (1, n_in, smp)
                pls[h] = pl
            win_h = winner(rows.tolist())
            if win_h is None:
                stop = 2
                break
            win_n, win_s, fin = int(rows[win_h, 1]), int(rows[win_h, 2]), pls[win_h]
            fin_n, refined = win_n, 0
            if p["refine"]:
                if guard(win_n, span):
                    refined = 3
                else:
                    inl, _, _ = score(fin, XU, cU, p["dist_tol"])
                    re = refit(moments(kU[inl], cU[inl], kmin), kmin, leaf)
                    _, n2, s2 = score(re, XU, cU, p["dist_tol"])
                    if refit_kept(n2, s2, win_n, win_s):
                        refined, fin, fin_n = 1, re, n2
                    else:
                        refined = 2
            if fin_n < p["min_inliers"]:
                stop = 3
                break
            inl, n_in, smp = score(fin, XU, cU, p["dist_tol"])
            state[U[inl]] = r
            out_pl.append(orient_out(fin))
            out_c.append(centroid(moments(kU[inl], cU[inl], kmin), kmin, leaf))
            out_st.append([n_in, n_r, int(rows[:, 0].sum()), win_h, win_n, refined, 0, 0])
            out_s.append(smp)
            res["n_planes"] += 1; res["n_assigned"] += n_in
        res["stop_reason"] = stop
    g = np.zeros(4)
    uh = up_unit(p["up"])
    if uh is not None:
        res["ground_index"], gp = ground(out_pl, [s[0] for s in out_st], uh, p["up_min_cos"])
        g = np.array(gp, dtype=np.float64)
    return dict(result=res, planes=np.array(out_pl, dtype=np.float64).reshape(-1, 4), centroid=np.array(out_c, dtype=np.float64).reshape(-1, 3),
                stats=np.array(out_st, dtype=np.int32).reshape(-1, 8), samples=np.array(out_s, dtype=np.int64), ground=g,
                voxel_plane=state[:min(voxel_cap, V)].astype(np.int32), hyp=np.array(hyp, dtype=np.int64).reshape(-1, Hn, 3))
