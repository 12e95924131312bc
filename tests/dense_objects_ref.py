"""The numpy statement of esl_dense_objects (include/esl.h, "per-instance ellipsoids from the dense map", steps 1-9) on top of
dense_ref.DenseMap.extract().  The arithmetic follows the header operation by operation, in Python floats (IEEE doubles, no contraction);
components come from a plain union-find over the pairs that a sorted search of every neighbour key finds.
Test infrastructure only: nothing here is imported by the package."""
import math

import numpy as np

import dense_ref as dr

DEFAULTS = dict(reach=2, min_votes=1, min_count=1, min_component=100, max_components=65536, plane_dist=0.05)
RESULT = ("status", "n_voxels", "n_in_range", "n_gated", "n_kept", "n_components_all", "n_components", "n_ok")
GUARD = 1 << 62


def plane(g):
    """steps 1 and 6 -> (n^ (3 floats), d^, u, v)"""
    g = [float(x) for x in g]
    nn = math.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
    if not all(math.isfinite(x) for x in g) or not math.isfinite(nn) or not nn >= 1e-12:
        raise ValueError("ground_world not finite or its normal shorter than 1e-12")
    n = [g[0] / nn, g[1] / nn, g[2] / nn]
    d = g[3] / nn
    k = 0
    for a in (1, 2):
        if abs(n[a]) < abs(n[k]):
            k = a
    e = [0.0, 0.0, 0.0]; e[k] = 1.0
    u = [e[1] * n[2] - e[2] * n[1], e[2] * n[0] - e[0] * n[2], e[0] * n[1] - e[1] * n[0]]
    un = math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    u = [x / un for x in u]
    v = [n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]]
    return n, d, u, v


def centers(keys, leaf):
    return (np.asarray(keys).astype(np.float64) + 0.5) * leaf


def proj(a, p):
    """(a0 p0 + a1 p1) + a2 p2 of every row of p"""
    return (a[0] * p[:, 0] + a[1] * p[:, 1]) + a[2] * p[:, 2]


def guard(n, span):
    return n * span * span >= GUARD          # Python integers do not overflow


def half_offsets(reach):
    """the offsets of the (2 reach + 1)^3 cube that are lexicographically above (0, 0, 0): 13, 62 or 171"""
    r = range(-reach, reach + 1)
    return [(x, y, z) for x in r for y in r for z in r if (x, y, z) > (0, 0, 0)]


def components(keys, lab, reach):
    """keys (n, 3) in ascending packed order, lab (n,) -> root index of every voxel; the root is the component's smallest index"""
    n = len(keys)
    packed = dr.pack(keys)
    assert (np.diff(packed.astype(np.int64)) > 0).all()
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    idx = np.arange(n)
    for off in half_offsets(reach):
        nb = keys + np.array(off, np.int64)
        ok = (np.abs(nb) <= dr.KEY_MAX).all(axis=1)
        q = dr.pack(nb[ok])
        pos = np.searchsorted(packed, q)
        hit = pos < n
        hit[hit] = packed[pos[hit]] == q[hit]
        i, j = idx[ok][hit], pos[hit]
        same = lab[i] == lab[j]
        for a, b in zip(i[same].tolist(), j[same].tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], dtype=np.int64)


def quat(R):
    """the library's q_from_R of the row-major 3 x 3 R (a list of 9), negated when w < 0"""
    t = R[0] + R[4] + R[8]
    if t > 0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t; t = 0.5 / t
        x = (R[7] - R[5]) * t; y = (R[2] - R[6]) * t; z = (R[3] - R[1]) * t
    elif R[0] >= R[4] and R[0] >= R[8]:
        t = math.sqrt(R[0] - R[4] - R[8] + 1.0)
        x = 0.5 * t; t = 0.5 / t
        w = (R[7] - R[5]) * t; y = (R[3] + R[1]) * t; z = (R[6] + R[2]) * t
    elif R[4] >= R[8]:
        t = math.sqrt(R[4] - R[8] - R[0] + 1.0)
        y = 0.5 * t; t = 0.5 / t
        w = (R[2] - R[6]) * t; z = (R[7] + R[5]) * t; x = (R[1] + R[3]) * t
    else:
        t = math.sqrt(R[8] - R[0] - R[4] + 1.0)
        z = 0.5 * t; t = 0.5 / t
        w = (R[3] - R[1]) * t; x = (R[2] + R[6]) * t; y = (R[5] + R[7]) * t
    if w < 0:
        x, y, z, w = -x, -y, -z, -w
    return [x, y, z, w]


def quad(a, C, b):
    r0 = (C[0] * b[0] + C[1] * b[1]) + C[2] * b[2]
    r1 = (C[1] * b[0] + C[3] * b[1]) + C[4] * b[2]
    r2 = (C[2] * b[0] + C[4] * b[1]) + C[5] * b[2]
    return (a[0] * r0 + a[1] * r1) + a[2] * r2


def frame(pl, n, mom):
    """step 6 -> (x, y, n^, (C_uu, C_uv, C_vv)); mom = the nine integers s (3), M (xx xy xz yy yz zz)"""
    nh, _, u, v = pl
    dn = float(n)
    m = [float(mom[0]) / dn, float(mom[1]) / dn, float(mom[2]) / dn]
    C = [float(mom[3]) / dn - m[0] * m[0], float(mom[4]) / dn - m[0] * m[1], float(mom[5]) / dn - m[0] * m[2],
         float(mom[6]) / dn - m[1] * m[1], float(mom[7]) / dn - m[1] * m[2], float(mom[8]) / dn - m[2] * m[2]]
    cuu, cuv, cvv = quad(u, C, u), quad(u, C, v), quad(v, C, v)
    th = 0.5 * math.atan2(2 * cuv, cuu - cvv)
    c, s = math.cos(th), math.sin(th)
    x = [c * u[a] + s * v[a] for a in range(3)]
    y = [nh[1] * x[2] - nh[2] * x[1], nh[2] * x[0] - nh[0] * x[2], nh[0] * x[1] - nh[1] * x[0]]
    return x, y, list(nh), (cuu, cuv, cvv)


def moments(k):
    """step 5 of the members' keys (m, 3) int64 -> (kmin, kmax, the nine integers), Python integers"""
    kmin, kmax = k.min(axis=0), k.max(axis=0)
    d = (k - kmin).astype(object)          # exact integers of any size
    mom = [int(d[:, a].sum()) for a in range(3)]
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        mom.append(int((d[:, a] * d[:, b]).sum()))
    return kmin, kmax, mom


def objects(ext, leaf, N, ground, comp_cap=None, voxel_cap=None, **over):
    """ext = DenseMap.extract() (all voxels).  Returns what Context.dense_objects returns, and `margins`: the smallest |h - plane_dist|
    of a gated voxel, and per object of status 0 its anisotropy sqrt((C_uu - C_vv)^2 + 4 C_uv^2) / (C_uu + C_vv)."""
    p = dict(DEFAULTS); p.update(over)
    res = dict.fromkeys(RESULT, 0)
    if ext["n_voxels"] < 0:
        res.update(status=3, n_voxels=-1)
        return dict(result=res, objs=np.zeros((0, 10)), stats=np.zeros((0, 6), np.int32), comp=np.zeros((0, 6), np.int32),
                    voxel_comp=np.zeros(0, np.int32), margins=dict(height=np.inf, anisotropy={}))
    pl = plane(ground)
    nh, dh = pl[0], pl[1]
    V = ext["n_voxels"]
    keys = ext["key"].astype(np.int64); count = ext["count"].astype(np.int64); lab = ext["inst"].astype(np.int64); votes = ext["votes"].astype(np.int64)
    assert len(keys) == V
    inr = (lab >= 0) & (lab < N)
    gated = inr & (votes >= p["min_votes"]) & (count >= p["min_count"])
    h = proj(nh, centers(keys, leaf)) + dh
    kept = gated & (h >= p["plane_dist"])
    res.update(n_voxels=V, n_in_range=int(inr.sum()), n_gated=int(gated.sum()), n_kept=int(kept.sum()))
    margins = dict(height=float(np.abs(h[gated] - p["plane_dist"]).min()) if gated.any() else np.inf, anisotropy={})
    ki = np.flatnonzero(kept)          # ascending packed key
    root = components(keys[ki], lab[ki], p["reach"]) if len(ki) else np.zeros(0, np.int64)
    roots, inv, size = np.unique(root, return_inverse=True, return_counts=True)
    samples = np.zeros(len(roots), np.int64); np.add.at(samples, inv, count[ki])
    res["n_components_all"] = len(roots)
    big = np.flatnonzero(size >= p["min_component"])
    rlab = lab[ki][roots]
    order = big[np.lexsort((roots[big], -size[big], rlab[big]))]          # label, then size descending, then key
    R = len(order)
    res["n_components"] = R
    comp_cap = R if comp_cap is None else comp_cap
    voxel_cap = V if voxel_cap is None else voxel_cap
    objs = np.zeros((N, 10)); stats = np.zeros((N, 6), np.int32)
    comp = np.zeros((min(comp_cap, R), 6), np.int32); vox = np.full(min(voxel_cap, V), -1, np.int32)
    if R > p["max_components"]:
        res["status"] = 3
        return dict(result=res, objs=objs, stats=stats, comp=comp, voxel_comp=vox, margins=margins)
    table = np.concatenate([np.stack([rlab[order], size[order], samples[order]], axis=-1), keys[ki][roots[order]]], axis=-1).reshape(R, 6)
    comp[:] = table[:len(comp)]
    rowof = np.full(len(roots), -2, np.int64); rowof[order] = np.arange(R)
    full = np.full(V, -1, np.int64); full[ki] = rowof[inv]
    vox[:] = full[:len(vox)]
    for o in range(N):
        n_kept_o = int((lab[ki] == o).sum())
        rows = np.flatnonzero(table[:, 0] == o)
        st = stats[o]
        st[1], st[2], st[3] = n_kept_o, len(rows), -1
        if n_kept_o == 0:
            st[0] = 1; continue
        if len(rows) == 0:
            st[0] = 2; continue
        row = int(rows[0])
        st[3], st[4], st[5] = row, table[row, 1], table[row, 2]
        mk = keys[ki][rowof[inv] == row]
        kmin, kmax, mom = moments(mk)
        n = len(mk)
        if guard(n, int((kmax - kmin + 1).max())):
            st[0] = 6; continue
        x, y, z, (cuu, cuv, cvv) = frame(pl, n, mom)
        margins["anisotropy"][o] = math.hypot(cuu - cvv, 2 * cuv) / (cuu + cvv) if cuu + cvv > 0 else 0.0
        pc = centers(mk, leaf)
        c, half = [], []
        for ax in (x, y, z):
            pr = proj(ax, pc)
            mn, mx = float(pr.min()), float(pr.max())
            c.append((mn + mx) / 2); half.append((mx - mn) / 2 + leaf / 2)
        t = [(x[a] * c[0] + y[a] * c[1]) + z[a] * c[2] for a in range(3)]
        q = quat([x[0], y[0], z[0], x[1], y[1], z[1], x[2], y[2], z[2]])
        objs[o] = t + q + half
        res["n_ok"] += 1
    return dict(result=res, objs=objs, stats=stats, comp=comp, voxel_comp=vox, margins=margins)


# ---- placing voxels exactly through esl_dense_add_frames ------------------------------------------------------------------------------------
def voxel_frames(keys, leaf, labels, repeat=None):
    """One 1 x 1 frame per sample: K = (1, 1, 0, 0), raw depth 5000 (z = 1 m), identity rotation, t = (-X, -Y, 1 - Z) puts the sample at
    (X, Y, Z) = the centre of voxel `keys[i]`.  repeat[i] samples for voxel i (default 1), all with label labels[i] unless labels[i] is
    a sequence (one label per sample).  Returns the arguments of dense_add_frames as a dict."""
    cams, inst = [], []
    for i, k in enumerate(np.asarray(keys, dtype=np.int64)):
        ls = labels[i]
        ls = list(ls) if np.ndim(ls) else [int(ls)] * (1 if repeat is None else int(repeat[i]))
        X, Y, Z = ((float(k[a]) + 0.5) * leaf for a in range(3))
        for lb in ls:
            cams.append([-X, -Y, 1.0 - Z, 0.0, 0.0, 0.0, 1.0]); inst.append(lb)
    F = len(cams)
    return dict(cams=np.array(cams, dtype=np.float64).reshape(F, 7), K=(1.0, 1.0, 0.0, 0.0), rows=1, cols=1,
                depth=np.full((F, 1, 1), 5000, np.uint16), bgr=np.zeros((F, 1, 1, 3), np.uint8), inst=np.array(inst, np.int32).reshape(F, 1, 1))
