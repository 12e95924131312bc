"""The numpy statement of esl_render_map (include/esl.h, "rendering the map", steps 1-6): brute force, every pixel against every
object, no culling.  `render` is the statement; `sphere_hits` is a second, independent formulation of step 3 (the ray moved into the
object's frame and scaled by 1 / s, intersected with the unit sphere) from which the depth tolerance of the device comparison is
measured (tests/test_render_ref.py, render_scenes.TOL).  Test infrastructure only: nothing here is imported by the package."""
import numpy as np

DEFAULTS = dict(depth_scale=5000.0, depth_min=0.1, depth_max=6.0, depth_tol=0.05)
DRAWN, INVALID, INSIDE, BOUNDED = 1, 2, 4, 8


def q_to_R(q):
    """rotation matrix of the quaternion (x, y, z, w) by the library's formula (no normalisation of its own)"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def valid_object(v):
    """step 1 -> (ok, normalised quaternion, |half-axes|)"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        nrm = np.sqrt((v[3:7] ** 2).sum())
        s = np.abs(v[7:10])
        ok = bool(np.isfinite(v).all() and np.isfinite(nrm) and nrm > 0 and (s > 0).all())
    return ok, (v[3:7] / nrm if ok else None), s


def camera_frame(cam, v):
    """Rco, tco of a valid object: Rco = Rcw Rwo, tco = Rcw two + tcw"""
    _, q, _ = valid_object(v)
    Rc = q_to_R(np.asarray(cam[3:7], dtype=np.float64))
    return Rc @ q_to_R(q), Rc @ np.asarray(v[:3], dtype=np.float64) + np.asarray(cam[:3], dtype=np.float64)


def body(Rco, tco, s):
    """step 2 -> A, g, c0"""
    A = Rco @ np.diag(1.0 / (s * s)) @ Rco.T
    g = A @ tco
    return A, g, float(tco @ g - 1.0)


def conic_box(Rco, tco, s, K):
    """(C22, box or None) of the projected outline: the dual conic C* = sum_k s_k^2 m_k m_k^T - m_3 m_3^T of M = K [Rco | tco] and its
    tangent lines, as the bbox edge evaluates them"""
    fx, fy, cx, cy = K
    Kmat = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    Mm = Kmat @ np.column_stack([Rco, tco])
    C = (Mm[:, :3] * (s * s)) @ Mm[:, :3].T - np.outer(Mm[:, 3], Mm[:, 3])
    C22 = C[2, 2]
    du, dv = C[0, 2] ** 2 - C[0, 0] * C22, C[1, 2] ** 2 - C[1, 1] * C22
    if not (C22 < 0) or not (du >= 0) or not (dv >= 0):
        return C22, None
    su, sv = np.sqrt(du), np.sqrt(dv)
    return C22, np.array([(C[0, 2] + su) / C22, (C[1, 2] + sv) / C22, (C[0, 2] - su) / C22, (C[1, 2] - sv) / C22])


def pixel_rays(K, rows, cols):
    """step 3: dx, dy of every pixel, (rows, cols) each"""
    fx, fy, cx, cy = K
    dx = (np.arange(cols, dtype=np.float64) - cx) / fx
    dy = (np.arange(rows, dtype=np.float64) - cy) / fy
    return np.broadcast_to(dx[None, :], (rows, cols)), np.broadcast_to(dy[:, None], (rows, cols))


def quadric_hits(A, g, c0, dx, dy):
    """step 3 -> (hit mask, z (NaN where no hit), the margin |Delta| / (beta^2 + alpha |c0|))"""
    alpha = A[0, 0] * dx * dx + 2 * A[0, 1] * dx * dy + 2 * A[0, 2] * dx + A[1, 1] * dy * dy + 2 * A[1, 2] * dy + A[2, 2]
    beta = g[0] * dx + g[1] * dy + g[2]
    delta = beta * beta - alpha * c0
    hit = (beta > 0) & (delta > 0)
    z = np.full(dx.shape, np.nan)
    z[hit] = c0 / (beta[hit] + np.sqrt(delta[hit]))
    with np.errstate(all="ignore"):
        margin = np.abs(delta) / (beta * beta + alpha * abs(c0))
    # beta decides only where Delta > 0; there beta^2 > alpha c0 > 0, so |beta| is away from 0 whenever Delta's margin holds
    return hit, z, margin


def sphere_hits(Rco, tco, s, dx, dy):
    """the second formulation: origin and direction of the ray in the object's frame, scaled by 1 / s; unit sphere; z = (-b - sqrt D) / a"""
    o = (Rco.T @ (-tco)) / s
    d = np.stack([dx, dy, np.ones_like(dx)], axis=-1) @ Rco          # = Rco^T d per pixel
    d = d / s
    a = (d * d).sum(-1)
    b = d @ o
    c = float(o @ o - 1.0)
    D = b * b - a * c
    hit = (c > 0) & (b < 0) & (D > 0)
    z = np.full(dx.shape, np.nan)
    z[hit] = (-b[hit] - np.sqrt(D[hit])) / a[hit]
    return hit, z


def compare(raw, z, p):
    """step 6 on arrays -> category 0 agree, 1 nearer, 2 farther, 3 no data; and the margin ||z_meas - z| - depth_tol| where it decides"""
    zm = raw.astype(np.float64) / p["depth_scale"]
    nodata = (raw == 0) | ~(zm >= p["depth_min"]) | ~(zm <= p["depth_max"])
    cat = np.where(nodata, 3, np.where(np.abs(zm - z) <= p["depth_tol"], 0, np.where(zm < z - p["depth_tol"], 1, 2)))
    margin = np.where(nodata, np.inf, np.abs(np.abs(zm - z) - p["depth_tol"]))
    return cat, margin


def render(cams, objs, K, rows, cols, depth_meas=None, margins=True, **over):
    """steps 1-6 -> dict(depth (F, rows, cols), inst, cover (F, M, 2), cmp (F, M, 4) or None, flags (F, M), margins: dict of the
    smallest decision margins met (render_scenes.check_conditions; the gap between a pixel's two nearest bodies only with `margins`,
    which holds M images), params)"""
    p = dict(DEFAULTS); p.update(over)
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    F, M = len(cams), len(objs)
    dx, dy = pixel_rays(K, rows, cols)
    depth = np.full((F, rows, cols), np.nan); inst = np.full((F, rows, cols), -1, dtype=np.int32)
    cover = np.zeros((F, M, 2), dtype=np.int32); flags = np.zeros((F, M), dtype=np.int32)
    cmp_ = None if depth_meas is None else np.zeros((F, M, 4), dtype=np.int32)
    rows_b = [o.tobytes() for o in objs]
    twin = np.array([rows_b.index(b) for b in rows_b], dtype=np.int64)          # the first row with the same bits
    mg = dict(delta=np.inf, c0=np.inf, gap=np.inf, tol=np.inf, c22=np.inf)
    for f in range(F):
        best = np.full((rows, cols), np.inf); who = np.full((rows, cols), -1, dtype=np.int32)
        zs = np.full((M, rows, cols), np.inf) if margins else None
        for m in range(M):
            ok, _, s = valid_object(objs[m])
            if not ok:
                flags[f, m] = INVALID
                continue
            Rco, tco = camera_frame(cams[f], objs[m])
            A, g, c0 = body(Rco, tco, s)
            mg["c0"] = min(mg["c0"], abs(c0))
            if not c0 > 0:
                flags[f, m] = INSIDE
                continue
            C22, box = conic_box(Rco, tco, s, K)
            mg["c22"] = min(mg["c22"], abs(C22) / (tco[2] ** 2 + (s * s).max()))
            if C22 < 0 and tco[2] < 0:
                flags[f, m] = 0          # wholly behind; the ray cast below finds no hit either (beta < 0 everywhere)
            elif C22 < 0 and tco[2] > 0 and box is not None and np.isfinite(box).all():
                flags[f, m] = DRAWN | BOUNDED
            else:
                flags[f, m] = DRAWN
            hit, z, margin = quadric_hits(A, g, c0, dx, dy)
            mg["delta"] = min(mg["delta"], float(margin.min()))
            cover[f, m, 0] = hit.sum()
            zz = np.where(hit, z, np.inf)
            if margins:
                zs[m] = zz
            nearer = zz < best          # strict: a tie keeps the lower m
            who = np.where(nearer, m, who); best = np.where(nearer, zz, best)
        won = who >= 0
        depth[f][won] = best[won]; inst[f] = who
        if margins and won.any():          # the nearest hit of another body; bit-identical copies of the winner's row are the same body
            other = zs.copy()
            other[twin[:, None, None] == twin[np.maximum(who, 0)][None, :, :]] = np.inf
            second = other.min(0)[won]
            gap = np.where(np.isfinite(second), second, np.inf) - np.where(np.isfinite(second), best[won], 0.0)
            mg["gap"] = min(mg["gap"], float(gap.min()))
        cover[f, :, 1] = np.bincount(who[won], minlength=M)
        if depth_meas is not None:
            cat, tm = compare(np.asarray(depth_meas)[f], np.where(won, best, 0.0), p)
            for k in range(4):
                cmp_[f, :, k] = np.bincount(who[won & (cat == k)], minlength=M)
            if won.any():
                mg["tol"] = min(mg["tol"], float(tm[won].min()))
    return dict(depth=depth, inst=inst, cover=cover, cmp=cmp_, flags=flags, margins=mg, params=p)
