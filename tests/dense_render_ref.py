"""The numpy statement of esl_dense_render (include/esl.h, "viewing the dense map", steps 1-8) on top of dense_ref.DenseMap.extract().
The arithmetic follows the header operation by operation in IEEE doubles (np.rint for llrint); the winner of a pixel is a plain minimum
over packed Python integers.  The device is compared with it exactly, so nothing here may be "simplified".
Test infrastructure only: nothing here is imported by the package."""
import numpy as np

import dense_ref as dr
import render_ref as rr

DEFAULTS = dict(depth_scale=5000.0, depth_min=0.1, depth_max=6.0, depth_tol=0.05, footprint=1.0, max_radius=8, min_count=1,
                zbuf_bytes=268435456)
COORD_MAX = float(1 << 30)
ZFIX = float(1 << 20)
EMPTY = (1 << 64) - 1
FRAME_COLS = ("n_drawn", "n_depth_out", "n_outside", "covered", "agree", "nearer", "farther", "nodata")


def axis(f, c, x, z, e, max_radius, n):
    """step 3 along one axis on arrays -> ok, lo, hi (doubles holding integers where ok) and the three coordinates"""
    with np.errstate(all="ignore"):
        u = (f * x) / z + c
        u0 = (f * (x - e)) / z + c
        u1 = (f * (x + e)) / z + c
        ok = (np.abs(u) <= COORD_MAX) & (np.abs(u0) <= COORD_MAX) & (np.abs(u1) <= COORD_MAX)          # NaN and infinities compare false
        col = np.floor(u + 0.5)
        c0 = np.minimum(col, np.ceil(u0)); c1 = np.maximum(col, np.floor(u1))
        c0 = np.maximum(c0, col - float(max_radius)); c1 = np.minimum(c1, col + float(max_radius))
        c0 = np.maximum(c0, 0.0); c1 = np.minimum(c1, float(n - 1))
        ok = ok & (c0 <= c1)
    return ok, c0, c1, (u, u0, u1)


def project(xyz, cam, K, rows, cols, e, p):
    """steps 2 and 3 of every voxel in one frame -> dict(z, depth_in, drawn, box (n, 4) int64 = c0 c1 r0 r1 where drawn, coords)"""
    fx, fy, cx, cy = (float(v) for v in K)
    R, t = dr.pose(cam)
    p0, p1, p2 = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        pc = [((R[a, 0] * p0 + R[a, 1] * p1) + R[a, 2] * p2) + t[a] for a in range(3)]
        z = pc[2]
        depth_in = (z >= p["depth_min"]) & (z <= p["depth_max"])          # a NaN fails
    okx, c0, c1, cu = axis(fx, cx, pc[0], z, e, p["max_radius"], cols)
    oky, r0, r1, cv = axis(fy, cy, pc[1], z, e, p["max_radius"], rows)
    drawn = depth_in & okx & oky
    box = np.stack([np.where(drawn, v, 0.0) for v in (c0, c1, r0, r1)], axis=-1).astype(np.int64)
    return dict(z=z, depth_in=depth_in, drawn=drawn, box=box, coords=cu + cv)


def boundary(v, half=False):
    """the distance of every v to the nearest integer (half: to the nearest half-integer): how close a floor, ceil or rint is to flipping"""
    with np.errstate(all="ignore"):
        return np.abs(v - np.floor(v) - 0.5) if half else np.abs(v - np.rint(v))


def render(ext, leaf, cams, K, rows, cols, depth_meas=None, vox_cap=None, **over):
    """steps 1-8.  ext = DenseMap.extract() of this moment.  Returns dict(result, depth, voxel, bgr, inst, frame, vox) and, for the
    tests' premises, margins (the smallest boundary distances over the drawn voxels) and area (n_frames lists of the drawn footprints'
    pixel counts)."""
    p = dict(DEFAULTS); p.update(over)
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    F, npix = len(cams), rows * cols
    if ext["n_voxels"] < 0:          # step 8
        return dict(result=dict(status=int(ext.get("status", 3)), n_voxels=-1, n_small=0, n_chunks=0))
    for c in cams:
        dr.pose(c)          # an invalid pose anywhere: nothing runs
    n = int(ext["n_voxels"])
    xyz = np.asarray(ext["xyz"], dtype=np.float64).reshape(n, 3)
    count = np.asarray(ext["count"]).reshape(n)
    small = count < p["min_count"]
    chunk = max(1, int(p["zbuf_bytes"]) // (8 * npix))          # step 7
    e = p["footprint"] * leaf / 2
    n_vw = n if vox_cap is None else min(int(vox_cap), n)
    depth = np.full((F, rows, cols), np.nan); voxel = np.full((F, rows, cols), -1, np.int32)
    bgr = np.zeros((F, rows, cols, 3), np.uint8); inst = np.full((F, rows, cols), -1, np.int32)
    frame = np.zeros((F, 8), np.int32); vox = np.zeros((n, 4), np.int32)
    margins = dict(round=np.inf, ceil=np.inf, floor=np.inf, zq=np.inf, tol=np.inf)
    areas = []
    for f in range(F):
        pr = project(xyz, cams[f], K, rows, cols, e, p)
        live = ~small
        drawn = live & pr["drawn"]
        frame[f, 0] = int(drawn.sum())
        frame[f, 1] = int((live & ~pr["depth_in"]).sum())
        frame[f, 2] = int((live & pr["depth_in"] & ~pr["drawn"]).sum())
        z = pr["z"]
        with np.errstate(all="ignore"):
            zq = np.rint(z * ZFIX)          # step 4
        idx = np.flatnonzero(drawn)
        if len(idx):
            u, u0, u1, v, v0, v1 = (a[idx] for a in pr["coords"])
            margins["round"] = min(margins["round"], float(boundary(np.concatenate([u, v]) + 0.5).min()))
            margins["ceil"] = min(margins["ceil"], float(boundary(np.concatenate([u0, v0])).min()))
            margins["floor"] = min(margins["floor"], float(boundary(np.concatenate([u1, v1])).min()))
            margins["zq"] = min(margins["zq"], float(boundary(z[idx] * ZFIX, half=True).min()))
        zb = [EMPTY] * npix
        area = []
        for i in idx.tolist():
            c0, c1, r0, r1 = (int(b) for b in pr["box"][i])
            word = (int(zq[i]) << 32) | i
            area.append((c1 - c0 + 1) * (r1 - r0 + 1))
            for r in range(r0, r1 + 1):
                for c in range(c0, c1 + 1):
                    if word < zb[r * cols + c]:
                        zb[r * cols + c] = word
        areas.append(area)
        win = np.array([w & 0xFFFFFFFF if w != EMPTY else -1 for w in zb], dtype=np.int64).reshape(rows, cols)
        has = win >= 0
        wi = win[has]
        depth[f][has] = z[wi]          # step 5: the winner's own z
        voxel[f][has] = wi
        bgr[f][has] = np.asarray(ext["bgr"]).reshape(n, 3)[wi]
        inst[f][has] = np.asarray(ext["inst"]).reshape(n)[wi]
        frame[f, 3] = int(has.sum())
        np.add.at(vox[:, 0], wi, 1)
        if depth_meas is not None:          # step 6
            cat, mg = rr.compare(np.asarray(depth_meas)[f][has], z[wi], p)
            margins["tol"] = min(margins["tol"], float(mg.min()) if mg.size else np.inf)
            for k_ in range(4):
                frame[f, 4 + k_] = int((cat == k_).sum())
            for k_ in range(3):
                np.add.at(vox[:, 1 + k_], wi[cat == k_], 1)
    result = dict(status=0, n_voxels=n, n_small=int(small.sum()), n_chunks=(F + chunk - 1) // chunk)
    return dict(result=result, depth=depth, voxel=voxel, bgr=bgr, inst=inst, frame=frame, vox=vox[:n_vw], margins=margins, area=areas)
