"""The numpy statement of esl_dense_carve_frames (include/esl.h, "carving the dense map", steps C1-C7) on top of
dense_update_ref.DenseUpdateMap: the voxels are its extract(), the owners' samples are dense_ref.samples(), and apply is its
remove_frames on the carved-depth images.  The arithmetic follows the header operation by operation in IEEE doubles; the device is
compared with it exactly, so nothing here may be "simplified".  Test infrastructure only: nothing here is imported by the package."""
import numpy as np

import dense_ref as dr
import render_ref as rr

DEFAULTS = dict(depth_scale=5000.0, depth_min=0.1, depth_max=6.0, depth_tol=0.05, window=1, min_through=2, through_per_agree=1, apply=0)
COORD_MAX = float(1 << 30)
AGREE, NEARER, THROUGH, NODATA, DEPTH_OUT, OUTSIDE = range(6)
MAX_OBS = 65535
ZERO_REMOVED = dict(n_sampled=0, n_zero=0, n_depth_out=0, n_key_out=0, n_used=0, n_missing=0, n_emptied=0, status=0)


def observe(xyz, cam, K, rows, cols, depth, p):
    """step C2 of every voxel in one frame -> (n,) classes 0 agree, 1 nearer, 2 through, 3 no data, 4 depth out, 5 outside"""
    fx, fy, cx, cy = (float(v) for v in K)
    R, t = dr.pose(cam)
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    depth = np.asarray(depth)
    n, w = len(xyz), int(p["window"])
    p0, p1, p2 = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    cls = np.full(n, OUTSIDE, np.int64)
    with np.errstate(all="ignore"):
        pc = [((R[a, 0] * p0 + R[a, 1] * p1) + R[a, 2] * p2) + t[a] for a in range(3)]
        z = pc[2]
        depth_in = (z >= p["depth_min"]) & (z <= p["depth_max"])          # a NaN fails
        u = (fx * pc[0]) / z + cx
        v = (fy * pc[1]) / z + cy
        ok = (np.abs(u) <= COORD_MAX) & (np.abs(v) <= COORD_MAX)          # NaN and infinities compare false
        col = np.floor(u + 0.5); row = np.floor(v + 0.5)
        centre = (col >= 0.0) & (col <= float(cols - 1)) & (row >= 0.0) & (row <= float(rows - 1))
    cls[~depth_in] = DEPTH_OUT
    view = np.flatnonzero(depth_in & ok & centre)
    c, r, zv = col[view].astype(np.int64), row[view].astype(np.int64), z[view]
    seen = np.zeros((len(view), 4), bool)
    for dy in range(-w, w + 1):
        for dx in range(-w, w + 1):
            rr_, cc = r + dy, c + dx
            inside = (rr_ >= 0) & (rr_ <= rows - 1) & (cc >= 0) & (cc <= cols - 1)          # the window clipped to the image
            raw = depth[np.clip(rr_, 0, rows - 1), np.clip(cc, 0, cols - 1)]
            cat, _ = rr.compare(raw, zv, p)
            for k in range(4):
                seen[:, k] |= inside & (cat == k)
    cls[view] = np.where(seen[:, 0], AGREE, np.where(seen[:, 1], NEARER, np.where(seen[:, 2], THROUGH, NODATA)))
    return cls


def verdict(vox, p):
    """step C4 on the (n, 4) counts -> (n,) bool; Python integers would not overflow either, int64 is the header's word"""
    agree, through = vox[:, 0].astype(np.int64), vox[:, 2].astype(np.int64)
    return (through >= int(p["min_through"])) & (through >= int(p["through_per_agree"]) * agree)


def carve(m, cams_obs, depth_obs, cams_own, depth_own, K, rows, cols, bgr_own=None, inst_own=None, vox_cap=None, **over):
    """steps C1-C7 on the DenseUpdateMap m (changed when apply = 1).  Returns dict(result, vox, carved, obs, depth_kept, mask, own) and,
    for the tests, cls (F_obs, n) and carved_depth (the images the removal took)."""
    p = dict(DEFAULTS); p.update(over)
    cams_obs = np.asarray(cams_obs, dtype=np.float64).reshape(-1, 7)
    cams_own = np.zeros((0, 7)) if cams_own is None else np.asarray(cams_own, dtype=np.float64).reshape(-1, 7)
    Fo, Fw = len(cams_obs), len(cams_own)
    assert Fo <= MAX_OBS
    if m.status:          # step C7
        return dict(result=dict(status=m.status, n_voxels=-1, n_tested=0, n_carved=0, samples_found=0, samples_carved=0, removed=dict(ZERO_REMOVED)))
    for c in list(cams_obs) + list(cams_own):
        dr.pose(c)          # an invalid pose anywhere: nothing runs
    ext = m.extract()          # step C1
    n = int(ext["n_voxels"])
    xyz = np.asarray(ext["xyz"], dtype=np.float64).reshape(n, 3)
    cls = np.zeros((Fo, n), np.int64)
    obs = np.zeros((Fo, 8), np.int32); vox = np.zeros((n, 4), np.int32)
    for f in range(Fo):
        cls[f] = observe(xyz, cams_obs[f], K, rows, cols, np.asarray(depth_obs)[f], p)
        for k in range(4):
            obs[f, 3 + k] = int((cls[f] == k).sum())
            vox[:, k] += (cls[f] == k)
        obs[f, 0] = int((cls[f] <= NODATA).sum()); obs[f, 1] = int((cls[f] == DEPTH_OUT).sum()); obs[f, 2] = int((cls[f] == OUTSIDE).sum())
    carved = verdict(vox, p)
    tested = vox[:, :3].sum(axis=1) > 0
    # step C5
    live = {int(k): i for i, k in enumerate(dr.pack(ext["key"]).tolist())} if n else {}
    depth_own = np.zeros((0, rows, cols), np.uint16) if depth_own is None else np.asarray(depth_own, dtype=np.uint16)
    kept = depth_own.copy(); mask = np.zeros((Fw, rows, cols), np.uint8); own = np.zeros((Fw, 4), np.int32)
    for f in range(Fw):
        s = dr.samples(cams_own[f], K, rows, cols, depth_own[f], m.p)
        idx = np.array([live.get(int(k), -1) for k in dr.pack(s["k"]).tolist()], np.int64).reshape(-1)
        found = idx >= 0
        cv = np.zeros(len(idx), bool)
        cv[found] = carved[idx[found]]
        own[f] = [len(idx), int(found.sum()), int(cv.sum()), int((~found).sum())]
        mask[f][s["row"][cv], s["col"][cv]] = 1
    kept[mask == 1] = 0
    cdepth = np.where(mask == 1, depth_own, 0).astype(np.uint16)
    removed = dict(ZERO_REMOVED)
    status = 0
    if p["apply"] and Fw:          # step C6
        removed = m.remove_frames(cams_own, K, rows, cols, cdepth, bgr_own, inst_own)
        status = removed["status"]
    n_vw = n if vox_cap is None else min(int(vox_cap), n)
    result = dict(status=status, n_voxels=n, n_tested=int(tested.sum()), n_carved=int(carved.sum()), samples_found=int(own[:, 1].sum()),
                  samples_carved=int(own[:, 2].sum()), removed=removed)
    return dict(result=result, vox=vox[:n_vw], carved=carved.astype(np.uint8)[:n_vw], obs=obs, depth_kept=kept, mask=mask, own=own, cls=cls,
                carved_depth=cdepth)
