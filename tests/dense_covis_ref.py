"""The numpy statement of esl_dense_covis_frames (include/esl.h, "covisibility of the dense map", steps V1-V7) on top of
dense_update_ref.DenseUpdateMap: the voxels are its extract(), "sees" is dense_carve_ref.observe's class agree (step V2), B is the
boolean F x n matrix of it, the pair counts are B B^T and the cull loop of step V6 runs in plain Python integers.  The device is
compared with it exactly.  Test infrastructure only: nothing here is imported by the package."""
import numpy as np

import dense_carve_ref as dcr
import dense_ref as dr

DEFAULTS = dict(depth_scale=5000.0, depth_min=0.1, depth_max=6.0, depth_tol=0.05, window=1, min_others=3, cover_num=9, cover_den=10, max_cull=0,
                reserved=0)
MAX_FRAMES = 4096


def redundant(seen, covered, num, den):
    """step V5 on Python integers"""
    return seen >= 1 and int(covered) * int(den) >= int(num) * int(seen)


def before(unc_a, fa, unc_b, fb):
    """step V6: candidate a leaves before candidate b"""
    return (unc_a, fa) < (unc_b, fb)


def pair_count(a, b):
    """step V4 on two rows of 64-bit words (Python integers)"""
    return sum(bin(int(x) & int(y)).count("1") for x, y in zip(a, b))


def cull(B, keep, p):
    """step V6 on the boolean matrix B -> (round per frame, [(frame, uncovered)] in the order of leaving)"""
    F = len(B)
    alive = [True] * F
    rounds = [-1] * F
    order = []
    seen = [int(B[f].sum()) for f in range(F)]
    for r in range(int(p["max_cull"])):
        k = B[[f for f in range(F) if alive[f]]].sum(axis=0).astype(np.int64) if any(alive) else np.zeros(B.shape[1], np.int64)
        best = None
        for f in range(F):
            if not alive[f] or (keep is not None and keep[f]):
                continue
            cov = int((B[f] & (k - 1 >= int(p["min_others"]))).sum())
            if not redundant(seen[f], cov, p["cover_num"], p["cover_den"]):
                continue
            if best is None or before(seen[f] - cov, f, best[1], best[0]):
                best = (f, seen[f] - cov)
        if best is None:
            break
        alive[best[0]] = False
        rounds[best[0]] = r
        order.append(best)
    return rounds, order


def covis(m, cams, depth, K, rows, cols, keep=None, vox_cap=None, **over):
    """steps V1-V7 on the DenseUpdateMap m.  Returns dict(result, vox, frame, pair) and, for the tests, B (F, n) bool and order."""
    p = dict(DEFAULTS); p.update(over)
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    F = len(cams)
    assert F <= MAX_FRAMES
    if m.status:          # step V7
        return dict(result=dict(status=m.status, n_voxels=-1, n_seen=0, n_culled=0, sum_seen=0, sum_pairs=0))
    for c in cams:
        dr.pose(c)          # an invalid pose anywhere: nothing runs
    ext = m.extract()          # step V1
    n = int(ext["n_voxels"])
    xyz = np.asarray(ext["xyz"], dtype=np.float64).reshape(n, 3)
    B = np.zeros((F, n), bool)
    frame = np.zeros((F, 8), np.int32)
    for f in range(F):
        cls = dcr.observe(xyz, cams[f], K, rows, cols, np.asarray(depth)[f], p)          # step V2
        B[f] = cls == dcr.AGREE
        frame[f, 0] = int((cls <= dcr.NODATA).sum()); frame[f, 1] = int((cls == dcr.DEPTH_OUT).sum()); frame[f, 2] = int((cls == dcr.OUTSIDE).sum())
    k = B.sum(axis=0).astype(np.int64)
    Bi = B.astype(np.int64)
    pair = (Bi @ Bi.T).astype(np.int32)          # step V4
    frame[:, 3] = B.sum(axis=1)
    frame[:, 4] = (B & (k - 1 >= int(p["min_others"]))).sum(axis=1)          # step V5, round 0
    frame[:, 5] = (B & (k == 1)).sum(axis=1)
    rounds, order = cull(B, keep, p)
    frame[:, 6] = rounds
    n_vw = n if vox_cap is None else min(int(vox_cap), n)
    result = dict(status=0, n_voxels=n, n_seen=int((k >= 1).sum()), n_culled=len(order), sum_seen=int(frame[:, 3].sum()),
                  sum_pairs=int(np.triu(pair.astype(np.int64), 1).sum()))
    return dict(result=result, vox=k.astype(np.int32)[:n_vw], frame=frame, pair=pair, B=B, order=order)
