"""numpy statement of esl_predict_boxes / esl_associate_boxes (include/esl.h, "2-D data association").  Pure numpy; imports nothing of
the product.  It projects the reference's way -- the dual conic C* = P Q* P^T by matrix products, the box from the conic -- where the
product uses the closed form of csrc/esl_math.hpp.  Beside every result it returns `margin`: the smallest distance of a decision
quantity from its threshold (assoc2d_scenes.check_conditions)."""
import numpy as np

DEFAULTS = dict(min_iou=0.3, occl_ratio=0.7, min_box_px=10.0, match_labels=1, occlusion=1)


def params(**over):
    p = dict(DEFAULTS)
    for k, v in over.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose_matrix(v):
    T = np.eye(4)
    T[:3, :3] = quat_to_R(v[3:7]); T[:3, 3] = v[:3]
    return T


def dual_conic(Tcw, obj, K):
    """C* = P Q* P^T with Q* = T_wo diag(s^2, -1) T_wo^T and P = K [I | 0] T_cw"""
    Two = pose_matrix(obj[:7])
    Qs = Two @ np.diag([obj[7] ** 2, obj[8] ** 2, obj[9] ** 2, -1.0]) @ Two.T
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    P = Km @ pose_matrix(Tcw)[:3, :]
    return P @ Qs @ P.T


def raw_box(Tcw, obj, K, margins=None):
    """the unclipped box of the projected outline: the tangent lines x = const, y = const of the dual conic; NaN when the outline is
    not a real ellipse"""
    C = dual_conic(Tcw, obj, K)
    du = C[0, 2] ** 2 - C[0, 0] * C[2, 2]
    dv = C[1, 2] ** 2 - C[1, 1] * C[2, 2]
    if margins is not None:
        margins += [abs(C[2, 2]), abs(du), abs(dv)]
    if not (C[2, 2] < 0) or not (du >= 0) or not (dv >= 0):
        return np.full(4, np.nan)
    su, sv = np.sqrt(du), np.sqrt(dv)
    return np.array([(C[0, 2] + su) / C[2, 2], (C[1, 2] + sv) / C[2, 2], (C[0, 2] - su) / C[2, 2], (C[1, 2] - sv) / C[2, 2]])


def _inside(u, v, rows, cols, margins):
    margins += [abs(u), abs(u - cols), abs(v), abs(v - rows)]
    return 0 < u < cols and 0 < v < rows


def visible(Tcw, obj, K, rows, cols, margins):
    """the bbox edge's predicate (the reference's checkVisibility): centre in front of the camera, camera centre outside the
    ellipsoid, projected centre or the top-left / bottom-right corner of the projected box inside the image"""
    Tc = pose_matrix(Tcw)
    pc = Tc[:3, :3] @ obj[:3] + Tc[:3, 3]
    margins.append(abs(pc[2]))
    if pc[2] < 0:
        return False
    cam_w = -Tc[:3, :3].T @ Tc[:3, 3]
    xo = (quat_to_R(obj[3:7]).T @ (cam_w - obj[:3])) / obj[7:10]
    margins.append(abs(xo @ xo - 1.0))
    if xo @ xo - 1.0 < 0:
        return False
    if _inside(K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3], rows, cols, margins):
        return True
    bb = raw_box(Tcw, obj, K, margins)
    if np.isnan(bb[0]):
        return False
    return _inside(bb[0], bb[1], rows, cols, margins) or _inside(bb[2], bb[3], rows, cols, margins)


def area(b):
    return (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])


def overlap(a, b):
    """area of the intersection of boxes (broadcasting over leading axes)"""
    w = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
    h = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
    return np.where((w > 0) & (h > 0), w * h, 0.0)


def iou(a, b):
    i = overlap(a, b)
    return i / (area(a) + area(b) - i)


def predict(Tcw, objs, K, rows, cols, p=None):
    """steps 1 and 2 for one frame: dict(boxes (M, 4) clipped or NaN, raw (M, 4) unclipped, depth (M,), flags (M,), margin)"""
    p = params(**(p or {}))
    Tcw = np.asarray(Tcw, dtype=np.float64); objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    M = len(objs)
    boxes = np.full((M, 4), np.nan); raw = np.full((M, 4), np.nan); depth = np.full(M, np.nan); flags = np.zeros(M, np.int32)
    margins = [np.inf]
    Tc = pose_matrix(Tcw)
    for m in range(M):
        if not visible(Tcw, objs[m], K, rows, cols, margins):
            continue
        b = raw_box(Tcw, objs[m], K, margins)
        raw[m] = b
        if not np.all(np.isfinite(b)):
            continue
        c = np.array([max(b[0], 0.0), max(b[1], 0.0), min(b[2], float(cols)), min(b[3], float(rows))])
        margins += [abs(c[2] - c[0] - p["min_box_px"]), abs(c[3] - c[1] - p["min_box_px"])]
        if c[2] - c[0] >= p["min_box_px"] and c[3] - c[1] >= p["min_box_px"]:
            boxes[m] = c; flags[m] = 1
            depth[m] = (Tc[:3, :3] @ objs[m, :3] + Tc[:3, 3])[2]
    el = np.nonzero(flags & 1)[0]
    if p["occlusion"] and len(el) > 1:
        c, z = boxes[el], depth[el]
        nearer = (z[None, :] < z[:, None]) | ((z[None, :] == z[:, None]) & (el[None, :] < el[:, None]))   # [i, j]: j is nearer than i
        off = ~np.eye(len(el), dtype=bool)
        margins.append(np.abs(z[None, :] - z[:, None])[off].min())
        cover = overlap(c[:, None, :], c[None, :, :]) / area(c)[:, None]
        margins.append(np.abs(cover - p["occl_ratio"])[off].min())
        hidden = (nearer & off & (overlap(c[:, None, :], c[None, :, :]) >= p["occl_ratio"] * area(c)[:, None])).any(axis=1)
        flags[el[hidden]] |= 2
    return dict(boxes=boxes, raw=raw, depth=depth, flags=flags, margin=float(min(margins)))


def valid_box(b):
    return bool(np.all(np.isfinite(b)) and b[2] > b[0] and b[3] > b[1])


def associate(cams, objs, obj_labels, K, rows, cols, det_offsets, det_boxes, det_labels, p=None):
    """dict(assoc (n_det,), iou (n_det,), frame_stats (F, 4): eligible, occluded, assigned, spilled = 0; frames: predict() of every
    frame; margin)"""
    p = params(**(p or {}))
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7); objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    det_boxes = np.asarray(det_boxes, dtype=np.float64).reshape(-1, 4)
    F, n_det = len(cams), len(det_boxes)
    assoc = np.full(n_det, -1, np.int32); ious = np.zeros(n_det); stats = np.zeros((F, 4), np.int32)
    margin, frames = np.inf, []
    for f in range(F):
        pr = predict(cams[f], objs, K, rows, cols, p) if len(objs) else dict(boxes=np.zeros((0, 4)), flags=np.zeros(0, np.int32), margin=np.inf)
        frames.append(pr)
        margin = min(margin, pr["margin"])
        free = pr["flags"] == 1                      # eligible, not occluded, not yet claimed
        stats[f, 0] = int((pr["flags"] & 1).sum()); stats[f, 1] = int((pr["flags"] & 2).astype(bool).sum())
        for d in range(det_offsets[f], det_offsets[f + 1]):
            if not valid_box(det_boxes[d]):
                continue
            cand = np.nonzero(free & ((np.asarray(obj_labels) == det_labels[d]) if p["match_labels"] else True))[0]
            if len(cand) == 0:
                continue
            u = iou(det_boxes[d][None, :], pr["boxes"][cand])
            k = int(np.argmax(u))                    # first maximum: the lowest m on a tie
            best = u[k]
            if best > 0:
                margin = min(margin, abs(best - p["min_iou"]))
                if len(cand) > 1:
                    margin = min(margin, best - np.sort(u)[-2])
            if best >= p["min_iou"] and best > 0:
                assoc[d] = cand[k]; ious[d] = best; free[cand[k]] = False; stats[f, 2] += 1
    return dict(assoc=assoc, iou=ious, frame_stats=stats, frames=frames, margin=float(margin))
