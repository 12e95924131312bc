"""The numpy statement of esl_map_overlaps / esl_map_merge (include/esl.h, "map maintenance", steps 1 - 7), written for reading, not for
speed.  Test infrastructure: the product never imports it.  Beside every result it returns the margins that tests/map_merge_scenes.py
needs to decide whether exact agreement with another implementation is a fair demand."""
import functools

import numpy as np

DEFAULTS = dict(lattice=16, match_labels=1, min_iou=0.3, min_contain=0.7, max_pairs=4194304, pad=0)
GATE_SLACK = 1e-9


def params(**over):
    p = dict(DEFAULTS)
    for k, v in over.items():
        if k not in p:
            raise AttributeError(k)
        p[k] = v
    return p


# ---- step 2 ---------------------------------------------------------------------------------------------------------------------------------
def lattice_cells(n):
    """(n^3, 3) cells p in (px, py, pz) lexicographic order, and the mask of those whose triple k = 2 p + 1 - n lies in the ball"""
    p = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 3)
    k = 2 * p + 1 - n
    return p, (k * k).sum(1) <= n * n


@functools.lru_cache(maxsize=None)
def lattice(n):
    """(N_ball, 3) integer triples k, in order (read-only: the array is shared)"""
    p, inside = lattice_cells(n)
    k = (2 * p + 1 - n)[inside]
    k.setflags(write=False)
    return k


def n_ball(n):
    return len(lattice(n))


# ---- step 1 ---------------------------------------------------------------------------------------------------------------------------------
def rotation(q):
    """R of the NORMALISED quaternion (x, y, z, w)"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def prepare(objs):
    """per ellipsoid: valid, c, R, s, V, r"""
    objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    M = len(objs)
    out = dict(valid=np.zeros(M, bool), c=np.zeros((M, 3)), R=np.zeros((M, 3, 3)), s=np.ones((M, 3)), V=np.zeros(M), r=np.zeros(M))
    for i, v in enumerate(objs):
        with np.errstate(all="ignore"):
            nrm = np.sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6])
        s = np.abs(v[7:10])
        if not (np.isfinite(v).all() and np.isfinite(nrm) and nrm > 0 and (s > 0).all()):
            continue
        out["valid"][i] = True
        out["c"][i] = v[:3]; out["R"][i] = rotation(v[3:7] / nrm); out["s"][i] = s
        out["V"][i] = 4.0 / 3.0 * np.pi * s[0] * s[1] * s[2]; out["r"][i] = s.max()
    return out


# ---- step 3 ---------------------------------------------------------------------------------------------------------------------------------
def samples(pre, i, k, n):
    """the samples of ellipsoid i: x = c_i + R_i (s_i o u), u = k / n"""
    u = k / float(n)
    return pre["c"][i] + (pre["s"][i] * u) @ pre["R"][i].T


def q_of(pre, x, j):
    """q = |diag(1 / s_j) R_j^T (x - c_j)|^2 of the points x in ellipsoid j"""
    y = ((x - pre["c"][j]) @ pre["R"][j]) / pre["s"][j]
    return (y * y).sum(1)


def q_values(pre, i, j, k, n):
    """q of every sample of ellipsoid i in ellipsoid j"""
    return q_of(pre, samples(pre, i, k, n), j)


def measures(cnt_ij, cnt_ji, Vi, Vj, nb):
    inter = 0.5 * (cnt_ij * Vi + cnt_ji * Vj) / nb
    return inter / (Vi + Vj - inter), min(1.0, inter / min(Vi, Vj))


# ---- steps 4, 5 -----------------------------------------------------------------------------------------------------------------------------
def overlaps(objs, labels, **over):
    """dict(pairs (P, 2), counts (P, 2), iou, contain, link (P,) bool, n_pairs, n_candidates, over (bool: candidates > max_pairs),
    valid (M,), margins: q (closest |q - 1| of any sample), gate (closest relative distance of a gate quantity to its threshold),
    thr (closest distance of an iou / contain to its threshold))"""
    p = params(**over)
    n = p["lattice"]
    pre = prepare(objs)
    labels = np.asarray(labels, dtype=np.int32).reshape(-1)
    M = len(pre["valid"])
    k = lattice(n).astype(np.float64)
    nb = len(k)
    cand = []
    m_gate = np.inf
    for i in range(M):
        if not pre["valid"][i]:
            continue
        js = np.nonzero(pre["valid"][i + 1:])[0] + i + 1
        if p["match_labels"]:
            js = js[labels[js] == labels[i]]
        if len(js) == 0:
            continue
        d2 = ((pre["c"][js] - pre["c"][i]) ** 2).sum(1)
        thr = (pre["r"][js] + pre["r"][i]) ** 2 * (1 + GATE_SLACK)
        m_gate = min(m_gate, float(np.abs(d2 / thr - 1).min()))
        cand += [(i, int(j)) for j in js[d2 <= thr]]
    res = dict(n_candidates=len(cand), over=len(cand) > p["max_pairs"], valid=pre["valid"], n_valid=int(pre["valid"].sum()),
               margins=dict(q=np.inf, gate=m_gate, thr=np.inf), params=p)
    pairs, counts, ious, cons, links = [], [], [], [], []
    if not res["over"]:
        x = {}          # an ellipsoid's samples, made when its first candidate comes
        for i, j in cand:
            for m in (i, j):
                if m not in x:
                    x[m] = samples(pre, m, k, n)
            qa, qb = q_of(pre, x[i], j), q_of(pre, x[j], i)
            res["margins"]["q"] = min(res["margins"]["q"], float(np.abs(qa - 1).min()), float(np.abs(qb - 1).min()))
            ca, cb = int((qa <= 1).sum()), int((qb <= 1).sum())
            if ca + cb == 0:
                continue
            iou, con = measures(ca, cb, pre["V"][i], pre["V"][j], nb)
            res["margins"]["thr"] = min(res["margins"]["thr"], abs(iou - p["min_iou"]), abs(con - p["min_contain"]))
            pairs.append((i, j)); counts.append((ca, cb)); ious.append(iou); cons.append(con)
            links.append(iou >= p["min_iou"] or con >= p["min_contain"])
    res.update(pairs=np.array(pairs, np.int32).reshape(-1, 2), counts=np.array(counts, np.int32).reshape(-1, 2), iou=np.array(ious),
               contain=np.array(cons), link=np.array(links, bool), n_pairs=len(pairs))
    return res


def components(M, links):
    """group id (smallest member index) per object"""
    comp = np.arange(M)
    changed = True
    while changed:
        changed = False
        for a, b in links:
            lo = min(comp[a], comp[b])
            if comp[a] != lo or comp[b] != lo:
                comp[a] = comp[b] = lo
                changed = True
    return comp


# ---- steps 6, 7 -----------------------------------------------------------------------------------------------------------------------------
def merge(objs, labels, weights=None, obs_cam=None, obs_obj=None, **over):
    """dict(result: the fields of esl_merge_result, group, new_index, objs, labels, weights, obs_obj (or None), overlaps: the dict of
    overlaps())"""
    objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    labels = np.asarray(labels, dtype=np.int32).reshape(-1)
    M = len(objs)
    ov = overlaps(objs, labels, **over)
    have_list = obs_obj is not None and len(obs_obj) > 0
    if have_list:
        obs_cam = np.asarray(obs_cam, dtype=np.int64); obs_obj = np.asarray(obs_obj, dtype=np.int64)
    if weights is not None:
        w = np.asarray(weights, dtype=np.int64).reshape(-1)
    elif have_list:
        w = np.bincount(obs_obj[obs_obj >= 0], minlength=M).astype(np.int64)
    else:
        w = np.ones(M, np.int64)
    links = [] if ov["over"] else [tuple(pr) for pr, l in zip(ov["pairs"], ov["link"]) if l]
    comp = components(M, links)
    roots = np.nonzero(comp == np.arange(M))[0]
    number = {int(g): n for n, g in enumerate(roots)}
    new_index = np.array([number[int(g)] for g in comp], np.int32).reshape(-1)
    mo, ml, mw, sizes = np.zeros((len(roots), 10)), np.zeros(len(roots), np.int32), np.zeros(len(roots), np.int32), []
    for n, g in enumerate(roots):
        mem = np.nonzero(comp == g)[0]
        rep = min(mem, key=lambda m: (-w[m], m))
        mo[n] = objs[rep]; ml[n] = labels[rep]; mw[n] = w[mem].sum(); sizes.append(len(mem))
    out, n_conf = None, 0
    if obs_obj is not None:
        out = np.full(len(obs_obj), -1, np.int32)
    if have_list:
        best = {}
        for e in range(len(obs_obj)):
            o = int(obs_obj[e])
            if o < 0:
                continue
            key, order = (int(obs_cam[e]), int(new_index[o])), (-int(w[o]), o, e)
            if key not in best or order < best[key]:
                best[key] = order
        for e in range(len(obs_obj)):
            o = int(obs_obj[e])
            if o < 0:
                continue
            if best[(int(obs_cam[e]), int(new_index[o]))][2] == e:
                out[e] = new_index[o]
            else:
                n_conf += 1
    result = dict(status=3 if ov["over"] else 0, n_valid=ov["n_valid"], n_groups=len(roots), n_merged_groups=int(sum(s > 1 for s in sizes)),
                  largest_group=max(sizes) if sizes else 0, n_conflicts=n_conf, n_candidates=ov["n_candidates"], n_pairs=ov["n_pairs"],
                  n_links=len(links))
    if ov["over"]:          # status 3: the list is only cleaned, no conflict is settled
        result["n_conflicts"] = 0
        if have_list:
            out = np.where(obs_obj < 0, -1, obs_obj).astype(np.int32)
    return dict(result=result, group=comp.astype(np.int32), new_index=new_index, objs=mo, labels=ml, weights=mw, obs_obj=out, overlaps=ov)
