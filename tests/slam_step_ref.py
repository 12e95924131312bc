"""Extended-precision reference of one SLAM-mode trial step, recomputed from the device's OWN linearisation (the blocks
esl_lm_download returns): Schur complement, solve for x_c, back-substitution for x_o, the two retractions.  Everything is numpy.longdouble
(x87 extended: 64-bit mantissa), so the reference is ~2,000 times finer than the float64 arithmetic it judges and carries none of the
1e-6 of a numerically differentiated checker.  Beside it: the same quantities the plain float64 way (f64_yardsticks) -- the errors of
THOSE against the reference are what a float64 device is measured against -- and the table of graphs tests/test_gpu_slam_step.py runs
(their premises are asserted on the CPU in tests/test_slam_step_ref.py).  Test infrastructure; numpy only."""
import numpy as np

from oracle import np_oracle as npo

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is not an extended format here (eps %g): this reference needs one" % np.finfo(LD).eps
EPS64 = float(np.finfo(np.float64).eps)
SMALL_ANGLE = 1e-5          # se3_exp's branch (oracle/np_oracle.py: th < 1e-5)


# ---- packing and orders of esl_lm_download ----------------------------------------------------------------------------------
def unpack45(p):
    """packed upper triangle of a symmetric 9 x 9 block (row by row) -> the full block, dtype kept"""
    H = np.zeros((9, 9), dtype=np.asarray(p).dtype)
    iu = np.triu_indices(9)
    H[iu] = p
    H.T[iu] = p
    return H


def lower_to_full(S, n, lda):
    """which = 6: (n + 1) x n column-major, lower triangle of S, row n = b_s  ->  full S, b_s"""
    M = np.asarray(S).reshape(n, lda).T
    L = M[:n, :n]
    return np.tril(L) + np.tril(L, -1).T, M[n, :n].copy()


def edge_order(g):
    """(camera, ellipsoid) of every edge in the order of which = 9: stable sort by ellipsoid, bbox edges first, 3-D edges from
    n_bbox on (include/esl.h, esl_lm_download)"""
    ob, oe = np.argsort(g.bbox_obj, kind="stable"), np.argsort(g.e3d_obj, kind="stable")
    return (np.concatenate([g.bbox_cam[ob], g.e3d_cam[oe]]).astype(np.int64),
            np.concatenate([g.bbox_obj[ob], g.e3d_obj[oe]]).astype(np.int64))


def cam_slots(g):
    """slot of every camera among the free ones (-1: fixed)"""
    free = ~g.cam_fixed.astype(bool)
    slot = -np.ones(g.n_cams, dtype=np.int64)
    slot[free] = np.arange(int(free.sum()))
    return slot


def odom_pairs(g):
    """the (slot, slot) pairs of free cameras an odometry edge joins, low slot first"""
    slot = cam_slots(g)
    out = set()
    for i, j in zip(g.odom_i.tolist(), g.odom_j.tolist()):
        a, b = int(slot[i]), int(slot[j])
        if a >= 0 and b >= 0 and a != b:
            out.add((min(a, b), max(a, b)))
    return sorted(out)


# ---- small dense linear algebra in longdouble (numpy.linalg has none) -------------------------------------------------------
def chol_ld(A):
    A = np.array(A, dtype=LD)
    n = len(A)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0, "not positive definite"
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def inv_spd_ld(A):
    """inverse of a small symmetric positive definite matrix through its longdouble Cholesky factor"""
    A = np.asarray(A, dtype=LD)
    L = chol_ld(A)
    n = len(L)
    Li = np.zeros((n, n), dtype=LD)
    for j in range(n):
        Li[j, j] = 1 / L[j, j]
        for i in range(j + 1, n):
            Li[i, j] = -(L[i, j:i] @ Li[j:i, j]) / L[i, i]
    X = Li.T @ Li
    # one Newton step X + X (I - A X) on residuals of doubled precision: the factorisation alone leaves cond(A) * eps(longdouble),
    # which at the small damping (cond 1e4 .. 1e5) is all of the 1e-15 this reference is held to
    I = np.eye(n, dtype=LD)
    R = np.stack([residual_ld(A, X[:, j], I[:, j]) for j in range(n)], axis=1)
    X = X + X @ R
    return (X + X.T) / 2


_SPLIT = LD(2) ** 32 + 1          # Veltkamp's constant for a 64-bit mantissa


def _split(a):
    t = _SPLIT * a
    hi = t - (t - a)
    return hi, a - hi


def residual_ld(A, x, b):
    """b - A x with every product and every sum error-free transformed (Dekker's two-product, Knuth's two-sum; Ogita, Rump and Oishi's
    Dot2): the result is as if computed in twice longdouble's precision and rounded once, so a refinement on it is limited by the
    rounding of x itself and not by cond(A) * eps(longdouble)"""
    s = np.array(b, dtype=LD)
    c = np.zeros(len(s), dtype=LD)
    for j in range(len(x)):
        a, xj = A[:, j], x[j]
        if xj == 0:
            continue
        p = a * xj
        ah, al = _split(a)
        xh, xl = _split(xj)
        e = al * xl - (((p - ah * xh) - al * xh) - ah * xl)          # a * xj = p + e exactly
        t = s - p
        v = t - s
        c += ((s - (t - v)) + (-p - v)) - e                            # s - p = t + (that) exactly
        s = t
    return s + c


def solve_ref(A, b, max_steps=12):
    """Iterative refinement: float64 factorisation (numpy.linalg.solve), longdouble residuals (residual_ld), until the correction
    stops shrinking.  Returns (x, max-norm of the last correction applied)."""
    A = np.asarray(A, dtype=LD); b = np.asarray(b, dtype=LD)
    A64 = A.astype(np.float64)
    x = np.zeros(len(b), dtype=LD)
    if len(b) == 0:
        return x, 0.0
    last = np.inf
    for _ in range(max_steps):
        r = residual_ld(A, x, b)
        d = np.linalg.solve(A64, r.astype(np.float64)).astype(LD)
        size = float(np.abs(d).max())
        if size >= 0.5 * last:
            break
        x = x + d
        last = size
        if size == 0.0:
            break
    return x, last


# ---- the step -----------------------------------------------------------------------------------------------------------------
class Blocks:
    """the device's linearisation as longdouble arrays, and the per-ellipsoid (camera slot -> summed W) lists"""

    def __init__(self, g, Hoo45, bo, Hcc, bc, W, drop=()):
        """Hoo45 (N, 45), bo (N, 9), Hcc (nf, 6, 6), bc (nf, 6), W (54, n_edges) or None (no camera-ellipsoid block: every ellipsoid fixed);
        drop: edge positions left out of the sums (for planting an error)"""
        self.g, self.N = g, g.n_objs
        self.slot = cam_slots(g)
        self.nf = int((self.slot >= 0).sum())
        self.Hoo = np.array([unpack45(np.asarray(p, dtype=LD)) for p in np.asarray(Hoo45).reshape(self.N, 45)]).reshape(self.N, 9, 9)
        self.bo = np.asarray(bo, dtype=LD).reshape(self.N, 9)
        self.Hcc = np.asarray(Hcc, dtype=LD).reshape(self.nf, 6, 6)
        self.bc = np.asarray(bc, dtype=LD).reshape(self.nf, 6)
        self.pairs = odom_pairs(g)
        self.Wsum = [dict() for _ in range(self.N)]          # per ellipsoid: slot -> 6 x 9, summed over the pair's edges
        if W is not None:
            ucam, uobj = edge_order(g)
            W = np.asarray(W, dtype=LD).reshape(54, len(ucam))
            for u in range(len(ucam)):
                s = int(self.slot[ucam[u]])
                if s < 0 or u in drop:
                    continue
                d = self.Wsum[int(uobj[u])]
                blk = W[:, u].reshape(6, 9)
                d[s] = d[s] + blk if s in d else blk.copy()

    def stacked(self, o):
        """(slots ascending, (6k, 9) stack of their W blocks) of ellipsoid o"""
        slots = sorted(self.Wsum[o])
        if not slots:
            return slots, np.zeros((0, 9), dtype=LD)
        return slots, np.concatenate([self.Wsum[o][s] for s in slots], axis=0)


def rows_of(slots):
    return (6 * np.asarray(slots, dtype=np.int64)[:, None] + np.arange(6)[None, :]).reshape(-1)


def odom_mask(B):
    m = np.zeros((B.nf, B.nf), dtype=bool)
    for a, b in B.pairs:
        m[a, b] = m[b, a] = True
    return m


def schur_ref(B, lam, lam_obj=None):
    """S_ref = diag(H_cc + lam I) - sum_o W_o (H_oo + lam I)^-1 W_o^T and b_s_ref = b_c - sum_o W_o (H_oo + lam I)^-1 b_o, accumulated
    per ellipsoid.  The odometry off-diagonal blocks of H_cc are not downloadable: S_ref lacks them, and the mask of those block
    pairs is returned.  Returns (S_ref, b_s_ref, mask (nf, nf), Dinv (N, 9, 9)).  lam_obj: the damping of the ellipsoid blocks where
    it shall differ (for planting an error)."""
    lam = LD(lam)
    lo = lam if lam_obj is None else LD(lam_obj)
    n = 6 * B.nf
    S = np.zeros((n, n), dtype=LD)
    bs = B.bc.reshape(-1).copy()
    I6, I9 = np.eye(6, dtype=LD), np.eye(9, dtype=LD)
    for s in range(B.nf):
        S[6 * s:6 * s + 6, 6 * s:6 * s + 6] = B.Hcc[s] + lam * I6
    Dinv = np.zeros((B.N, 9, 9), dtype=LD)
    for o in range(B.N):
        Dinv[o] = inv_spd_ld(B.Hoo[o] + lo * I9)
        slots, Wst = B.stacked(o)
        if not slots:
            continue
        r = rows_of(slots)
        Y = Wst @ Dinv[o]
        S[np.ix_(r, r)] -= Y @ Wst.T
        bs[r] -= Y @ B.bo[o]
    return S, bs, odom_mask(B), Dinv


def schur_terms_on_pairs(B, Dinv):
    """sum_o W_io (H_oo + lam I)^-1 W_jo^T for the odometry-joined pairs (i < j): {(i, j): 6 x 6}"""
    out = {p: np.zeros((6, 6), dtype=LD) for p in B.pairs}
    for o in range(B.N):
        d = B.Wsum[o]
        for (a, b) in B.pairs:
            if a in d and b in d:
                out[(a, b)] += d[a] @ Dinv[o] @ d[b].T
    return out


def with_blocks(S, blocks):
    """S with the 6 x 6 blocks {(i, j): block at rows i, columns j} (and their transposes) set"""
    S = S.copy()
    for (a, b), blk in blocks.items():
        S[6 * a:6 * a + 6, 6 * b:6 * b + 6] = blk
        S[6 * b:6 * b + 6, 6 * a:6 * a + 6] = blk.T
    return S


def pair_blocks(S, pairs):
    return {(a, b): np.asarray(S)[6 * a:6 * a + 6, 6 * b:6 * b + 6].copy() for a, b in pairs}


def backsub_ref(B, Dinv, xc):
    """x_o = (H_oo + lam I)^-1 (b_o - W^T x_c) per ellipsoid"""
    xc = np.asarray(xc, dtype=LD).reshape(B.nf, 6)
    xo = np.zeros((B.N, 9), dtype=LD)
    for o in range(B.N):
        t = B.bo[o].copy()
        for s, blk in B.Wsum[o].items():
            t -= blk.T @ xc[s]
        xo[o] = Dinv[o] @ t
    return xo


def step_scale(B, lam, xc, xo):
    """g2o's computeScale: sum_j x_j (lam x_j + b_j) over all unknowns"""
    xc = np.asarray(xc, dtype=LD).reshape(-1); xo = np.asarray(xo, dtype=LD).reshape(-1)
    return (xc * (LD(lam) * xc + B.bc.reshape(-1))).sum() + (xo * (LD(lam) * xo + B.bo.reshape(-1))).sum()


def rel_err(a, ref):
    """max-norm error relative to the reference's max-norm"""
    ref = np.asarray(ref, dtype=LD).reshape(-1)
    if not ref.size:
        return 0.0
    d = float(np.abs(np.asarray(a, dtype=LD).reshape(-1) - ref).max())
    m = float(np.abs(ref).max())
    return d if m == 0.0 else d / m


def f64_yardsticks(B, lam, hodo, ref):
    """The step the plain float64 way, twice -- (1) numpy.linalg.solve of the whole (H + lam I) x = b, assembled from the blocks (hodo:
    {(i, j): 6 x 6} the odometry off-diagonal blocks of H_cc), (2) numpy Schur complement + numpy.linalg.cholesky + back-substitution --
    each against the longdouble reference ref = dict(S, bs, xc, xo; S, bs WITHOUT the odometry blocks, mask their place).  Returns
    dict(S, bs, xc, xo): per quantity the larger of the float64 errors (max-norm, relative to the quantity's max-norm)."""
    nf, N = B.nf, B.N
    n, m = 6 * nf, 9 * N
    Hcc, bc = B.Hcc.astype(np.float64), B.bc.astype(np.float64)
    Hoo, bo = B.Hoo.astype(np.float64), B.bo.astype(np.float64)
    lam = float(lam)
    hodo64 = {k: np.asarray(v, dtype=LD).astype(np.float64) for k, v in hodo.items()}
    # (1) the whole system
    H = np.zeros((n + m, n + m))
    for s in range(nf):
        H[6 * s:6 * s + 6, 6 * s:6 * s + 6] = Hcc[s]
    H[:n, :n] = with_blocks(H[:n, :n], hodo64)
    for o in range(N):
        H[n + 9 * o:n + 9 * o + 9, n + 9 * o:n + 9 * o + 9] = Hoo[o]
        for s, blk in B.Wsum[o].items():
            H[6 * s:6 * s + 6, n + 9 * o:n + 9 * o + 9] = blk.astype(np.float64)
            H[n + 9 * o:n + 9 * o + 9, 6 * s:6 * s + 6] = blk.astype(np.float64).T
    x = np.linalg.solve(H + lam * np.eye(n + m), np.concatenate([bc.reshape(-1), bo.reshape(-1)]))
    direct = dict(xc=rel_err(x[:n], ref["xc"]), xo=rel_err(x[n:], ref["xo"]) if m else 0.0)
    # (2) Schur + Cholesky + back-substitution
    S = np.zeros((n, n))
    bs = bc.reshape(-1).copy()
    Dinv = np.zeros((N, 9, 9))
    for s in range(nf):
        S[6 * s:6 * s + 6, 6 * s:6 * s + 6] = Hcc[s] + lam * np.eye(6)
    for o in range(N):
        Dinv[o] = np.linalg.inv(Hoo[o] + lam * np.eye(9))
        slots, Wst = B.stacked(o)
        if not slots:
            continue
        Wst = Wst.astype(np.float64)
        r = rows_of(slots)
        Y = Wst @ Dinv[o]
        S[np.ix_(r, r)] -= Y @ Wst.T
        bs[r] -= Y @ bo[o]
    keep = np.kron(~ref["mask"], np.ones((6, 6), dtype=bool)) if nf else np.zeros((0, 0), dtype=bool)
    out = dict(S=rel_err(np.where(keep, S, 0), np.where(keep, ref["S"], 0)), bs=rel_err(bs, ref["bs"]))
    Sfull = with_blocks(S, {(a, c): v + S[6 * a:6 * a + 6, 6 * c:6 * c + 6] for (a, c), v in hodo64.items()})
    L = np.linalg.cholesky(Sfull)
    xc = np.linalg.solve(L.T, np.linalg.solve(L, bs))
    xo = np.zeros((N, 9))
    for o in range(N):
        t = bo[o].copy()
        for s, blk in B.Wsum[o].items():
            t -= blk.astype(np.float64).T @ xc[6 * s:6 * s + 6]
        xo[o] = Dinv[o] @ t
    out["xc"] = max(direct["xc"], rel_err(xc, ref["xc"]))
    out["xo"] = max(direct["xo"], rel_err(xo, ref["xo"])) if m else 0.0
    out["xc_direct"], out["xo_direct"] = direct["xc"], direct["xo"]
    return out


def reference_step(B, lam, S_dev=None, hodo=None, lam_obj=None):
    """The whole reference step.  The odometry off-diagonal blocks come either from the device's S (S_dev: full float64 matrix; they
    are S_dev's blocks, and hodo = those + the reference's Schur terms) or from hodo itself ({(i, j): block of H_cc}).  Returns dict(S,
    bs: without the odometry blocks; mask; Dinv; terms; hodo; Sc: S with them; xc, xc_last; xo)."""
    S, bs, mask, Dinv = schur_ref(B, lam, lam_obj)
    terms = schur_terms_on_pairs(B, Dinv)
    S = with_blocks(S, {p: np.zeros((6, 6), dtype=LD) for p in B.pairs})          # what is left there is the Schur term alone: not part of S_ref
    if S_dev is not None:
        sd = pair_blocks(np.asarray(S_dev, dtype=LD), B.pairs)
        hodo = {p: sd[p] + terms[p] for p in B.pairs}
    else:
        hodo = {p: np.asarray(hodo[p], dtype=LD) for p in B.pairs}
        sd = {p: hodo[p] - terms[p] for p in B.pairs}
    Sc = with_blocks(S, sd)
    xc, last = solve_ref(Sc, bs)
    xo = backsub_ref(B, Dinv, xc)
    return dict(S=S, bs=bs, mask=mask, Dinv=Dinv, terms=terms, hodo=hodo, Sc=Sc, xc=xc, xc_last=last, xo=xo)


# ---- retractions in longdouble (oracle/np_oracle.py: se3_exp, cam_oplus, obj_oplus) ---------------------------------------------
def _quat_to_R_ld(q):
    x, y, z, w = [LD(v) for v in q]
    s = 2 / (x * x + y * y + z * z + w * w)
    return np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]], dtype=LD)


def _R_to_quat_ld(R):
    """the rotation's unit quaternion, w >= 0, through the largest of the four components (Shepperd)"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    c = [R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1], t]
    k = int(np.argmax([float(v) for v in c]))
    r = np.sqrt(1 + c[k])
    q = np.zeros(4, dtype=LD)
    if k == 3:
        q[:] = [(R[2, 1] - R[1, 2]) / (2 * r), (R[0, 2] - R[2, 0]) / (2 * r), (R[1, 0] - R[0, 1]) / (2 * r), r / 2]
    elif k == 0:
        q[:] = [r / 2, (R[0, 1] + R[1, 0]) / (2 * r), (R[0, 2] + R[2, 0]) / (2 * r), (R[2, 1] - R[1, 2]) / (2 * r)]
    elif k == 1:
        q[:] = [(R[0, 1] + R[1, 0]) / (2 * r), r / 2, (R[1, 2] + R[2, 1]) / (2 * r), (R[0, 2] - R[2, 0]) / (2 * r)]
    else:
        q[:] = [(R[0, 2] + R[2, 0]) / (2 * r), (R[1, 2] + R[2, 1]) / (2 * r), r / 2, (R[1, 0] - R[0, 1]) / (2 * r)]
    q = q / np.sqrt(q @ q)
    return -q if q[3] < 0 else q


def _T_from7_ld(v):
    T = np.eye(4, dtype=LD)
    T[:3, :3] = _quat_to_R_ld(v[3:7])
    T[:3, 3] = np.asarray(v[0:3], dtype=LD)
    return T


def _T_to7_ld(T):
    return np.concatenate([T[:3, 3], _R_to_quat_ld(T[:3, :3])])


def _skew_ld(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=LD)


def se3_exp_ld(u):
    """np_oracle.se3_exp in longdouble, its small-angle branch (th < 1e-5: R = I + W + W^2 put back on the rotations through the
    normalised quaternion, V = I + W + W^2) where np_oracle has it"""
    u = np.asarray(u, dtype=LD)
    w, ups = u[:3], u[3:]
    th = np.sqrt(w @ w)
    W = _skew_ld(w)
    I = np.eye(3, dtype=LD)
    if th < LD(SMALL_ANGLE):
        R = I + W + W @ W
        V = R.copy()
        t = np.sqrt(R[0, 0] + R[1, 1] + R[2, 2] + 1)             # Eigen's Quaterniond(Matrix3d), trace > 0
        q = np.array([(R[2, 1] - R[1, 2]) / (2 * t), (R[0, 2] - R[2, 0]) / (2 * t), (R[1, 0] - R[0, 1]) / (2 * t), t / 2], dtype=LD)
        R = _quat_to_R_ld(q / np.sqrt(q @ q))
    else:
        R = I + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * (W @ W)
        V = I + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * (W @ W)
    T = np.eye(4, dtype=LD)
    T[:3, :3] = R
    T[:3, 3] = V @ ups
    return T


def cam_oplus_ld(cam7, u):
    """exp(u) * Tcw on the 7-vector (x y z qx qy qz qw), quaternion unit with w >= 0"""
    return _T_to7_ld(se3_exp_ld(u) @ _T_from7_ld(cam7))


def obj_oplus_ld(obj10, u):
    """ellipsoid::exp_update on the 10-vector: pose * exp(u[:6]), scale + u[6:9]"""
    u = np.asarray(u, dtype=LD)
    return np.concatenate([_T_to7_ld(_T_from7_ld(obj10) @ se3_exp_ld(u[:6])), np.asarray(obj10[7:10], dtype=LD) + u[6:9]])


def cam_oplus_f64(cam7, u):
    """np_oracle's float64 retraction on the 7-vector"""
    return npo.T_to7(npo.cam_oplus(npo.T_from7(np.asarray(cam7, dtype=np.float64)), np.asarray(u, dtype=np.float64)))


def obj_oplus_f64(obj10, u):
    T, s = npo.obj_oplus(*npo.obj_from10(np.asarray(obj10, dtype=np.float64)), np.asarray(u, dtype=np.float64))
    return npo.obj_to10(T, s)


def state_err(a, ref):
    """max-norm distance of two 7- or 10-vectors, the quaternion taken up to its sign"""
    a = np.asarray(a, dtype=LD); ref = np.asarray(ref, dtype=LD)
    dq = min(float(np.abs(a[3:7] - ref[3:7]).max()), float(np.abs(a[3:7] + ref[3:7]).max()))
    rest = np.concatenate([a[:3] - ref[:3], a[7:] - ref[7:]])
    return max(dq, float(np.abs(rest).max()))


# ---- the graphs of tests/test_gpu_slam_step.py ------------------------------------------------------------------------------------
BASE_ARGS = dict(n_cams=100, n_objs=30, n_bbox_target=3000, seed=3, slam=True, frac_3d=0.3)

# name: (kind, cameras, ellipsoids, premises).  "sub": Graph.subset(range(cameras), the `ellipsoids` ellipsoids with the most edges among
# those cameras) of make_graph(**BASE_ARGS); premises are asserted by tests/test_slam_step_ref.py::test_case_premises:
#   nf free cameras; p6 / p9: 128-wide panels 6 nf and 9 N take; seg: 16-camera segments the free cameras take;
#   obj_list / cam_list "long": the longest per-ellipsoid / per-camera list is longer than 64; mixed: a free camera holds a bbox and a 3-D
#   edge on one ellipsoid; every_obj_seen: every ellipsoid has an edge from a free camera
CASES = {
    "A_2c_1e": ("sub", 2, 1, dict(nf=1, p6=1, p9=1, every_obj_seen=True)),
    "A_2c_2e": ("sub", 2, 2, dict(nf=1, p6=1, p9=1, every_obj_seen=True)),
    "A_3c_1e": ("sub", 3, 1, dict(nf=2, p6=1, p9=1, every_obj_seen=True)),
    "A_6c_2e": ("sub", 6, 2, dict(nf=5, p6=1, p9=1, every_obj_seen=True, mixed=True)),
    "B_22c_2e": ("sub", 22, 2, dict(nf=21, p6=1, p9=1, seg=2, every_obj_seen=True)),
    "B_22c_15e": ("sub", 22, 15, dict(nf=21, p6=1, p9=2, seg=2, every_obj_seen=True, mixed=True)),
    "B_23c_2e": ("sub", 23, 2, dict(nf=22, p6=2, p9=1, seg=2, every_obj_seen=True)),
    "B_23c_15e": ("sub", 23, 15, dict(nf=22, p6=2, p9=2, seg=2, every_obj_seen=True, mixed=True)),
    "C_44c_29e": ("sub", 44, 29, dict(nf=43, p6=3, p9=3, seg=3, every_obj_seen=True, mixed=True)),
    "C_17c_15e": ("sub", 17, 15, dict(nf=16, p6=1, p9=2, seg=1, every_obj_seen=True, mixed=True)),
    "C_18c_15e": ("sub", 18, 15, dict(nf=17, p6=1, p9=2, seg=2, every_obj_seen=True, mixed=True)),
    "D_66c_29e": ("sub", 66, 29, dict(nf=65, p6=4, p9=3, seg=5, obj_list="long", every_obj_seen=True, mixed=True)),
    "D_long_camera_list": ("make", dict(n_cams=6, n_objs=200, n_bbox_target=2000, seed=1, slam=True, frac_3d=0.5), None,
                           dict(nf=5, p6=1, p9=15, cam_list="long", mixed=True)),
    "E_257c_40e": ("make", dict(n_cams=257, n_objs=40, n_bbox_target=6 * 257, seed=41, slam=True), None,
                   dict(nf=256, p6=12, p9=3, seg=16, obj_list="long", mixed=True)),
}
F_CAMS = (2, 3, 4, 5, 6, 9, 10, 17, 18, 65, 66)      # all ellipsoids fixed: nf = 1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 65 in the cyclic reduction
F_OBJS = 15

# the large damping of each case, as a multiple of max_diag: every camera's |omega| of x_c is then below se3_exp's small-angle
# threshold (asserted from the checker's system on the CPU and from the reference on the device's blocks); the small one is 1e-5
LAM_SMALL = 1e-5
LAM_BIG = 1e4

_base = {}


def base_graph(pkg):
    if "g" not in _base:
        _base["g"] = pkg.synth.make_graph(**BASE_ARGS)[:3]
    return _base["g"]


def sub_case(pkg, n_cams, n_objs):
    g, c, o = base_graph(pkg)
    inb, ine = g.bbox_cam < n_cams, g.e3d_cam < n_cams
    cnt = np.bincount(np.concatenate([g.bbox_obj[inb], g.e3d_obj[ine]]).astype(np.int64), minlength=g.n_objs)
    objs = np.sort(np.argsort(-cnt, kind="stable")[:n_objs])
    return g.subset(np.arange(n_cams), objs), c[:n_cams].copy(), o[objs].copy()


def build_case(pkg, name):
    """(graph, cameras, ellipsoids) of one row of CASES"""
    kind, a, b, _ = CASES[name]
    if kind == "sub":
        return sub_case(pkg, a, b)
    return pkg.synth.make_graph(**a)[:3]


def build_f_case(pkg, n_cams, odometry):
    """case F: n_cams cameras against F_OBJS ellipsoids (all of them to be flagged fixed), with or without the odometry chain"""
    g, c, o = sub_case(pkg, n_cams, F_OBJS)
    if not odometry:
        g = pkg.Graph(g.K, g.n_cams, g.n_objs, g.cam_fixed, g.bbox_cam, g.bbox_obj, g.bbox_meas, g.bbox_weight, g.e3d_cam, g.e3d_obj,
                      g.e3d_meas, g.e3d_weight, g.grav_obj, g.grav_normal, g.grav_weight)
    return g, c, o


def per_cam_counts(g):
    return np.bincount(np.concatenate([g.bbox_cam, g.e3d_cam]).astype(np.int64), minlength=g.n_cams)


def per_obj_counts(g):
    """edges from FREE cameras per ellipsoid"""
    free = ~g.cam_fixed.astype(bool)
    return np.bincount(np.concatenate([g.bbox_obj[free[g.bbox_cam]], g.e3d_obj[free[g.e3d_cam]]]).astype(np.int64), minlength=g.n_objs)


def has_bbox_and_e3d_pair(g):
    bb = set(zip(g.bbox_cam.tolist(), g.bbox_obj.tolist()))
    return any((c, o) in bb and not g.cam_fixed[c] for c, o in zip(g.e3d_cam.tolist(), g.e3d_obj.tolist()))


def blocks_from_dense(g, H, b, fidx):
    """the checker's dense H, b (oracle/pyoracle.py build_system: cameras first, then ellipsoids) cut into the blocks the device
    downloads: (Blocks, hodo)"""
    slot = cam_slots(g)
    nf, N = int((slot >= 0).sum()), g.n_objs
    n = 6 * nf
    assert all(fidx[ci] == 6 * slot[ci] for ci in range(g.n_cams) if slot[ci] >= 0)
    assert all(fidx[g.n_cams + o] == n + 9 * o for o in range(N)) and len(b) == n + 9 * N
    iu = np.triu_indices(9)
    Hoo45 = np.array([H[n + 9 * o:n + 9 * o + 9, n + 9 * o:n + 9 * o + 9][iu] for o in range(N)])
    Hcc = np.array([H[6 * s:6 * s + 6, 6 * s:6 * s + 6] for s in range(nf)])
    ucam, uobj = edge_order(g)
    W = np.zeros((54, len(ucam)))
    seen = set()
    for u in range(len(ucam)):                                  # the pair's whole block on its first edge, zero on its others
        s, o = int(slot[ucam[u]]), int(uobj[u])
        if s >= 0 and (s, o) not in seen:
            seen.add((s, o))
            W[:, u] = H[6 * s:6 * s + 6, n + 9 * o:n + 9 * o + 9].reshape(-1)
    B = Blocks(g, Hoo45, b[n:].reshape(N, 9), Hcc, b[:n].reshape(nf, 6), W)
    return B, pair_blocks(H[:n, :n], B.pairs)
