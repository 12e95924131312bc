"""numpy reference of ESL_SOLVER_PCG: block-Jacobi preconditioned conjugate gradients on the reduced camera system S x = b_s from
x_0 = 0, stopping at the first k with |r_k|_2 <= rel_tol |b_s|_2 (g2o's LinearSolverPCG on the Schur complement).  Two variants: on
a dense S, and matrix-free from the camera block, the camera-ellipsoid coupling and the ellipsoids' 9 x 9 blocks.

Everything runs in numpy's extended precision (np.longdouble: 64-bit mantissa on x86), the small inverses included: at the
condition numbers of these systems (1e5) two float64 runs of the SAME recurrence that differ only in summation order end 2e-12 of
max|x| apart, which would make the reference its own largest error.  Test infrastructure only."""
import numpy as np

LD = np.longdouble


def diag_blocks(S, bs=6):
    n = S.shape[0] // bs
    return np.stack([S[bs * k:bs * k + bs, bs * k:bs * k + bs] for k in range(n)]) if n else np.zeros((0, bs, bs), S.dtype)


def inv_blocks(B):
    """inverses of a stack of symmetric positive definite blocks in extended precision (Gauss-Jordan, no pivoting)"""
    B = np.array(B, dtype=LD)
    k, d, _ = B.shape
    A = np.concatenate([B, np.broadcast_to(np.eye(d, dtype=LD), (k, d, d))], axis=2)
    for i in range(d):
        A[:, i, :] = A[:, i, :] / A[:, i, i:i + 1]
        for j in range(d):
            if j != i:
                A[:, j, :] = A[:, j, :] - A[:, j, i:i + 1] * A[:, i, :]
    return A[:, :, d:]


def _pcg(matvec, blocks, b, rel_tol, max_iters):
    """returns x, iterations, |r| / |b| at exit, converged"""
    n = len(b)
    Minv = inv_blocks(blocks)
    prec = lambda r: np.einsum("kij,kj->ki", Minv, r.reshape(-1, 6)).reshape(n)
    x = np.zeros(n, dtype=LD)
    r = np.array(b, dtype=LD)
    bb = r @ r
    if bb == 0:
        return np.zeros(n), 0, 0.0, True
    thr = LD(rel_tol) * LD(rel_tol) * bb
    if bb <= thr:
        return np.zeros(n), 0, 1.0, True
    z = prec(r)
    p = z.copy()
    rz = r @ z
    for k in range(1, max_iters + 1):
        q = matvec(p)
        alpha = rz / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        rr = r @ r
        if rr <= thr:
            return np.array(x, dtype=np.float64), k, float(np.sqrt(rr / bb)), True
        z = prec(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return np.array(x, dtype=np.float64), max_iters, float(np.sqrt((r @ r) / bb)), False


def pcg_dense(S, b, rel_tol=1e-10, max_iters=1000, blocks=None):
    """PCG on a dense S; blocks: the preconditioner's 6 x 6 blocks (default: the diagonal blocks of S)"""
    S = np.array(S, dtype=LD)
    return _pcg(lambda p: S @ p, diag_blocks(S) if blocks is None else blocks, b, rel_tol, max_iters)


def split_system(H, b, n_cam, lam):
    """the damped full system (cameras first) -> camera block, coupling, the ellipsoids' 9 x 9 blocks, the two right-hand sides"""
    Hl = np.array(H, dtype=LD) + LD(lam) * np.eye(len(b), dtype=LD)
    bl = np.array(b, dtype=LD)
    return Hl[:n_cam, :n_cam], Hl[:n_cam, n_cam:], diag_blocks(Hl[n_cam:, n_cam:], 9), bl[:n_cam], bl[n_cam:]


def schur_dense(Hcc, W, D, bc, bo):
    """S and b_s formed explicitly (extended precision)"""
    n, no = Hcc.shape[0], len(D)
    Dinv = inv_blocks(D)
    WD = np.einsum("aoi,oij->aoj", W.reshape(n, no, 9), Dinv).reshape(n, no * 9)
    return Hcc - WD @ W.T, bc - WD @ bo


def pcg_matrix_free(Hcc, W, D, bc, bo, rel_tol=1e-10, max_iters=1000):
    """S = Hcc - W D^-1 W^T is never formed: one product is W^T p, the 9 x 9 solves, W t; the preconditioner's blocks are
    Hcc_cc - sum_o W_co D_o^-1 W_co^T.  Returns x, iterations, |r| / |b|, converged, b_s, the blocks."""
    n, no = Hcc.shape[0], len(D)
    Dinv = inv_blocks(D)
    apply_dinv = lambda v: np.einsum("kij,kj->ki", Dinv, v.reshape(-1, 9)).reshape(-1)
    bs = bc - W @ apply_dinv(bo)
    Wc = W.reshape(n // 6, 6, no, 9)
    blocks = diag_blocks(Hcc) - np.einsum("caoi,oij,cboj->cab", Wc, Dinv, Wc)
    matvec = lambda p: Hcc @ p - W @ apply_dinv(W.T @ p)
    x, k, res, ok = _pcg(matvec, blocks, bs, rel_tol, max_iters)
    return x, k, res, ok, bs, blocks
