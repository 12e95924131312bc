"""The twisted (two-directional) solve of one camera segment, in numpy and in the library's scaling: what csrc/esl_cf_sweep.hpp computes
(k_cf_twist: the per-slot matrices; k_cf_sweep: the columns) written from the definitions.

Segment p of the dissected camera chain has n interior slots; G_p is block tridiagonal and positive definite, diagonal blocks A_i
(damping included), sub-diagonal blocks B_i = G_p(i + 1, i) (the library's cf_B: the coupling of the last interior slot to the separator
is not part of G_p).  The library's forward factor (k_cf_chain, k_cf_factor_blocks):

    L_i = chol(D+_i),  D+_0 = A_0,  D+_{i+1} = A_{i+1} - G_i^T G_i,  G_i = L_i^-1 B_i^T,  M_i = L_i^-1 G_{i-1}^T  (M_0 = 0)

and for a column w of W with V_i = L_i^-1 w_i (k_cf_edge_scale's records) the forward substitution x_i = V_i - M_i x_{i-1}, so that
y+_i = w_i - B_{i-1} D+_{i-1}^-1 y+_{i-1} = L_i x_i.  The mirror image from the last interior slot, scaled the same way
(u_i = L_i^-1 y-_i, y-_i = w_i - B_i^T D-_{i+1}^-1 y-_{i+1}, D-_i = A_i - B_i^T D-_{i+1}^-1 B_i):

    K_i = chol(D-_i),  D-_{n-1} = A_{n-1},  H_i = K_{i+1}^-1 G_i^T,  S_i = H_i^T H_i  (= L_i^-1 B_i^T D-_{i+1}^-1 B_i L_i^-T)
    D-_i = A_i - L_i S_i L_i^T
    Q_i = H_i^T K_{i+1}^-1 L_{i+1}   (Q_{n-1} = 0)          u_i = V_i - Q_i u_{i+1}
    P_i = (I - S_i)^-1               (P_{n-1} = I)          the twisted pivot D+_i + D-_i - A_i = L_i (I - S_i) L_i^T

Combination: Z_i = (D+_i + D-_i - A_i)^-1 (y+_i + y-_i - w_i) is block i of G_p^-1 w, and what the assembly reads is

    Y_i = L_i^T Z_i = P_i (x_i + u_i - V_i).

x_i is zero in front of the column's first entry and u_i behind its last one, and u_i = V_i exactly AT the last one: behind the last
entry Y_i = P_i x_i, in front of the first Y_i = P_i u_i, and only between the two (last one excluded) both directions meet.
"""
import numpy as np


def _chol(a):
    return np.linalg.cholesky(a)


def _lsolve(l, b):
    """l^-1 b, l lower triangular: forward substitution, row by row (the order of the kernels)"""
    x = np.zeros_like(b, dtype=np.float64)
    for r in range(len(l)):
        x[r] = (b[r] - l[r, :r] @ x[:r]) / l[r, r]
    return x


def segment_matrices(A, B):
    """A: (n, 6, 6) diagonal blocks, B: (n - 1, 6, 6) with B[i] = G_p(i + 1, i).  Returns dict(L, G, M, P, Q), each (n, 6, 6), as above
    (G[n - 1] = 0: nothing behind the last interior slot)."""
    n = len(A)
    L = np.zeros((n, 6, 6)); G = np.zeros((n, 6, 6)); M = np.zeros((n, 6, 6)); P = np.zeros((n, 6, 6)); Q = np.zeros((n, 6, 6))
    D = A[0].copy()
    for i in range(n):
        L[i] = _chol(D)
        if i > 0:
            M[i] = _lsolve(L[i], G[i - 1].T)
        if i + 1 < n:
            G[i] = _lsolve(L[i], B[i].T)
            D = A[i + 1] - G[i].T @ G[i]
    P[n - 1] = np.eye(6)
    K = _chol(A[n - 1])
    for i in range(n - 2, -1, -1):
        H = _lsolve(K, G[i].T)
        S = H.T @ H
        C = _chol(np.eye(6) - S)
        Ci = _lsolve(C, np.eye(6))
        P[i] = Ci.T @ Ci
        Q[i] = H.T @ _lsolve(K, L[i + 1])
        Dm = A[i] - L[i] @ S @ L[i].T
        K = _chol((Dm + Dm.T) / 2)
    return dict(L=L, G=G, M=M, P=P, Q=Q)


def scaled_records(mats, w):
    """V_i = L_i^-1 w_i; w: (n, 6, k)"""
    return np.stack([_lsolve(mats["L"][i], w[i]) for i in range(len(w))])


def sweep(mats, V):
    """Y (n, 6, k) of the columns V (n, 6, k) the way k_cf_sweep forms it: the forward pass stores P_i x_i from the column's first
    entry on, the backward pass stores P_i u_i in front of it and adds P_i (u_i - V_i) between the first and the last entry."""
    n, _, k = V.shape
    M, P, Q = mats["M"], mats["P"], mats["Q"]
    Y = np.zeros_like(V)
    live = np.abs(V).max(axis=1) > 0                      # (n, k)
    for c in range(k):
        at = np.flatnonzero(live[:, c])
        if len(at) == 0:
            continue
        first, last = at[0], at[-1]
        x = np.zeros(6)
        for i in range(first, n):
            x = V[i, :, c] - M[i] @ x
            Y[i, :, c] = P[i] @ x
        u = np.zeros(6)
        for i in range(last, -1, -1):
            u = V[i, :, c] - Q[i] @ u
            if i < first:
                Y[i, :, c] = P[i] @ u
            elif i < last:
                Y[i, :, c] = Y[i, :, c] + P[i] @ (u - V[i, :, c])
    return Y


def substitution(mats, V):
    """The parent's route to the same Y: x by forward substitution, then the segment's own backward sweep Y_i = x_i - G_i Z_{i+1},
    Z_i = L_i^-T Y_i (k_cf_forward<2> + k_cf_seg_back)."""
    n = len(V)
    x = np.zeros_like(V); Y = np.zeros_like(V)
    for i in range(n):
        x[i] = V[i] - (mats["M"][i] @ x[i - 1] if i > 0 else 0)
    Z = np.zeros(V.shape[1:])
    for i in range(n - 1, -1, -1):
        Y[i] = x[i] - mats["G"][i] @ Z
        Z = np.linalg.solve(mats["L"][i].T, Y[i])
    return Y


def dense(A, B):
    """G_p as one dense matrix"""
    n = len(A)
    G = np.zeros((6 * n, 6 * n))
    for i in range(n):
        G[6 * i:6 * i + 6, 6 * i:6 * i + 6] = A[i]
        if i + 1 < n:
            G[6 * i + 6:6 * i + 12, 6 * i:6 * i + 6] = B[i]
            G[6 * i:6 * i + 6, 6 * i + 6:6 * i + 12] = B[i].T
    return G


def random_segment(n, rng):
    """A segment shaped like H_cc + lambda I of a camera chain: per-camera information from a few observations plus the odometry edges'
    J^T J between neighbours."""
    A = np.zeros((n, 6, 6)); B = np.zeros((max(n - 1, 0), 6, 6))
    for i in range(n):
        j = rng.standard_normal((6, 8))
        A[i] = 1e-2 * np.eye(6) + j @ j.T
    for i in range(n - 1):
        ja, jb = 3 * rng.standard_normal((6, 6)), 3 * rng.standard_normal((6, 6))
        A[i] += ja.T @ ja; A[i + 1] += jb.T @ jb; B[i] = jb.T @ ja
    return A, B
