"""Numpy reference of the robust kernels (esl_lm_set_robust): oracle/np_oracle.py's graph and LM loop with g2o's robustified
edges.  An edge with raw chi2 e = r^T Omega r adds rho0(e) to chi2 and rho1(e) Omega as its information to H, b
(g2o base_binary_edge.hpp / base_unary_edge.hpp robustInformation; the rho2 term is left out, as in g2o).  Test infrastructure."""
import numpy as np

from oracle import np_oracle as npo

KINDS = {"none": 0, "huber": 1, "pseudo_huber": 2, "cauchy": 3, "tukey": 4}
CLASSES = {"bbox": 0, "e3d": 1, "grav": 2, "odom": 3}


def robustify(kind, delta, e):
    """(rho0, rho1) restated from g2o core/robust_kernel_impl.cpp (RobustKernelHuber / PseudoHuber / Cauchy / Tukey::robustify)."""
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    dsqr = delta * delta
    if kind == 1:
        if e <= dsqr:
            return e, 1.0
        sqrte = np.sqrt(e)
        return 2 * sqrte * delta - dsqr, delta / sqrte
    if kind == 2:
        aux2 = np.sqrt((1.0 / dsqr) * e + 1.0)
        return 2 * dsqr * (aux2 - 1), 1.0 / aux2
    if kind == 3:
        aux = (1.0 / dsqr) * e + 1.0
        return dsqr * np.log(aux), 1.0 / aux
    if kind == 4:
        if e <= dsqr:
            d = 1 - e * (1.0 / dsqr)
            dd = d * d
            return dsqr * (1 - dd * d), 3 * dd
        return dsqr, 0.0
    return e, 1.0


class RobustNpGraph(npo.NpGraph):
    """robust: {"bbox" | "e3d" | "grav" | "odom": (kind, delta)}; absent classes have no kernel."""

    def __init__(self, graph, cams, objs, robust=None):
        super().__init__(graph, cams, objs)
        self.robust = dict(robust or {})

    def rho(self, e, chi):
        k = self.robust.get(e[0])
        return (chi, 1.0) if k is None else robustify(k[0], k[1], chi)

    def chi2(self):
        c = 0.0
        for e in self.edges:
            r = self.residual(e)
            c += self.rho(e, r @ (e[4] * r))[0]
        return c

    def build(self, delta):
        H = np.zeros((self.n, self.n))
        b = np.zeros(self.n)
        for e in self.edges:
            r = self.residual(e)
            W = np.diag(e[4]) * self.rho(e, r @ (e[4] * r))[1]
            js = self.jacobians(e, delta)
            for (i, Ji) in js:
                b[i:i + Ji.shape[1]] -= Ji.T @ W @ r
                for (k, Jk) in js:
                    H[i:i + Ji.shape[1], k:k + Jk.shape[1]] += Ji.T @ W @ Jk
        return H, b


def optimize(graph, cams, objs, robust=None, max_iters=10, max_trials=10, tau=1e-5, delta=1e-9, drop_nan=True):
    """np_oracle.optimize (g2o LM, dense solve of the whole system) on the robustified graph."""
    G = RobustNpGraph(graph, cams, objs, robust)
    if drop_nan:
        G.drop_nan()
    G.finalize()
    trace = []
    lam, ni, nbad = -1.0, 2.0, 0
    cur = 0.0
    it = 0
    ok = True
    while it < max_iters and ok:
        cur = G.chi2()
        ini = cur
        H, b = G.build(delta)
        if it == 0:
            lam, ni, nbad = tau * np.max(np.abs(np.diag(H))), 2.0, 0
        q, rho = 0, 0.0
        while True:
            bak = (list(G.cams), list(G.objs))
            A = H + lam * np.eye(G.n)
            try:
                np.linalg.cholesky(A)
                x = np.linalg.solve(A, b)
                good = True
            except np.linalg.LinAlgError:
                x = np.zeros(G.n)
                good = False
            G.apply(x)
            tmp = G.chi2() if good else np.finfo(float).max
            rho = (cur - tmp) / (x @ (lam * x + b) + 1e-3)
            if rho > 0 and np.isfinite(tmp):
                alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                cur = tmp
            else:
                lam *= ni
                ni *= 2
                G.cams, G.objs = bak
            q += 1
            if not (rho < 0 and q < max_trials):
                break
        trace.append((cur, lam, q))
        it += 1
        if q == max_trials or rho == 0:
            ok = False
        else:
            nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
            if nbad >= 3:
                ok = False
    cams_out = np.array([npo.T_to7(T) for T in G.cams])
    objs_out = np.array([npo.obj_to10(T, s) for (T, s) in G.objs])
    return cams_out, objs_out, dict(iterations=it, trace=trace, chi2_final=cur, lambda_final=lam)


def edge_chi2(graph, cams, objs, edge_class, robust=None):
    """Raw chi2 and rho1 of every edge of one class in CALLER order (what esl_edge_chi2 reports; NaN-dropped boxes: weight 0)."""
    G = RobustNpGraph(graph, cams, objs, robust)
    g = graph
    k = (robust or {}).get(edge_class)
    rho1 = (lambda e: 1.0) if k is None else (lambda e: robustify(k[0], k[1], e)[1])
    out = []
    if edge_class == "bbox":
        for i in range(len(g.bbox_cam)):
            r = npo.res_bbox(G.cams[g.bbox_cam[i]], G.objs[g.bbox_obj[i]][0], G.objs[g.bbox_obj[i]][1], g.K, g.bbox_meas.reshape(-1, 4)[i])
            e = g.bbox_weight[i] * (r @ r)
            out.append((e, 0.0 if np.isnan(e) else rho1(e)))
    elif edge_class == "e3d":
        for i in range(len(g.e3d_cam)):
            r = npo.res_e3d(G.cams[g.e3d_cam[i]], G.objs[g.e3d_obj[i]][0], G.objs[g.e3d_obj[i]][1], g.e3d_meas.reshape(-1, 10)[i])
            e = g.e3d_weight[i] * (r @ r)
            out.append((e, rho1(e)))
    elif edge_class == "grav":
        for o in g.grav_obj:
            r = npo.res_grav(G.objs[o][0], g.grav_normal)
            e = g.grav_weight * float(r @ r) if np.ndim(r) else g.grav_weight * r * r
            out.append((e, rho1(e)))
    else:
        info = np.ones((len(g.odom_i), 6)) if g.odom_info is None else g.odom_info.reshape(-1, 6)
        for i in range(len(g.odom_i)):
            r = npo.res_odom(G.cams[g.odom_i[i]], G.cams[g.odom_j[i]], npo.T_from7(g.odom_meas.reshape(-1, 7)[i]))
            e = r @ (info[i] * r)
            out.append((e, rho1(e)))
    a = np.array(out, dtype=float).reshape(-1, 2)
    return a[:, 0], a[:, 1]
