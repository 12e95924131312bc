"""Numpy reference of fixed ellipsoid vertices (esl_graph_upload_fixed): oracle/np_oracle.py's graph, with the robust kernels of
tests/robust_ref.py, under g2o's setFixed semantics (sparse_optimizer.cpp:234, :454; base_binary_edge.hpp):
  * an edge all of whose vertices are fixed is inactive: a bbox / 3-D edge between a fixed ellipsoid and a fixed camera and every
    gravity prior on a fixed ellipsoid take part in nothing;
  * an edge between a fixed ellipsoid and a free camera is linearised with respect to the camera alone;
  * only free cameras and free ellipsoids get Hessian indices, and only they move.
Test infrastructure."""
import copy

import numpy as np

from oracle import np_oracle as npo
from tests import robust_ref as rr


class FixedNpGraph(rr.RobustNpGraph):
    def __init__(self, graph, cams, objs, obj_fixed=None, robust=None):
        super().__init__(graph, cams, objs, robust)
        self.fixed_obj = np.zeros(self.N, bool) if obj_fixed is None else (np.asarray(obj_fixed).reshape(-1) != 0)
        assert len(self.fixed_obj) == self.N
        self.inactive_edges = []

    def all_fixed(self, e):
        if e[0] == "odom":
            return bool(self.fixed_cam[e[1]] and self.fixed_cam[e[2]])
        return bool(self.fixed_obj[e[2]] and (e[1] < 0 or self.fixed_cam[e[1]]))

    def finalize(self):
        self.inactive_edges = [e for e in self.edges if self.all_fixed(e)]
        self.edges = [e for e in self.edges if not self.all_fixed(e)]
        used_c, used_o = set(), set()
        for e in self.edges:
            if e[0] == "odom":
                used_c.update([e[1], e[2]])
            else:
                used_o.add(e[2])
                if e[1] >= 0:
                    used_c.add(e[1])
        self.idx_c, self.idx_o, n = {}, {}, 0
        for c in range(self.F):
            if c in used_c and not self.fixed_cam[c]:
                self.idx_c[c] = n
                n += 6
        for o in range(self.N):
            if o in used_o and not self.fixed_obj[o]:
                self.idx_o[o] = n
                n += 9
        self.n = n

    def _num(self, e, kind, vid, dim, delta):
        J = np.zeros((len(e[4]), dim))
        for d in range(dim):
            rs = []
            for sgn in (1, -1):
                u = np.zeros(dim)
                u[d] = sgn * delta
                if kind == "cam":
                    cams = list(self.cams)
                    cams[vid] = npo.cam_oplus(self.cams[vid], u)
                    rs.append(self.residual(e, cams=cams))
                else:
                    objs = list(self.objs)
                    objs[vid] = npo.obj_oplus(*self.objs[vid], u)
                    rs.append(self.residual(e, objs=objs))
            J[:, d] = (rs[0] - rs[1]) / (2 * delta)
        return J

    def jacobians(self, e, delta):
        """as NpGraph.jacobians, but a fixed ellipsoid contributes no block (an anchored edge: the camera block alone)"""
        out = []
        if e[0] == "odom":
            for v in (e[1], e[2]):
                if v in self.idx_c:
                    out.append((self.idx_c[v], self._num(e, "cam", v, 6, delta)))
            return out
        if e[1] >= 0 and e[1] in self.idx_c:
            out.append((self.idx_c[e[1]], self._num(e, "cam", e[1], 6, delta)))
        if e[2] in self.idx_o:
            out.append((self.idx_o[e[2]], self._num(e, "obj", e[2], 9, delta)))
        return out
    # apply: NpGraph.apply walks idx_c / idx_o only, so fixed ellipsoids never move


def optimize(graph, cams, objs, obj_fixed=None, robust=None, **kw):
    """robust_ref.optimize's LM loop (np_oracle.optimize's, with the kernels) on the FixedNpGraph: the loop builds its graph through
    the module attribute, which is pointed at this class for the duration of the call."""
    orig = rr.RobustNpGraph
    rr.RobustNpGraph = lambda g, c, o, r=None: FixedNpGraph(g, c, o, obj_fixed, r)
    try:
        return rr.optimize(graph, cams, objs, robust=robust, **kw)
    finally:
        rr.RobustNpGraph = orig


def edge_chi2(graph, cams, objs, edge_class, obj_fixed=None, robust=None):
    """what esl_edge_chi2 reports on a flagged graph, caller order: robust_ref.edge_chi2, inactive edges with weight 0"""
    chi, w = rr.edge_chi2(graph, cams, objs, edge_class, robust)
    if obj_fixed is None or edge_class == "odom":
        return chi, w
    fo = np.asarray(obj_fixed).reshape(-1) != 0
    fc = np.ones(graph.n_cams, bool) if graph.cam_fixed is None else graph.cam_fixed.astype(bool)
    w = w.copy()
    if edge_class == "bbox":
        w[fo[graph.bbox_obj] & fc[graph.bbox_cam]] = 0.0
    elif edge_class == "e3d":
        w[fo[graph.e3d_obj] & fc[graph.e3d_cam]] = 0.0
    else:
        w[fo[np.asarray(graph.grav_obj, dtype=int)]] = 0.0
    return chi, w


def without_edges_of(graph, obj_fixed):
    """the graph with every edge of the flagged ellipsoids deleted (what a mapping-mode run with those ellipsoids fixed sees)"""
    fo = np.asarray(obj_fixed).reshape(-1) != 0
    g = copy.copy(graph)
    kb, ke = ~fo[graph.bbox_obj], ~fo[graph.e3d_obj]
    g.bbox_cam, g.bbox_obj, g.bbox_weight = graph.bbox_cam[kb], graph.bbox_obj[kb], graph.bbox_weight[kb]
    g.bbox_meas = np.ascontiguousarray(graph.bbox_meas.reshape(-1, 4)[kb])
    g.e3d_cam, g.e3d_obj, g.e3d_weight = graph.e3d_cam[ke], graph.e3d_obj[ke], graph.e3d_weight[ke]
    g.e3d_meas = np.ascontiguousarray(graph.e3d_meas.reshape(-1, 10)[ke])
    go = np.asarray(graph.grav_obj, dtype=graph.bbox_obj.dtype)
    g.grav_obj = go[~fo[go]] if len(go) else go
    return g
