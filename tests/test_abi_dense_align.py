"""esl_dense_normals / esl_dense_align_frames at the ABI: the symbols load on a CPU-only box, the structs have the sizes include/esl.h
states and the *_default functions fill what abi.py's defaults hold."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("esl_dense_normal_params_default", "esl_dense_normals", "esl_dense_align_params_default", "esl_dense_align_frames")


def test_symbols_load(pkg):
    L = pkg.lib.load()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in pkg.lib.EXPORTS, name
    assert L.esl_abi_version() == 5          # additive: detected by the symbol


def test_struct_sizes_match_the_header(pkg):
    txt = open(os.path.join(ROOT, "include", "esl.h")).read()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"\}\s*(esl_dense_(?:normal|align)_\w+);\s*/\*\s*(\d+) bytes", txt)}
    assert sizes == dict(esl_dense_normal_params=24, esl_dense_normal_result=16, esl_dense_align_params=80, esl_dense_align_frame=384,
                         esl_dense_align_result=16)
    a = pkg.abi
    for name, cls in (("esl_dense_normal_params", a.EslDenseNormalParams), ("esl_dense_normal_result", a.EslDenseNormalResult),
                      ("esl_dense_align_params", a.EslDenseAlignParams), ("esl_dense_align_frame", a.EslDenseAlignFrame),
                      ("esl_dense_align_result", a.EslDenseAlignResult)):
        assert ctypes.sizeof(cls) == sizes[name], name
    assert a.EslDenseAlignFrame.H.offset == 80 and a.EslDenseAlignParams.normals.offset == 56 and a.DENSE_ALIGN_ROW == 37


def test_defaults(pkg):
    L = pkg.lib.load()
    n = pkg.abi.EslDenseNormalParams(max_curvature=-1.0, radius=-1, min_count=-1, min_neighbors=-1, pad=0)
    L.esl_dense_normal_params_default(ctypes.byref(n))
    d = pkg.abi.default_dense_normal_params()
    assert (n.max_curvature, n.radius, n.min_count, n.min_neighbors) == (0.05, 1, 1, 5) == (d.max_curvature, d.radius, d.min_count, d.min_neighbors)
    p = pkg.abi.EslDenseAlignParams()
    L.esl_dense_align_params_default(ctypes.byref(p))
    q = pkg.abi.default_dense_align_params()
    for k in ("max_dist", "damping", "min_pivot_ratio", "tol_t", "tol_r", "iters", "stride", "reach", "min_inliers"):
        assert getattr(p, k) == getattr(q, k), k
    assert (p.max_dist, p.damping, p.min_pivot_ratio, p.tol_t, p.tol_r, p.iters, p.stride, p.reach, p.min_inliers) == (0.0, 0.0, 1e-6, 1e-5, 1e-5, 4, 2, 1, 100)
    assert (p.normals.max_curvature, p.normals.radius, p.normals.min_count, p.normals.min_neighbors) == (0.05, 1, 1, 5)
    r = pkg.abi.default_dense_align_params(reach=2, radius=2, min_neighbors=12)
    assert (r.reach, r.normals.radius, r.normals.min_neighbors) == (2, 2, 12)
