"""esl_dense_carve_frames at the ABI: the symbols load on a CPU-only box, the structs have the sizes include/esl.h states and
esl_dense_carve_params_default fills what abi.py's defaults hold."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("esl_dense_carve_params_default", "esl_dense_carve_frames")
FIELDS = ("depth_scale", "depth_min", "depth_max", "depth_tol", "window", "min_through", "through_per_agree", "apply")


def test_symbols_load(pkg):
    L = pkg.lib.load()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in pkg.lib.EXPORTS, name
    assert L.esl_abi_version() == 5          # additive: detected by the symbol


def test_struct_sizes_match_the_header(pkg):
    txt = open(os.path.join(ROOT, "include", "esl.h")).read()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"\}\s*(esl_dense_carve_\w+);\s*/\*\s*(\d+) bytes", txt)}
    assert sizes == dict(esl_dense_carve_params=48, esl_dense_carve_result=96)
    a = pkg.abi
    assert ctypes.sizeof(a.EslDenseCarveParams) == sizes["esl_dense_carve_params"]
    assert ctypes.sizeof(a.EslDenseCarveResult) == sizes["esl_dense_carve_result"]
    assert a.EslDenseCarveParams.window.offset == 32 and a.EslDenseCarveParams.apply.offset == 44
    assert a.EslDenseCarveResult.samples_found.offset == 16 and a.EslDenseCarveResult.removed.offset == 32
    assert ctypes.sizeof(a.EslDenseRemoveResult) == 64


def test_defaults(pkg):
    L = pkg.lib.load()
    p = pkg.abi.EslDenseCarveParams(-1.0, -1.0, -1.0, -1.0, -1, -1, -1, -1)
    L.esl_dense_carve_params_default(ctypes.byref(p))
    d = pkg.abi.default_dense_carve_params()
    assert tuple(getattr(p, k) for k in FIELDS) == (5000.0, 0.1, 6.0, 0.05, 1, 2, 1, 0) == tuple(getattr(d, k) for k in FIELDS)
    assert pkg.abi.DENSE_CARVE_DEFAULTS == {k: getattr(d, k) for k in FIELDS}
    q = pkg.abi.default_dense_carve_params(window=4, apply=1)
    assert (q.window, q.apply, q.min_through) == (4, 1, 2)
    L.esl_dense_carve_params_default(None)          # a null pointer is ignored
