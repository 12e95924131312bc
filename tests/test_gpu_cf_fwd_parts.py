"""The slab sweep k_cf_forward<2> with a chunk's slab in quarters or eighths (ESL_CF_FWD_PARTS=4 | 8 when the context is created) against
the halves it had (=2, esl_cf.hpp): the parts only decide how much LDS a one-wave workgroup holds.  Every part walks the chunk's entry
range and takes its own slots, the entries of a slot are added in list order, so slabs, R and Y -- and with them everything
downstream -- have the same bits: first trial and two runs of the default path compared bit for bit, at segments of one, two and three
chunks, on a short last segment, and on the awkward structures (an ellipsoid seen only inside the second chunk of a stride-32 segment,
which is the third chunk of a stride-48 segment: cameras 81 .. 95).  256 free cameras: every chunk full, the last segment exactly full
at stride 32 and a whole chunk short at 48; 499: a last chunk of three slots -- less than a quarter of a chunk, an eighth and half of one."""
import pytest

from tests.test_gpu_cf_onesided import _graph
from tests.test_gpu_cf_onesided_gather import _assert_same, _everything
from tests.test_gpu_cf_sep_overlap import _awkward_graph
from tests.test_gpu_cf_stride import _awkward_graph32

pytestmark = pytest.mark.gpu


def _context(pkg, monkeypatch, parts, stride):
    monkeypatch.setenv("ESL_CF_FWD_PARTS", str(parts))
    if stride:
        monkeypatch.setenv("ESL_CF_STRIDE", str(stride))
    try:
        return pkg.Context(0)
    finally:
        monkeypatch.delenv("ESL_CF_FWD_PARTS", raising=False)
        monkeypatch.delenv("ESL_CF_STRIDE", raising=False)


@pytest.mark.parametrize("which,stride", [("257", None), ("257", 32), ("257", 48), ("300", None), ("300", 32), ("300", 48), ("500", None), ("1100", None),
                                          ("awkward", None), ("awkward32", 32), ("awkward32", 48)])
def test_quarters_and_eighths_of_a_chunk_give_the_bits_of_halves(pkg, monkeypatch, which, stride):
    g, c, o = {"257": lambda: _graph(257, 40, 6), "500": lambda: _graph(500, 50, 10), "300": lambda: _graph(300, 80, 10), "1100": lambda: _graph(1100, 60, 6), "awkward": lambda: _awkward_graph(pkg),
               "awkward32": lambda: _awkward_graph32(pkg)}[which]()
    monkeypatch.setenv("ESL_CF_SPARSE", "3")
    res = {}
    for parts in (2, 4, 8):
        cx = _context(pkg, monkeypatch, parts, stride)
        try:
            res[parts] = _everything(pkg, cx, g, c, o)
            assert res[parts][2]["stride"] == (stride or 16)
        finally:
            cx.close()
    _assert_same(res[2], res[4])
    _assert_same(res[2], res[8])

