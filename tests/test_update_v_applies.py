"""The size rule that puts a rank-K update on the 128 x 128 tile kernel (esl_chol.hpp, chol_update_v_applies), through the host-only
debug entry.  The camera-first trial depends on it twice: only this kernel can ASSIGN T = -Xs^T Xs, which lets the segments' products
run beside the update, and only its launch takes the occupancy cap that makes them resident there (ESL_CF_OVERLAP=4).  The rule:
at least 1,024 tiles of 256 x 128 in the region (half of them for a whole lower triangle), even leading dimensions and base."""


def _ld(n_o):
    return (n_o + 1 + 127) // 128 * 128   # the leading dimension the library gives T and the separators' rows of X


def _whole(lib, n_o):
    return lib.update_v_applies(_ld(n_o), n_o + 1, 0, n_o, True, _ld(n_o))


def test_first_order_with_the_assign_form(pkg):
    """32 tile rows of 256 x 64 tile columns of 128, halved: 1,024 -- from order 8,065 on, i.e. 897 ellipsoids (order 8,073)."""
    lib = pkg.lib
    first = next(n for n in range(1, 20000) if _whole(lib, n))
    assert first == 8065
    assert all(_whole(lib, n) for n in (8065, 8073, 9001, 18000, 32768))
    assert not any(_whole(lib, n) for n in (1, 126, 450, 4096, 8064))
    assert _whole(lib, 9 * 897) and not _whole(lib, 9 * 896)


def test_regions_and_parity(pkg):
    lib = pkg.lib
    ld = _ld(18000)
    assert lib.update_v_applies(ld, 18001, 0, 2304)            # a column range: 71 x 18 tiles
    assert not lib.update_v_applies(ld, 18001, 0, 1152)        # 71 x 9
    assert lib.update_v_applies(ld, 18001, 9216, 18000)        # a trailing triangle of 8,784 columns
    assert not lib.update_v_applies(ld, 18001, 10368, 18000)   # ... of 7,632
    assert not lib.update_v_applies(ld, 18001, 18000, 18000) and not lib.update_v_applies(ld, 18001, 18001, 18002)   # empty regions
    assert not lib.update_v_applies(ld + 1, 18001, 0, 18000, True, ld)       # 16-byte accesses: odd leading dimension of T,
    assert not lib.update_v_applies(ld, 18001, 0, 18000, True, ld + 1)       # ... of the external operand,
    assert lib.update_v_applies(ld, 18001, 0, 18000, False, ld + 1)          # ... which does not matter when there is none,
    assert not lib.update_v_applies(ld, 18001, 1, 18000)                     # ... odd base


def test_other_tile_kernel(pkg, monkeypatch):
    """ESL_UPD_V=0 puts the big updates on the 256 x 128 tile, which has neither an assign form nor the cap."""
    monkeypatch.setenv("ESL_UPD_V", "0")
    assert not _whole(pkg.lib, 18000)
