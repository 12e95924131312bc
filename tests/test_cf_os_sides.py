"""The one-sided assembly's pair list with twins merged and the shorter side walked (csrc/esl_cf_plan.hpp cf_os_sides; esl_cf.hpp
k_cf_os_list), on the CPU: tests/cf_os_sides_main.cpp compiles the plan header alone, plain and with the address and undefined-behaviour
sanitizers, runs as a child process and is held against numpy written from the definitions -- run heads per (segment, ellipsoid), then
sum over the segments of the lower triangle of min.outer(heads, heads), plus the b row's heads.  All counts are integers and compare
exactly; the flops are sums of integers far below 2^53.  No GPU, nothing loaded into Python.

The premises tests/test_gpu_cf_os_sides.py rests on are asserted here from the graphs alone: blocks that walk the column side, that
tie, that mix both sides over their segments; runs of two entries and an ellipsoid without one; and block lengths, of the merged list
and of the parent's (ESL_CF_OS_LIST=0), that still cover the paths of k_cf_T_onesided_lds named in tests/test_cf_onesided_pairs.py."""
import functools
import importlib
import importlib.util
import os

import numpy as np
import pytest

from tests import cf_os_sides_ref as sides
from tests import cf_plan_ref as ref

SHAPES = {"257": (257, 40, 6), "300": (300, 80, 10), "500": (500, 50, 10), "1100": (1100, 60, 6), "large": (301, 920, 40)}


@functools.lru_cache(maxsize=None)
def _counts_mod():
    spec = importlib.util.spec_from_file_location("cf_onesided_counts", os.path.join(ref.ROOT, "scripts", "cf_onesided_counts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _graph(name):
    synth = importlib.import_module("object-oriented-slam_amd.synth")
    n_cams, n_objs, per_cam = SHAPES[name]
    return synth.make_graph(n_cams, n_objs, per_cam * n_cams, seed=41, slam=True)[0]


@functools.lru_cache(maxsize=None)
def _defs(name, S):
    L = ref.lists(_graph(name))
    d = sides.definitions(L, S)
    return L, d, sides.block_matrices(d["heads"][:, d["unrank"]])


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("cf_os_sides")
    exe = sides.build(d, sanitize=request.param == "sanitized")
    assert exe is not None, "no host compiler (hipcc): the plan's host program cannot be built"
    return exe, d


@pytest.mark.parametrize("S", [16, 32, 48])
@pytest.mark.parametrize("name", list(SHAPES))
def test_plan_counts_equal_the_definitions(program, name, S):
    exe, d = program
    L, df, (both, row, _, _, _) = _defs(name, S)
    N = L["N"]
    pl = sides.run(exe, L, d, sparse=3, stride=S)
    assert pl["sparse"] == 1 and pl["form"] == 3 and pl["S"] == S and pl["os_offsets"] == 1 and pl["os_list"] == 1
    assert np.array_equal(pl["os_run"], df["run"])
    assert np.array_equal(pl["os_heads"], df["heads"][pl["inc_p"], pl["inc_o"]])
    assert int(df["heads"].sum()) == pl["os_heads"].sum() == np.count_nonzero(pl["os_run"])
    tril = np.tril_indices(N)
    brow = int(df["heads"].sum())
    assert pl["osm_npairs"] == int(both[tril].sum()) + brow
    assert pl["osm_row_npairs"] == int(row[tril].sum()) + brow
    assert pl["osm_flops"] == 2.0 * 6.0 * (81.0 * float(both[tril].sum()) + 9.0 * brow)
    assert pl["os_list_npairs"] == pl["osm_npairs"] <= pl["osm_row_npairs"] <= pl["os_npairs"]
    # the fields of the parent's list keep their definitions (tests/test_cf_plan.py), and the switch chooses the length that is built
    ent = df["ent"][:, df["unrank"]]
    old = int((ent.T @ (ent > 0))[tril].sum()) + int(ent.sum())
    assert pl["os_npairs"] == old and pl["os_flops"] == 2.0 * 6.0 * (81.0 * (old - int(ent.sum())) + 9.0 * int(ent.sum()))
    off = sides.run(exe, L, d, os_list=0, sparse=3, stride=S)
    assert off["os_list"] == 0 and off["os_list_npairs"] == off["os_npairs"] == old
    for k in ("osm_npairs", "osm_row_npairs", "osm_flops", "os_flops"):
        assert off[k] == pl[k], k
    assert np.array_equal(off["os_run"], pl["os_run"]) and np.array_equal(off["os_heads"], pl["os_heads"])
    # the script states the same counts
    g = _graph(name)
    s_both, s_row, _, _, s_brow = _counts_mod().block_sides(g, S)
    assert np.array_equal(s_both, both[tril]) and np.array_equal(s_row, row[tril]) and np.array_equal(s_brow, df["heads"][:, df["unrank"]].sum(0))
    assert _counts_mod().side_totals(g, S) == (pl["os_npairs"], pl["osm_row_npairs"], pl["osm_npairs"])


def test_forms_without_the_assembly_have_no_list(program):
    exe, d = program
    L = ref.lists(_graph("257"))
    for sparse in (-1, 0, 1, 2):
        pl = sides.run(exe, L, d, sparse=sparse)
        assert not (pl["sparse"] == 1 and pl["form"] == 3) and pl["os_list"] == 0     # (X dense: the form is not looked at)
        assert pl["osm_npairs"] == pl["osm_row_npairs"] == pl["os_list_npairs"] == 0 and pl["osm_flops"] == 0
        assert pl["os_run"].size == 0 and pl["os_heads"].size == 0


def _paths(p, b):
    """the paths of k_cf_T_onesided_lds by block length (tests/test_cf_onesided_pairs.py): a single pair, exactly one and two batches, one
    piece of the list, a second piece, a last K-step that is half padding, a full batch and a short one, a short batch in a later
    piece; the b row: more than one piece, odd lengths"""
    return np.array([(p == 1).any(), (p == 8).any(), (p == 16).any(), (p == 64).any(), (p > 64).any(), (p % 2 == 1).any(),
                     ((p > 8) & (p < 16)).any(), ((p % 8 != 0) & (p > 64)).any(), b.max() > 64, (b % 2 == 1).any()])


def test_premises_of_the_gpu_test():
    twinless = 0
    for name in SHAPES:
        for S in (16, 32, 48):
            L, df, (both, row, swapped, ties, rowside) = _defs(name, S)
            off = ~np.eye(L["N"], dtype=bool) & np.tri(L["N"], dtype=bool)
            tril = np.tril_indices(L["N"])
            print(name, S, "blocks that walk the column side", int((swapped[off] > 0).sum()), "with a tie", int((ties[off] > 0).sum()),
                  "mixed", int(((swapped > 0) & (rowside > 0))[off].sum()), "runs of two", int((df["run"] == 2).sum()),
                  "pairs", int(both[tril].sum()), "of", int(row[tril].sum()))
            assert (swapped[off] > 0).any() and (ties[off] > 0).any() and ((swapped > 0) & (rowside > 0))[off].any()
            assert ((swapped > 0) & (ties > 0))[off].any()                       # a tie and a swapped segment in one block
            assert (both[off] < row[off]).any() and (df["run"] == 2).any() and df["run"].max() == 2
            assert (np.diag(swapped) == 0).all() and (np.diag(both) == df["heads"][:, df["unrank"]].sum(0)).all()
            seen = df["ent"].sum(0) > 0
            twinless += int((seen & (df["ent"] == df["heads"]).all(0)).sum())
    assert twinless > 0     # an ellipsoid whose cameras each have one edge to it: every run of it has one entry (the large graph has them)
    # the lengths at stride 16, what ESL_CF_SPARSE=3 runs on these sizes: the merged list and the parent's, over the graphs of the GPU test
    new, old = np.zeros(10, bool), np.zeros(10, bool)
    for name in ("300", "500"):
        L, df, (both, _, _, _, _) = _defs(name, 16)
        tril = np.tril_indices(L["N"])
        ent = df["ent"][:, df["unrank"]]
        new |= _paths(both[tril], df["heads"].sum(0)); old |= _paths((ent.T @ (ent > 0))[tril], ent.sum(0))
    assert new.all() and old.all(), (new, old)
    L, df, (both, _, _, _, _) = _defs("500", 16)
    assert (both > 128).any()     # three pieces of the list
