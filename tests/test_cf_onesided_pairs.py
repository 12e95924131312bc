"""The block lengths that tests/test_gpu_cf_onesided_gather.py rests on, counted on the CPU from the graph alone (no GPU, no library):
pairs per block of T = entries of o1 at interior slots of the segments where o2 is live (scripts/cf_onesided_counts.py block_pairs).
k_cf_T_onesided_lds takes its pairs in batches of 8 and its list in pieces of 64; a block of odd length ends in a K-step that is
half padding.  Which ellipsoid of a block is o1 follows T's order, so only the counts that do not depend on it are held exactly.
"""
import functools
import importlib
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _lengths(n_cams, n_objs, per_cam):
    spec = importlib.util.spec_from_file_location("cf_onesided_counts", os.path.join(ROOT, "scripts", "cf_onesided_counts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    synth = importlib.import_module("object-oriented-slam_amd.synth")
    g = synth.make_graph(n_cams, n_objs, per_cam * n_cams, seed=41, slam=True)[0]
    return mod.block_pairs(g)


@pytest.mark.parametrize("shape,blocks,empty,b_row,lengths", [
    ((300, 80, 10), 3240, 104, 92, (1, 8, 16, 64)),
    ((500, 50, 10), 1275, 23, 219, (1, 64)),
])
def test_block_lengths_cover_the_kernel_paths(shape, blocks, empty, b_row, lengths):
    pairs, rhs = _lengths(*shape)
    print(shape, "blocks", pairs.size, "empty", int((pairs == 0).sum()), {n: int((pairs == n).sum()) for n in (1, 8, 16, 64)},
          "> 64:", int((pairs > 64).sum()), "> 128:", int((pairs > 128).sum()), "odd:", int((pairs % 2 == 1).sum()), "longest b row", int(rhs.max()))
    assert pairs.size == blocks and int((pairs == 0).sum()) == empty and int(rhs.max()) == b_row
    for n in lengths:   # a single pair, exactly one and two batches, exactly one piece of the list
        assert (pairs == n).any(), n
    assert (pairs > 64).any() and (pairs % 2 == 1).any()          # a second piece of the list; a last K-step that is half padding
    assert ((pairs > 8) & (pairs < 16)).any()                     # a full batch and a short one behind it
    assert ((pairs % 8 != 0) & (pairs > 64)).any()                # a short batch in a later piece of the list
    assert rhs.max() > 64 and (rhs % 2 == 1).any()                # the b row: more than one piece, odd lengths
    if shape == (500, 50, 10):
        assert (pairs > 128).any()                                # three pieces of the list
