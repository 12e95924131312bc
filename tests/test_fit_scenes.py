"""The premises of tests/fit_scenes.py on the CPU: every built scene does what its name says in the C checker
(oracle/esl_oracle_fit.c), and -- stage counters and status -- in the independent numpy restatement (oracle/np_fit.py).
What a scene is FOR (which clustering substrate of csrc/esl_fit.hip, which branch of the cluster choice) is asserted here
through the counters that select it: M against 2048, the chosen cluster's size against 1024, the cell extent against 1020,
neighbours per point against the 16-entry strip, the workspace capacity against 8192.  These are the two restatements'
expected values for a device test of the same scenes, which the suite does not have yet.

All fits run with symmetry_lm_iters = 0 (the LM's own noise floor is not what these scenes are about)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_scenes as fs        # noqa: E402


@functools.lru_cache(maxsize=None)
def _checker(name):
    from oracle import pyoracle as po
    s = fs.scene(name)
    kw = dict(symmetry_lm_iters=0); kw.update(s.params)
    return po.fit_frame(s.depth, s.boxes, s.labels, s.Twc, s.intr, s.ground, po.default_fit_params(**kw))


# (status, in-range samples, points M after the plane filter, clusters >= min_cluster_size, chosen cluster size) per box;
# None = not fixed by construction (voxels merge where the pitch is below the leaf): the relations below cover those
X = None
EXPECT = {
    "m2047": [(0, 2047, 2047, 1, 2047)], "m2048": [(0, 2048, 2048, 1, 2048)], "m2049": [(0, 2049, 2049, 1, 2049)],
    "m2048_pair": [(0, 2048, 2048, 1, 2048)], "m2050": [(0, 2050, 2050, 1, 2050)],
    "nc1024": [(0, 1024, 1024, 1, 1024)], "nc1024_dual": [(0, 1024, 1024, 1, 1024)], "nc1025": [(0, 1025, 1025, 1, 1025)],
    "strip_extent": [(0, 1200, 1200, 1, 1200)],
    "m2048_tol50": [(0, 2048, 2048, 1, 2048)],
    "tol75_bridges": [(0, 1268, 1268, 1, 1268)],      # 5 x 256 less 4 x 4 emptied, plus 4 spurs
    "mixed": [(0, 14000, 14000, 1, 14000), (0, 2048, 2048, 1, 2048), (0, 1024, 1024, 1, 1024), (0, 1360, X, 2, X), (4, 0, 0, 0, 0),
              (0, 800, 800, 1, 800)],
    "mixed_small_only": [(0, 2048, 2048, 1, 2048), (0, 1024, 1024, 1, 1024), (0, 1360, X, 2, X), (4, 0, 0, 0, 0), (0, 800, 800, 1, 800)],
    "choice_near_small": [(0, 1650, X, 2, X)], "choice_largest_small": [(0, 1650, X, 2, 1200)],
    "choice_near_global": [(0, X, X, 2, X)], "choice_largest_global": [(0, X, X, 2, 2250)],
    "choice_near_large": [(0, X, X, 2, X)], "choice_largest_large": [(0, X, X, 2, 8000)],
    "choice_lone_small": [(0, 1200, 1200, 1, 1200)], "choice_none_small": [(2, 1890, 1890, 2, 0)],
    "choice_lone_large": [(0, 7000, 7000, 1, 7000)], "choice_none_large": [(2, 13000, 13000, 2, 0)],
    "choice_lone_tight": [(0, 8000, 8000, 1, 8000)],
    "minsize_eq_small": [(0, 2048, 2048, 1, 2048)], "minsize_above_small": [(2, 2048, 2048, 0, 0)],
    "minsize_eq_large": [(0, 14000, 14000, 1, 14000)], "minsize_above_large": [(2, 14000, 14000, 0, 0)],
    "tie_small": [(0, 800, 800, 2, 400)], "tie_small_a": [(0, 400, 400, 1, 400)], "tie_small_b": [(0, 400, 400, 1, 400)],
    "tie_large": [(0, 9000, 9000, 2, 4500)], "tie_large_a": [(0, 4500, 4500, 1, 4500)], "tie_large_b": [(0, 4500, 4500, 1, 4500)],
    "centre_hole": [(1, 1861, 1861, 0, 0)], "centre_one": [(1, 1861, 1861, 0, 0)], "centre_two": [(0, 1861, 1861, 1, 1861)],
    "boxes_overhang": [(0, 1500, 1500, 1, 1500), (0, 884, 884, 1, 884), (0, 1080, 1080, 1, 1080), (0, 1080, 1080, 1, 1080),
                       (0, 1200, 1200, 1, 1200), (0, 1380, 1380, 1, 1380), (1, 1600, 1600, 0, 0), (0, 1598, 1598, 1, 1598)],
    "boxes_degenerate": [(4, 0, 0, 0, 0)] * 7,
    "stride1": [(0, 61 * 89, X, 1, X)], "stride2": [(0, 31 * 45, X, 1, X)], "stride5": [(0, 61 * 45, 61 * 45, 1, 61 * 45)],
    "stride7": [(0, 44 * 32, 44 * 32, 1, 44 * 32)],
    # 2048 samples less 3 at 0.1 m, 2 at 6.0002 m, 1 at 65535 and the centre pixel at 0.1 m; 501 (0.1002 m) and 30000 (6 m) are in range
    "depth_limits": [(0, 2041, X, 1, X)],
    "depth_min_low": [(0, 2048, X, 1, X)],
    "huge_box": [(0, 856, 856, 1, 856)],
}


def test_every_scene_has_its_premise():
    assert set(EXPECT) == set(fs.NAMES)


@pytest.mark.parametrize("name", fs.NAMES)
def test_scene_premise_in_the_checker(po, name):
    e, p, st, dbg = _checker(name)
    want = EXPECT[name]
    assert len(want) == len(st)
    for b, (status, n0, M, ncl, nc) in enumerate(want):
        got = (int(st[b]), int(dbg[b][0]), int(dbg[b][2]), int(dbg[b][3]), int(dbg[b][4]))
        print(name, b, got)
        for g, w in zip(got, (status, n0, M, ncl, nc)):
            assert w is None or g == w, (name, b, got, want[b])
        if status == 0:
            # no eigenvector luck: the three half-axes are apart by a factor of 1.2 at least
            ax = np.sort(e[b][7:10])
            assert ax[0] > 0 and ax[1] >= 1.2 * ax[0] and ax[2] >= 1.2 * ax[1], (name, b, ax)
        else:
            assert not e[b].any()


@pytest.mark.parametrize("name", fs.NAMES)
def test_scene_counters_in_the_numpy_restatement(po, name):
    """status and the six stage counters of oracle/np_fit.py (np.unique voxel grid, cKDTree clusters) equal the checker's"""
    from oracle import np_fit
    s = fs.scene(name)
    e, p, st, dbg = _checker(name)
    for b in range(len(st)):
        r = np_fit.fit_one(s.depth, s.boxes[b], s.labels[b], s.Twc, s.intr, s.ground, symmetry_lm_iters=0, **s.params)
        assert r["status"] == st[b], (name, b)
        np.testing.assert_array_equal(r["counts"], dbg[b][:6], err_msg=f"{name} box {b}")
        if st[b] == 0:
            np.testing.assert_allclose(np.sort(r["ell"][7:9]), np.sort(e[b][7:9]), atol=1e-8)
            assert abs(r["ell"][9] - e[b][9]) < 1e-8


def _points(name, b=0):
    """the scan's float32 camera-frame points of box b (= world points: identity pose), written out once more"""
    s = fs.scene(name)
    st = s.params.get("stride", 3)
    fx, fy, cx, cy, scale = s.intr
    x1, y1, x2, y2 = [int(v) for v in s.boxes[b]]
    h, w = s.depth.shape
    pts = []
    for y in range(y1, y2, st):
        for x in range(x1, x2, st):
            if x < 0 or y < 0 or x >= w or y >= h:
                continue
            z = s.depth[y, x] / scale
            if z > s.params.get("depth_min", 0.1) and z <= 6.0:
                pts.append(((x - cx) * z / fx, (y - cy) * z / fy, z))
    return np.array(pts, dtype=np.float32)


def test_strip_spans_more_than_1020_cells_with_few_points():
    """the extent fallback's premise: M <= 2048 and yet more cluster cells along x than the LDS cell key's 10 bits take"""
    s = fs.scene("strip_extent")
    P = _points("strip_extent").astype(np.float64)
    assert len(P) == 1200 <= 2048
    cells = np.floor(P / s.params["cluster_tolerance"])
    ext = cells.max(axis=0) - cells.min(axis=0)
    assert ext[0] >= 1020 and ext[1] < 1020 and ext[2] < 1020, ext
    gap = np.linalg.norm(np.diff(P, axis=0), axis=1)
    assert gap.max() < s.params["cluster_tolerance"] and s.params["voxel_leaf"] < np.abs(np.diff(P[:, 0])).min()


def test_large_tolerance_overflows_a_sixteen_entry_neighbour_strip():
    """Every pair of neighbours is recorded once, in the strip of one of its two points.  More than 16 M pairs cannot fit M
    strips of 16; at the default tolerance no point has more than 8 neighbours, so no strip of any scene overflows there."""
    P = _points("m2048_tol50").astype(np.float64)
    d2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    assert (d2 <= 0.05 ** 2).sum() // 2 > 16 * len(P)
    assert (d2 <= 0.02 ** 2).sum(axis=1).max() <= 8


def test_bridges_are_single_pairs_recorded_by_an_overflowing_strip():
    """Across each gap of tol75_bridges exactly one pair of points lies within the tolerance.  A pair is recorded by the point
    whose cell comes first in (z, y, x) order (the search visits a point's own cell and the 13 cells after it); that point has
    more than 16 neighbours in later cells alone, so its strip is flushed at least once while it collects them."""
    P = _points("tol75_bridges").astype(np.float64)
    x1, y1 = fs.BOX_2048[0], fs.BOX_2048[1]
    fx, fy, cx, cy, scale = fs.INTR
    col = np.rint((P[:, 0] * fx / P[:, 2] + cx - x1) / 3).astype(int)
    row = np.rint((P[:, 1] * fy / P[:, 2] + cy - y1) / 3).astype(int)
    d2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    nb = d2 <= fs.BRIDGE_TOL ** 2
    cell = np.floor(P / fs.BRIDGE_TOL).astype(np.int64)
    order = (cell[:, 2] * 2 ** 20 + cell[:, 1]) * 2 ** 20 + cell[:, 0]
    for k in range(4):
        left = col <= 14 * k + 7
        cross = np.argwhere(nb & left[:, None] & ~left[None, :])
        assert len(cross) == 1
        a, b = cross[0]
        assert ((col[a], row[a]), (col[b], row[b])) == fs.bridge_sample(k)
        assert order[a] != order[b]
        owner = a if order[a] < order[b] else b
        assert (nb[owner] & (order > order[owner])).sum() > 16
        assert abs(np.sqrt(d2[a, b]) / fs.BRIDGE_TOL - 1) > 0.03      # (the bridging pairs are not near the tolerance themselves)


@pytest.mark.parametrize("size", ["small", "global", "large"])
def test_near_and_largest_cluster_premises(po, size):
    near, largest = _checker(f"choice_near_{size}"), _checker(f"choice_largest_{size}")
    # same image, same two clusters: center_dis alone moves the choice from the small near cluster to the large far one
    np.testing.assert_array_equal(near[3][0][:4], largest[3][0][:4])
    big = int(largest[3][0][4])
    assert int(near[3][0][2]) == int(near[3][0][4]) + big and 100 <= int(near[3][0][4]) < big
    assert (int(near[3][0][2]) <= 2048) == (size == "small")


@pytest.mark.parametrize("size", ["small", "large"])
def test_cluster_choice_premises(po, size):
    # a lone cluster is taken although it is as far from the centre as in the scene where a second cluster makes that fatal
    lone, none = fs.scene(f"choice_lone_{size}"), fs.scene(f"choice_none_{size}")
    assert lone.params == none.params == {} and (lone.boxes == none.boxes).all()
    cp = fs.centre_pixels(lone.boxes[0])
    assert all(lone.depth[y, x] == none.depth[y, x] for x, y in cp)
    z = np.array([lone.depth[y, x] for x, y in cp]) / 5000.0
    assert ((z == 0) | (z == 1.0)).all() and (z == 1.0).sum() >= 2      # the centre lies at 1 m, the patches at 2.5 m
    assert _checker(f"choice_lone_{size}")[2][0] == 0 and _checker(f"choice_none_{size}")[2][0] == 2
    # the tie goes to the patch with the smaller voxel key (z is the key's leading field: the nearer patch, a), not to the
    # patch under the box centre (b)
    t, a, b = _checker(f"tie_{size}"), _checker(f"tie_{size}_a"), _checker(f"tie_{size}_b")
    assert a[3][0][4] == b[3][0][4] == t[3][0][4] and t[3][0][3] == 2
    np.testing.assert_allclose(t[0][0], a[0][0], rtol=0, atol=1e-12)
    assert np.abs(t[0][0][:3] - b[0][0][:3]).max() > 0.05
    s = fs.scene(f"tie_{size}")
    assert all(s.depth[y, x] == 0 or s.depth[y, x] / 5000.0 > 2.0 for x, y in fs.centre_pixels(s.boxes[0]))      # (a ends below 2 m)


def _capacity(s):
    """the frame's workspace capacity as esl_fit_frame sizes it: the largest box's sample grid (+ 2 per side), as a power of two"""
    st, cap = s.params.get("stride", 3), 64
    for b in s.boxes:
        w, h = int(b[2] - b[0]) // st + 2, int(b[3] - b[1]) // st + 2
        if w > 0 and h > 0:
            cap = max(cap, w * h)
    q = 1024
    while q < cap:
        q <<= 1
    return q


def test_large_scenes_exceed_the_capacity_of_the_in_workgroup_clustering():
    """more than 4 x 2048 points of capacity send every box of a frame to the grid-wide clustering kernels"""
    large = {"mixed", "choice_near_large", "choice_largest_large", "choice_lone_large", "choice_none_large", "choice_lone_tight",
             "minsize_eq_large", "minsize_above_large", "tie_large", "huge_box"}
    for name in fs.NAMES:
        assert (_capacity(fs.scene(name)) > 8192) == (name in large), name
    # in between: more than 2048 points in a frame that stays inside the workgroup (clustering in global memory)
    for name in ("m2049", "m2050", "choice_near_global", "choice_largest_global", "stride5", "tie_large_a", "tie_large_b"):
        assert _checker(name)[3][0][2] > 2048 and _capacity(fs.scene(name)) <= 8192


def test_centre_patch_premises():
    for name, n in (("centre_hole", 0), ("centre_one", 1), ("centre_two", 2)):
        s = fs.scene(name)
        assert sum(s.depth[y, x] / 5000.0 > 0.1 for x, y in fs.centre_pixels(s.boxes[0])) == n
    # 0.1 m exactly: outside the scan's range (double: 0.1 <= depth_min), inside the centre patch's (float 0.1f > 0.1);
    # 0.08 m: inside the scan's range once depth_min = 0.05, outside the centre patch's hard-coded 0.1
    for name, v in (("depth_limits", 500), ("depth_min_low", 400)):
        s = fs.scene(name)
        cp = fs.centre_pixels(s.boxes[0])
        assert sum(s.depth[y, x] == v for x, y in cp) == 1
    assert float(np.float32(500 / 5000.0)) > 0.1 >= 500 / 5000.0
