"""The numpy statement of esl_dense_render (tests/dense_render_ref.py) on its own: analytic known answers, the premises every device
scene of tests/test_gpu_dense_render.py relies on, and csrc/esl_dense_proj.hpp held to the statement on the host (plain and under
AddressSanitizer + UBSan, as a stand-alone program: nothing is preloaded into Python)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as dr                 # noqa: E402
import dense_render_ref as drr         # noqa: E402
import dense_render_scenes as rs       # noqa: E402
import dense_scenes as sc              # noqa: E402
from dense_prog import BUILDS, BUILD_IDS, NONFINITE, build_prog, check_ladder          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(name, **kw):
    c = rs.case(name)
    return drr.render(rs.extract(c["map"]), rs.leaf_of(c["map"]), c["cams"], c["K"], c["rows"], c["cols"], c["depth_meas"], **dict(c["params"], **kw))


def pixels(r, f, i):
    """(rows, cols) of the pixels voxel i wins in frame f, as sorted unique lists"""
    rr_, cc = np.nonzero(r["voxel"][f] == i)
    return sorted(set(rr_.tolist())), sorted(set(cc.tolist()))


def test_probe_map_order():
    e = rs.extract("probe")
    assert e["n_voxels"] == len(rs.PROBE_KEYS) and e["key"].tolist() == [list(k) for k in rs.PROBE_KEYS]
    assert e["xyz"].tolist() == [[(k + 0.5) / 64 for k in key] for key in rs.PROBE_KEYS]          # dyadic: exact


# ---- analytic known answers ---------------------------------------------------------------------------------------------------------------
def test_axis_voxel_and_half_footprint_at_twice_the_distance():
    r = run("axis")
    # frame 0: voxel 4 at p_c = (0, 0, 1): u = 32, u0 = 30, u1 = 34: pixels 30 .. 34 x 22 .. 26, z = 1
    assert pixels(r, 0, 4) == (list(range(22, 27)), list(range(30, 35)))
    assert (r["voxel"][0] == 4).sum() == 25 and r["depth"][0, 24, 32] == 1.0 and (r["depth"][0][r["voxel"][0] == 4] == 1.0).all()
    assert (r["voxel"][0] == 5).sum() == 0          # two voxels on one ray: the nearer wins every pixel of the farther's 3 x 3
    # frame 1: the same voxel at z = 2: u0 = 31, u1 = 33: half the width
    assert pixels(r, 1, 4) == ([23, 24, 25], [31, 32, 33]) and r["depth"][1, 24, 32] == 2.0
    a0, a1 = r["area"]
    # the unclipped footprints themselves: voxels 4 and 7 at 1 m, voxel 5 at 2 m (drawn, and hidden); voxels 4 and 7 at 2 m
    assert a0.count(25) == 2 and a0.count(9) == 1 and 9 in a1 and 25 not in a1
    assert r["frame"][0].tolist()[:3] == [7, 1, 1] and r["frame"][1].tolist()[:3] == [8, 1, 0]
    # clipped by each image edge (frame 0): left, top, bottom, right
    assert pixels(r, 0, 1) == (list(range(22, 27)), [0, 1, 2]) and pixels(r, 0, 2) == ([0, 1, 2], list(range(30, 35)))
    assert pixels(r, 0, 6) == ([46, 47], list(range(30, 35))) and pixels(r, 0, 8) == (list(range(22, 27)), [62, 63])
    assert (r["voxel"][0] == 0).sum() == 0 and (r["voxel"][0] == 3).sum() == 0          # outside; behind the camera
    assert r["frame"][:, 3].tolist() == [int((r["voxel"][f] >= 0).sum()) for f in range(2)] and (r["frame"][:, 4:] == 0).all()
    assert r["vox"][:, 0].sum() == r["frame"][:, 3].sum() and (r["vox"][:, 1:] == 0).all()
    assert r["result"] == dict(status=0, n_voxels=9, n_small=0, n_chunks=1)


def test_half_pixel_goes_to_the_upper_pixel():
    r = run("half_pixel", footprint=0.0)
    # u = 31.5, v = 23.5 exactly: floor(u + 0.5) = 32, 24
    assert pixels(r, 0, 4) == ([24], [32])
    r = run("half_pixel")          # u0 = 29.5, u1 = 33.5: ceil 30, floor 33, and col 32 inside
    assert pixels(r, 0, 4) == ([22, 23, 24, 25], [30, 31, 32, 33])


def test_footprint_and_radius():
    assert pixels(run("footprint0"), 0, 7) == ([36], [44])
    assert pixels(run("radius0"), 0, 7) == ([36], [44])                                   # clamped by max_radius
    assert pixels(run("radius1"), 0, 7) == ([35, 36, 37], [43, 44, 45])                  # clamped by max_radius
    assert pixels(run("radius8"), 0, 7) == (list(range(34, 39)), list(range(42, 47)))
    assert pixels(run("footprint15"), 0, 7) == (list(range(33, 40)), list(range(41, 48)))          # e = 3 pixels


def test_culls():
    r = run("depth_max")          # voxel 5 at z = 2 > 1.5, voxel 3 behind
    assert r["frame"][0].tolist()[:3] == [6, 2, 1]
    r = run("depth_min_exact")          # z == depth_min is drawn
    assert r["frame"][0].tolist()[:3] == [7, 1, 1] and r["voxel"][0, 24, 32] == 4 and r["depth"][0, 24, 32] == 1.0
    r = run("nonfinite")          # voxel 4 at z = 0 with depth_min = 0: 0 / 0 is no coordinate
    assert r["frame"][0, 2] >= 1 and (r["voxel"] != 4).all()
    c = rs.case("nonfinite")
    pr = drr.project(rs.extract("probe")["xyz"], c["cams"][0], c["K"], c["rows"], c["cols"], rs.LEAF / 2, dict(drr.DEFAULTS, depth_min=0.0))
    assert pr["z"][4] == 0.0 and pr["depth_in"][4] and not pr["drawn"][4] and np.isnan(pr["coords"][0][4])


def test_zq_tie_goes_to_the_lower_index():
    r = run("tie")
    e = rs.extract("tie")
    assert e["xyz"][0, 2] == 63.5 / 64 + 2.0 ** -25 and e["xyz"][1, 2] == 63.5 / 64
    # footprint 1.5: voxel 0 covers columns 30 .. 34 (u0 = 29.0000001, u1 = 34.9999999) x rows 22 .. 26, voxel 1 columns 33 .. 39 x rows
    # 21 .. 27: columns 33 and 34 are contested, zq ties, voxel 0 wins although it is farther; the depth is its own
    assert (r["voxel"][0, 22:27, 30:35] == 0).all() and (r["depth"][0, 22:27, 30:35] == 1.0 + 2.0 ** -25).all()
    assert (r["voxel"][0, 22:27, 35] == 1).all() and (r["depth"][0, 22:27, 35] == 1.0).all() and (r["voxel"][0, 21, 33:40] == 1).all()
    assert r["vox"][:, 0].tolist() == [25, 39]


def test_exact_tolerance_boundary_and_every_class():
    r = run("tol")
    # frames: |z_meas - z| == depth_tol above (agree), one raw unit more (farther), == depth_tol below (agree), one more (nearer), no data
    assert r["frame"][:, 3].tolist() == [25] * 5
    assert r["frame"][:, 4:].tolist() == [[25, 0, 0, 0], [0, 0, 25, 0], [25, 0, 0, 0], [0, 25, 0, 0], [0, 0, 0, 25]]
    assert r["vox"].tolist() == [[125, 50, 25, 25]] and r["margins"]["tol"] == 0.0


def test_min_count():
    r = run("min_count2")
    assert r["result"]["n_small"] == 2 and r["frame"][0].tolist()[:3] == [2, 0, 0]
    assert sorted(set(r["voxel"][0].reshape(-1).tolist())) == [-1, 1, 2]
    assert run("min_count2", min_count=1)["result"]["n_small"] == 0


def test_invalid_map_and_pose():
    c = rs.case("axis")
    assert rs.scene("full")["map"].status == 3
    assert drr.render(rs.extract("full"), rs.LEAF, c["cams"], c["K"], c["rows"], c["cols"]) == dict(result=dict(status=3, n_voxels=-1, n_small=0, n_chunks=0))
    with pytest.raises(dr.InvalidPose):
        drr.render(rs.extract("probe"), rs.LEAF, [[0, 0, 0, 0, 0, 0, 0]], c["K"], c["rows"], c["cols"])


# ---- the premises of the device scenes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rs.GENERAL)
def test_general_scenes_keep_their_margins(name):
    r = run(name)
    mg = r["margins"]
    print(name, mg, r["result"], r["frame"].tolist())
    assert mg["round"] >= sc.MIN_KEY and mg["ceil"] >= sc.MIN_KEY and mg["floor"] >= sc.MIN_KEY, mg
    assert mg["zq"] >= sc.MIN_FIX, mg
    if name != "overdraw":
        assert mg["tol"] >= sc.MIN_KEY, mg


def test_room_premises():
    r = run("room")
    F, rows, cols = r["voxel"].shape
    assert (F, rows, cols) == (3, 48, 64) and 1000 < r["result"]["n_voxels"] < 8000
    assert ((r["voxel"] >= 0).sum(axis=(1, 2)) > rows * cols // 2).all()          # a winner on more than half of the pixels of every frame
    assert (r["frame"][:, 4:].sum(axis=1) == r["frame"][:, 3]).all() and (r["frame"][:, 4] > r["frame"][:, 3] // 2).all()
    assert r["vox"].sum(axis=0).tolist() == r["frame"][:, [3, 4, 5, 6]].sum(axis=0).tolist()
    assert len(set(r["inst"].reshape(-1).tolist())) > 3 and r["bgr"].max() > 0
    s = run("room_shift")
    assert (s["frame"][1, 4:] > 0).all(), s["frame"].tolist()          # every class in the shifted frame
    assert s["frame"][[0, 2]].tolist() == r["frame"][[0, 2]].tolist() and s["voxel"].tobytes() == r["voxel"].tobytes()
    # one frame per chunk: the same result but n_chunks
    one = run("room_shift", zbuf_bytes=8 * rows * cols)
    assert one["result"] == dict(s["result"], n_chunks=3)
    for k in ("depth", "voxel", "bgr", "inst", "frame", "vox"):
        assert one[k].tobytes() == s[k].tobytes()
    # the map after a removal: fewer voxels, another list
    d = run("removed")
    assert 0 < d["result"]["n_voxels"] < r["result"]["n_voxels"]


def test_overdraw_premises():
    r = run("overdraw")
    assert r["result"]["n_voxels"] == 3200 and r["frame"][:, 0].tolist() == [3200, 3200]
    assert (r["frame"][:, 3] <= 40).all() and (r["frame"][:, 3] >= 4).all(), r["frame"].tolist()          # a handful of pixels
    e = rs.extract("overdraw")
    won = np.flatnonzero(r["vox"][:, 0])
    assert (e["key"][won][:, 2] == 63).all()          # the nearer layer; within it zq ties and the lowest index of a pixel wins


def test_grids():
    for n in rs.LIST_LENGTHS:
        r = run(f"grid{n}")
        assert r["result"]["n_voxels"] == n and r["frame"][:, :3].sum(axis=1).tolist() == [n, n]
    assert run("grid257")["frame"][0, 2] > 0 and run("grid0")["frame"].tolist() == [[0] * 8] * 2
    assert len(run("grid65", vox_cap=10)["vox"]) == 10


# ---- the header against the statement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan_ubsan"])
def test_proj_header_matches_the_statement(tmp_path, flags):
    exe = build_prog(tmp_path, "dense_render_main", flags)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "dense_proj ok"
    n_drawn = n_other = 0
    for name in ("axis", "half_pixel", "radius1", "footprint15", "depth_max", "nonfinite", "tie", "room", "overdraw", "grid257"):
        c = rs.case(name)
        p = dict(drr.DEFAULTS, **c["params"])
        ext, leaf = rs.extract(c["map"]), rs.leaf_of(c["map"])
        e = p["footprint"] * leaf / 2
        for cam in c["cams"]:
            pr = drr.project(ext["xyz"], cam, c["K"], c["rows"], c["cols"], e, p)
            head = (f"{e!r} {p['max_radius']} {c['rows']} {c['cols']} {p['depth_min']!r} {p['depth_max']!r} "
                    + " ".join(repr(float(v)) for v in c["K"]) + f" {len(ext['xyz'])}\n" + " ".join(repr(float(v)) for v in cam) + "\n")
            body = "\n".join(" ".join(repr(float(v)) for v in row) for row in ext["xyz"])
            out = subprocess.run([exe, "project"], input=head + body + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
            assert len(out) == len(ext["xyz"]) + 1
            zbits = pr["z"].view(np.uint64)
            with np.errstate(all="ignore"):
                zq = np.rint(pr["z"] * drr.ZFIX)
            for i, got in enumerate(out[:-1]):
                if pr["drawn"][i]:
                    want = f"0 {int(zbits[i])} {int(zq[i])} " + " ".join(str(int(b)) for b in pr["box"][i]); n_drawn += 1
                else:
                    want = f"{2 if pr['depth_in'][i] else 1} {int(zbits[i])} 0 0 0 0 0"; n_other += 1
                assert got == want, (name, i)
    assert n_drawn > 5000 and n_other > 10


# ---- what esl_dense_render refuses for its parameters (csrc/esl_dense_check.hpp), text by text and in order -------------------------------
TINY = 5e-324          # the smallest positive double: the first value above 0, its negative the first below
# the depth gate of esl_dense_render and esl_dense_carve_frames: the six refusals in their order, the texts as the entries have always given them
GATE_RUNGS = [
    ("depth_scale not finite or <= 0", [dict(depth_scale=TINY)], [dict(depth_scale=0.0), dict(depth_scale=-1.0)] + [dict(depth_scale=v) for v in NONFINITE]),
    ("depth_min not finite or negative", [dict(depth_min=0.0)], [dict(depth_min=-TINY)] + [dict(depth_min=v) for v in NONFINITE]),
    ("depth_max not finite or negative", [dict(depth_min=0.0, depth_max=0.0)], [dict(depth_max=-TINY)] + [dict(depth_max=v) for v in NONFINITE]),
    ("depth_tol not finite or negative", [dict(depth_tol=0.0)], [dict(depth_tol=-TINY)] + [dict(depth_tol=v) for v in NONFINITE]),
    ("depth_min > depth_max", [dict(depth_min=6.0)], [dict(depth_min=5000.0, depth_max=4999.0), dict(depth_min=float(np.nextafter(6.0, np.inf)))]),
    ("depth_max > 4095", [dict(depth_max=4095.0)], [dict(depth_max=float(np.nextafter(4095.0, np.inf)))]),
]


@pytest.mark.parametrize("flags", BUILDS, ids=BUILD_IDS)
def test_render_params_check_texts_and_order(tmp_path, flags):
    """drn_params_check: every rung at its last accepted and first refused value, NaN and the infinities in every double, and the
    earlier rung's text when two fail.  npix = rows cols: 16 for a 4 x 4 image, 2^28 for the largest."""
    exe = build_prog(tmp_path, "dense_render_main", flags)
    defaults = dict(drr.DEFAULTS, npix=16)
    assert defaults["zbuf_bytes"] == 268435456 and defaults["depth_max"] == 6.0 and defaults["max_radius"] == 8
    rungs = GATE_RUNGS + [
        ("footprint not finite or negative", [dict(footprint=0.0)], [dict(footprint=-TINY)] + [dict(footprint=v) for v in NONFINITE]),
        ("max_radius outside 0 .. 64", [dict(max_radius=0), dict(max_radius=64)], [dict(max_radius=-1), dict(max_radius=65)]),
        ("min_count < 1", [dict(min_count=1)], [dict(min_count=0)]),
        ("zbuf_bytes < 8 rows cols", [dict(zbuf_bytes=128), dict(npix=1 << 28, zbuf_bytes=1 << 31)],
         [dict(zbuf_bytes=127), dict(npix=1 << 28, zbuf_bytes=(1 << 31) - 1), dict(zbuf_bytes=-1)]),
    ]
    fields = ["depth_scale", "depth_min", "depth_max", "depth_tol", "footprint", "max_radius", "min_count", "zbuf_bytes", "npix"]
    check_ladder(exe, fields, defaults, rungs)
