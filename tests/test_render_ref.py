"""esl_render_map without a device: the numpy statement (tests/render_ref.py) against known answers, its two formulations of the ray
cast against each other (which measures the device tolerance render_scenes.TOL), the containment of the hit pixels in the bbox edge's
box, csrc/esl_render_ray.hpp in a stand-alone program (plain and under AddressSanitizer / UBSan) against the statement, and the binding."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as rr          # noqa: E402
import render_scenes as sc       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def all_scenes():
    s = {f"room{seed}": sc.room_scene(seed) for seed in sc.ALL_ROOM_SEEDS}
    s.update(crowd=sc.crowd_scene(), occluders=sc.occluder_scene(), across=sc.across_scene(), nothing=sc.nothing_scene())
    return s


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return sc.reference(all_scenes()[name])


# ---- known answers ----------------------------------------------------------------------------------------------------------------------------------
def test_sphere_on_the_axis():
    r, D, f, rows, cols = 0.5, 3.0, 60.0, 41, 61
    K = (f, f, 30.0, 20.0)
    ref = rr.render(sc.IDENTITY_CAM, sc.sphere([0, 0, D], r), K, rows, cols)
    assert ref["depth"][0, 20, 30] == D - r and ref["inst"][0, 20, 30] == 0
    # the cone of the sphere: the ray through (i, j) pixels off the principal point hits iff sin^2 of its angle to the axis < r^2 / D^2,
    # (i^2 + j^2) / (i^2 + j^2 + f^2) < r^2 / D^2, in integers with r / D = 1 / 6 and f = 60: 35 (i^2 + j^2) < 3600
    n = sum(1 for j in range(-20, 21) for i in range(-30, 31) if 35 * (i * i + j * j) < 3600)
    assert n > 300 and list(ref["cover"][0, 0]) == [n, n] and (ref["inst"][0] == 0).sum() == n
    assert ref["flags"][0, 0] == rr.DRAWN | rr.BOUNDED
    assert np.nanmin(ref["depth"]) == D - r and np.nanmax(ref["depth"]) < D


def test_two_spheres_on_one_ray():
    K = (60.0, 60.0, 30.0, 20.0)
    objs = np.stack([sc.sphere([0, 0, 5.0], 1.0), sc.sphere([0, 0, 2.0], 0.25)])
    ref = rr.render(sc.IDENTITY_CAM, objs, K, 41, 61)
    assert ref["depth"][0, 20, 30] == 1.75 and ref["inst"][0, 20, 30] == 1
    small = ref["inst"][0] == 1
    assert ref["cover"][0, 1, 0] == ref["cover"][0, 1, 1] == small.sum() > 0          # the near one is hidden nowhere
    assert ref["cover"][0, 0, 0] - ref["cover"][0, 0, 1] == small.sum()              # and hides exactly its own pixels of the far one
    ring = ref["inst"][0] == 0
    assert ring.any() and (ref["depth"][0][ring] > 4.0).all()


def test_inside_behind_across():
    n = ref_of("nothing")
    assert list(n["flags"][0]) == [rr.INSIDE, rr.INVALID, rr.INVALID, rr.INVALID, 0]
    assert (n["inst"] == -1).all() and np.isnan(n["depth"]).all() and not n["cover"].any()
    a = sc.check_conditions(ref_of("across"))
    assert list(a["flags"][0]) == [rr.DRAWN, rr.DRAWN | rr.BOUNDED]
    assert a["cover"][0, 0, 1] > 50 and 0 < a["cover"][0, 1, 1]
    hit = a["inst"][0] == 0
    assert hit[:, -1].any() or hit[:, 0].any() or hit[0].any() or hit[-1].any()          # it leaves the image: its outline is no ellipse
    assert np.nanmin(a["depth"][0][hit]) < 0.5          # nearer than any plane in front could be cut by a box


def test_union_of_occluders_premise():
    r = sc.check_conditions(ref_of("occluders"))
    n = r["cover"][0, 0, 0]
    assert n > 500 and r["cover"][0, 0, 1] == 0
    assert r["cover"][0, 1, 0] == r["cover"][0, 1, 1]          # the nearer occluder is hidden nowhere
    both = r["cover"][0, 2, 0] - r["cover"][0, 2, 1]
    assert 0 < both < 0.1 * r["cover"][0, 2, 0]          # the two overlap in a narrow strip in front of B's middle


# ---- the two formulations -------------------------------------------------------------------------------------------------------------------------
def test_generator_seeds_meet_the_conditions():
    worst = min(sc.check_conditions(ref_of(f"room{seed}"))["margins"]["delta"] for seed in sc.ALL_ROOM_SEEDS)
    print(f"smallest |Delta| margin over the rooms: {worst:.2e}")
    sc.check_conditions(ref_of("crowd"))
    crowd = ref_of("crowd")
    tile = crowd["inst"][0, 16:32, 16:32]
    on_tile = [m for m in range(sc.CROWD_M) if crowd["cover"][0, m, 0] and (tile == m).any()]
    assert len(on_tile) >= 20 and min(on_tile) < 256 // 2 and max(on_tile) > 200


def test_two_formulations():
    worst, pairs = 0.0, 0
    for name, s in all_scenes().items():
        dx, dy = rr.pixel_rays(s["K"], s["rows"], s["cols"])
        for cam in s["cams"]:
            for v in s["objs"]:
                ok, _, sv = rr.valid_object(v)
                if not ok:
                    continue
                Rco, tco = rr.camera_frame(cam, v)
                A, g, c0 = rr.body(Rco, tco, sv)
                h2, z2 = rr.sphere_hits(Rco, tco, sv, dx, dy)
                if not c0 > 0:
                    assert not h2.any()
                    continue
                h1, z1, _ = rr.quadric_hits(A, g, c0, dx, dy)
                assert np.array_equal(h1, h2), name          # identical hit sets
                if h1.any():
                    worst = max(worst, float(np.abs(z1[h1] - z2[h1]).max()))
                    pairs += int(h1.sum())
    print(f"largest depth disagreement of the two formulations over {pairs} hits: {worst:.2e} m")
    assert pairs > 50000
    assert 0.5 * sc.FORMULATION_GAP <= worst <= sc.FORMULATION_GAP, "render_scenes.FORMULATION_GAP no longer states what is measured"
    assert sc.TOL == max(10 * sc.FORMULATION_GAP, 1e-9)


# ---- containment in the box -----------------------------------------------------------------------------------------------------------------------
def test_hits_lie_in_the_bbox_edges_box(po):
    checked = tight = 0
    worst_px = 0.0
    for name in [f"room{seed}" for seed in sc.ROOM_SEEDS] + ["crowd", "occluders", "across"]:
        s, ref = all_scenes()[name], ref_of(name)
        dx, dy = rr.pixel_rays(s["K"], s["rows"], s["cols"])
        for f, cam in enumerate(s["cams"]):
            for m, v in enumerate(s["objs"]):
                if not ref["flags"][f, m] & rr.BOUNDED:
                    continue
                box = np.asarray(po.project_bbox(cam, v, s["K"]))
                assert np.isfinite(box).all()
                Rco, tco = rr.camera_frame(cam, v)
                hit, _, _ = rr.quadric_hits(*rr.body(Rco, tco, np.abs(v[7:10])), dx, dy)
                if not hit.any():
                    continue
                ys, xs = np.nonzero(hit)
                assert box[0] < xs.min() and xs.max() < box[2] and box[1] < ys.min() and ys.max() < box[3], (name, f, m)
                checked += 1
                # A body at least 8 px across whose outline lies inside the image: its extreme hit columns and rows lie within one pixel
                # of the box, counted in pixels -- the outermost column the box reaches is floor(b2), and the last hit column is that one
                # or its neighbour.  As a real-valued distance b2 - max(col) the figure can pass 1 (1.0255 at the largest, printed below): the outline's
                # tip falls between two pixel rows, and at the rows beside it the outline is already narrower.
                if min(box[2] - box[0], box[3] - box[1]) >= 8 and box[0] > 0 and box[1] > 0 and box[2] < s["cols"] - 1 and box[3] < s["rows"] - 1:
                    assert xs.min() - np.ceil(box[0]) <= 1 and np.floor(box[2]) - xs.max() <= 1, (name, f, m, box, xs.min(), xs.max())
                    assert ys.min() - np.ceil(box[1]) <= 1 and np.floor(box[3]) - ys.max() <= 1, (name, f, m, box, ys.min(), ys.max())
                    worst_px = max(worst_px, xs.min() - box[0], box[2] - xs.max(), ys.min() - box[1], box[3] - ys.max())
                    tight += 1
    print(f"{checked} bodies inside their box, {tight} of them at least 8 px across: largest real-valued distance box edge - extreme hit {worst_px:.4f} px")
    assert checked > 150 and tight > 20


# ---- the header, stand-alone ------------------------------------------------------------------------------------------------------------------------
def build_ray_prog(tmp, flags):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/render_ray_main.cpp"
    exe = str(tmp / "render_ray_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", *flags, "-o", exe, os.path.join(ROOT, "tests", "render_ray_main.cpp")])
    return exe


def fmt(x):
    return " ".join("nan" if np.isnan(v) else repr(float(v)) for v in np.asarray(x, dtype=np.float64).reshape(-1))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan_ubsan"])
def test_ray_header_matches_the_statement(tmp_path, flags):
    exe = build_ray_prog(tmp_path, flags)
    far = dict(cams=sc.IDENTITY_CAM[None, :], objs=np.stack([sc.sphere([4e7, -3e7, 2.0], 0.5), sc.sphere([-9.0, 0.2, 3.0], 0.5)]), K=sc.K,
               rows=sc.ROWS, cols=sc.COLS)          # boxes far outside the image, one of them beyond the range of an int
    records, expect = [], []
    for s in (sc.room_scene(0), sc.room_scene(1), sc.across_scene(), sc.nothing_scene(), far):
        dx, dy = rr.pixel_rays(s["K"], s["rows"], s["cols"])
        for cam in s["cams"]:
            for v in s["objs"]:
                ok, q, sv = rr.valid_object(v)
                if ok:
                    Rco, tco = rr.camera_frame(cam, v)
                    C22, box = rr.conic_box(Rco, tco, sv, s["K"])
                    n = np.column_stack([Rco, tco]).T          # the columns of [Rco | tco], one per line
                else:
                    n, C22, box = np.zeros((4, 3)), 0.0, None
                box = np.full(4, np.nan) if box is None else box
                records.append(" ".join([fmt(v), fmt(n), fmt(box), fmt([C22]), fmt(s["K"]), str(s["rows"]), str(s["cols"])]))
                expect.append((s, ok, q, sv, (Rco, tco, C22, box) if ok else None, dx, dy))
    p = rr.DEFAULTS
    cmps = [(0, 2.0), (10000, 2.0), (10200, 2.0), (10300, 2.0), (9800, 2.0), (9700, 2.0), (499, 0.1), (500, 0.1), (30000, 6.0), (30001, 6.0),
            (65535, 6.0)]
    text = f"{len(records)}\n" + "\n".join(records) + f"\n{len(cmps)}\n" + "".join(
        f"{raw} {z!r} {p['depth_scale']!r} {p['depth_min']!r} {p['depth_max']!r} {p['depth_tol']!r}\n" for raw, z in cmps)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])          # 5: a hit pixel outside its body's bounds
    lines = iter(r.stdout.splitlines())
    n_hits = n_bounded = 0
    for s, ok, q, sv, geom, dx, dy in expect:
        w = next(lines).split()
        assert w[0] == "valid" and int(w[1]) == int(ok)
        if not ok:
            continue
        got = np.array(w[2:], dtype=np.float64)
        assert np.abs(got - np.concatenate([q, sv])).max() <= 1e-15
        Rco, tco, C22, box = geom
        A, g, c0 = rr.body(Rco, tco, sv)
        w = next(lines).split()
        b = np.array(w[1:], dtype=np.float64)
        want = np.array([A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2], g[0], g[1], g[2], c0])
        assert w[0] == "body" and np.abs(b - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        w = next(lines).split()
        fl, x0, x1, y0, y1 = map(int, w[1:])
        rows, cols = s["rows"], s["cols"]
        if not c0 > 0:
            assert (fl, x1 < x0) == (rr.INSIDE, True)
            continue
        if C22 < 0 and tco[2] < 0:
            assert (fl, x1 < x0) == (0, True)
            continue
        hit, z, _ = rr.quadric_hits(A, g, c0, dx, dy)
        if C22 < 0 and np.isfinite(box).all():
            assert fl == rr.DRAWN | rr.BOUNDED
            e = (max(np.floor(box[0]) - 1, 0), min(np.ceil(box[2]) + 1, cols - 1), max(np.floor(box[1]) - 1, 0), min(np.ceil(box[3]) + 1, rows - 1))
            if e[0] <= e[1] and e[2] <= e[3]:
                assert (x0, x1, y0, y1) == tuple(int(v) for v in e)
            else:
                assert x1 < x0 and y1 < y0 and not hit.any()
            n_bounded += 1
        else:
            assert fl == rr.DRAWN and (x0, x1, y0, y1) == (0, cols - 1, 0, rows - 1)
        ys, xs = np.nonzero(hit)
        for y, x in zip(ys, xs):          # row-major, as the program walks
            w = next(lines).split()
            assert (w[0], int(w[1]), int(w[2])) == ("hit", x, y)
            assert abs(float(w[3]) - z[y, x]) <= sc.TOL
            assert x0 <= x <= x1 and y0 <= y <= y1          # the bounds contain every hit pixel
        n_hits += len(ys)
    # render_behind: z lies in (c0 / (2 beta), c0 / beta), so against a running minimum below half the hit's depth it says "cannot win"
    # for every hit (five of the program's thirteen minima), never against one within 1e-7 of the depth or beyond (four), and the
    # program has checked each "cannot win" against the depth itself
    w = next(lines).split()
    assert w[0] == "behind" and 5 * n_hits <= int(w[1]) <= 9 * n_hits
    want_cmp = [3, 0, 0, 2, 0, 1, 3, 0, 0, 3, 3]          # no data, agree, agree, farther, agree, nearer, below depth_min, at it, at depth_max, ...
    assert [next(lines) for _ in cmps] == [f"cmp {k}" for k in want_cmp]
    assert next(lines, None) is None and n_hits > 3000 and n_bounded > 60
    cat, _ = rr.compare(np.array([c[0] for c in cmps], dtype=np.uint16), np.array([c[1] for c in cmps]), p)
    assert list(cat) == want_cmp


# ---- the binding ----------------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_listed_exported_and_struct_size(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esl.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+esl_render_map\s*\(", txt) and re.search(r"\}\s*esl_render_params\s*;", txt)
    assert {"esl_render_params_default", "esl_render_map"} <= set(pkg.lib.EXPORTS)
    L = pkg.lib.load()
    assert ctypes.sizeof(pkg.abi.EslRenderParams) == 32
    p = pkg.abi.EslRenderParams()
    L.esl_render_params_default(ctypes.byref(p))          # host code: runs without a device
    d = pkg.abi.default_render_params()
    for k, _ in pkg.abi.EslRenderParams._fields_:
        assert getattr(p, k) == getattr(d, k) == rr.DEFAULTS[k], k
    assert L.esl_abi_version() == 5
    assert callable(pkg.Context.render_map)
