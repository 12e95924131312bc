"""The numpy statement of esl_dense_carve_frames (tests/dense_carve_ref.py) on its own: the premises every device scene of
tests/test_gpu_dense_carve.py relies on, the exact scenes' classes made by hand, and csrc/esl_dense_carve.hpp held to the statement on
the host (plain and under AddressSanitizer + UBSan, as a stand-alone program: nothing is preloaded into Python).

The statement's numbers on `ghost` (48 x 64, leaf 0.05, observers = the last three views, owners = all six, min_through 2,
through_per_agree 1): 7376 voxels, 208 of them with samples from box pixels only, 5 mixed.
  window 0: 209 carved = 204 box-only + 5 static (wall voxels at a depth edge read one pixel beside their own surface)
  window 1: 192 carved = 192 box-only + 0 static; 389 samples carved        <- the default window
  window 2: 183 carved = 183 box-only + 0 static
  observers = all six frames, window 1: 189 carved, all box-only, 0 static: the box's own frames agree with its voxels, so the few
  voxels with as many agreeing as through observations are kept (through >= through_per_agree * agree fails for 3 of the 192)
`ghost_odd` (45 x 61): 7090 voxels, 215 box-only; window 1: 199 carved, 0 static."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_carve_ref as dcr          # noqa: E402
import dense_carve_scenes as cs        # noqa: E402
import dense_ref as dr                 # noqa: E402
from dense_prog import BUILDS, BUILD_IDS, NONFINITE, build_prog, check_ladder          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(sc, m, obs, own, **kw):
    o, w = list(obs), list(own)
    sub = lambda a, i: None if a is None else a[i]          # noqa: E731
    return dcr.carve(m, sc["cams"][o], sc["depth"][o], sc["cams"][w], sc["depth"][w], sc["K"], sc["rows"], sc["cols"], sub(sc["bgr"], w),
                     sub(sc["inst"], w), **kw)


def invariants(r):
    F = len(r["cls"])
    in_view = (r["cls"] <= dcr.NODATA).sum(axis=0)
    assert np.array_equal(r["vox"].sum(axis=1), in_view)          # each voxel's four counts sum to its in-view frames
    assert r["vox"].sum(axis=0).tolist() == r["obs"][:, 3:7].sum(axis=0).tolist()          # column sums agree
    assert np.array_equal(r["obs"][:, 3:7].sum(axis=1), r["obs"][:, 0]) and (r["obs"][:, :3].sum(axis=1) == r["result"]["n_voxels"]).all()
    assert (r["obs"][:, 7] == 0).all() and r["obs"].shape == (F, 8)
    assert np.array_equal(r["own"][:, 1] + r["own"][:, 3], r["own"][:, 0]) and np.array_equal(r["own"][:, 2], r["mask"].sum(axis=(1, 2)))


@pytest.mark.parametrize("name", ["ghost", "ghost_odd"])
def test_ghost_premises(name):
    sc = cs.ghost_scene(name)
    m = cs.build(sc)
    box, other = cs.voxel_origin(sc, m)
    box_only, static = (box > 0) & (other == 0), box == 0
    assert (sc["hit"][:3].sum(axis=(1, 2)) > 100).all() and not sc["hit"][3:].any()
    r = run(sc, m, (3, 4, 5), range(6))
    invariants(r)
    cv = r["carved"].astype(bool)
    print(name, r["result"], int(box_only.sum()), int((cv & box_only).sum()), int((cv & static).sum()))
    assert not (cv & static).any()          # no voxel whose samples all come from non-box pixels is carved
    must = box_only & (r["vox"][:, 2] >= 2) & (r["vox"][:, 0] == 0)
    assert must.sum() > 150 and cv[must].all()
    assert (cv & box_only).sum() * 4 >= box_only.sum() * 3          # a clear majority: the statement gives 192 of 208 and 199 of 215
    if name == "ghost":
        assert (len(cv), int(box_only.sum()), int(cv.sum()), r["result"]["samples_carved"]) == (7376, 208, 192, 389)
        w0 = run(sc, m, (3, 4, 5), range(6), window=0)
        c0 = w0["carved"].astype(bool)
        assert (int(c0.sum()), int((c0 & static).sum())) == (209, 5)          # why the default window is 1
    else:
        assert len(cv) % 64 and len(cv) % 256 and r["own"][0, 0] % 64 and r["own"][0, 0] % 256
    # the carved samples are box pixels of the first three frames, nothing else
    assert (r["mask"][3:] == 0).all() and not (r["mask"].astype(bool) & ~sc["hit"]).any()
    assert ((r["depth_kept"] == 0) == (r["mask"] == 1)).all() and (r["depth_kept"][r["mask"] == 0] == sc["depth"][r["mask"] == 0]).all()
    assert r["result"]["removed"] == dcr.ZERO_REMOVED and m.extract()["n_voxels"] == len(cv)          # apply = 0 leaves the map


def test_all_six_observers():
    sc = cs.ghost_scene("ghost")
    m = cs.build(sc)
    box, other = cs.voxel_origin(sc, m)
    r = run(sc, m, range(6), range(6))
    invariants(r)
    cv = r["carved"].astype(bool)
    late = run(sc, m, (3, 4, 5), range(6))["carved"].astype(bool)
    # the box's own frames add agreeing observations: nothing new is carved, a few box voxels are kept, no static voxel is carved
    assert not (cv & ~late).any() and 0 < (late & ~cv).sum() < 10 and not (cv & (box == 0)).any() and cv.sum() == 189
    assert r["result"]["n_tested"] == r["result"]["n_voxels"]          # every voxel is seen by the frame that made it
    # through_per_agree = 0 leaves min_through alone
    r0 = run(sc, m, range(6), range(6), through_per_agree=0)
    assert np.array_equal(r0["carved"], (r0["vox"][:, 2] >= 2).astype(np.uint8)) and np.array_equal(r0["vox"], r["vox"])


@pytest.mark.parametrize("name", list(cs.GHOSTS))
def test_apply_equals_the_map_of_the_kept_images(name):
    sc = cs.ghost_scene(name)
    m = cs.build(sc)
    slots0 = m.slots()
    r = run(sc, m, (3, 4, 5), range(6), apply=1)
    res = r["result"]
    assert res["status"] == 0 and res["n_carved"] > 50 and res["removed"]["n_missing"] == 0 and res["removed"]["status"] == 0
    assert res["removed"]["n_used"] == res["samples_carved"] and res["removed"]["n_emptied"] == res["n_carved"]
    assert m.slots()["dead_voxels"] == slots0["dead_voxels"] + res["n_carved"]
    fresh = cs.build(dict(sc, depth=r["depth_kept"]))
    a, b = m.extract(), fresh.extract()
    assert a["n_voxels"] == b["n_voxels"] == res["n_voxels"] - res["n_carved"]
    for k in ("key", "xyz", "count", "bgr", "inst", "votes"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert m.info() == fresh.info()
    again = run(sc, m, (3, 4, 5), range(6), apply=1)
    assert again["result"]["n_carved"] == 0 and again["result"]["samples_carved"] == 0


def test_half_the_owners_thin_the_voxels():
    sc = cs.ghost_scene("ghost")
    m = cs.build(sc)
    full = run(sc, cs.build(sc), (3, 4, 5), range(6))
    r = run(sc, m, (3, 4, 5), (0, 2, 4), apply=1)
    assert np.array_equal(r["carved"], full["carved"]) and 0 < r["result"]["samples_carved"] < full["result"]["samples_carved"]
    # frame 1's samples stay: some carved voxels live on with fewer samples, none of them gained any
    assert 0 < r["result"]["removed"]["n_emptied"] < r["result"]["n_carved"] and r["result"]["removed"]["n_missing"] == 0
    cv = full["carved"].astype(bool)
    before = cs.build(sc).extract()
    after = {tuple(k): c for k, c in zip(m.extract()["key"].tolist(), m.extract()["count"].tolist())}
    left = [after.get(tuple(k), 0) for k in before["key"][cv].tolist()]
    assert all(a <= b for a, b in zip(left, before["count"][cv].tolist())) and 0 < sum(1 for a in left if a > 0) < len(left)


@pytest.mark.parametrize("name", cs.EXACT)
def test_exact_scenes(name):
    e = cs.exact_scene(name)
    m = cs.build(e["map"])
    same = (tuple(e["K"]), e["rows"], e["cols"]) == (tuple(e["map"]["K"]), 1, 1)          # the owners share the observers' K and image size
    r = dcr.carve(m, e["cams_obs"], e["depth_obs"], e["map"]["cams"] if same else None, e["map"]["depth"] if same else None, e["K"], e["rows"],
                  e["cols"], **e["params"])
    invariants(r)
    want = cs.exact_classes(name, m)
    assert np.array_equal(r["cls"], want), (r["cls"].tolist(), want.tolist())
    assert set(np.unique(want)) >= {dict(tol=2, gate=4, half=0, border=5, mix=1, mix_w0=3)[name]}
    # the verdict at min_through = 1: carved iff through >= 1 and through >= agree
    assert np.array_equal(r["carved"], ((r["vox"][:, 2] >= 1) & (r["vox"][:, 2] >= r["vox"][:, 0])).astype(np.uint8))
    # owners at K = (1, 1, 0, 0), rows = cols = 1: one sample per voxel, found; it is carved iff its voxel is
    if same:
        assert r["own"][:, :2].tolist() == [[1, 1]] * len(e["points"]) and r["own"][:, 2].sum() == r["carved"].sum()
    assert same == (name in ("tol", "gate"))


def test_invalid_map_and_pose():
    sc = cs.full_scene()
    m = cs.build(sc)
    assert m.status == 3
    e = cs.exact_scene("tol")
    r = dcr.carve(m, e["cams_obs"], e["depth_obs"], None, None, e["K"], 1, 1)
    assert r == dict(result=dict(status=3, n_voxels=-1, n_tested=0, n_carved=0, samples_found=0, samples_carved=0, removed=dcr.ZERO_REMOVED))
    with pytest.raises(dr.InvalidPose):
        dcr.carve(cs.build(e["map"]), [[0, 0, 0, 0, 0, 0, 0]], e["depth_obs"][:1], None, None, e["K"], 1, 1)
    empty = dcr.carve(cs.build(e["map"], frames=[]), e["cams_obs"], e["depth_obs"], e["map"]["cams"], e["map"]["depth"], e["K"], 1, 1)
    assert empty["result"]["n_voxels"] == 0 and empty["own"].tolist() == [[1, 0, 0, 1]] and (empty["obs"] == 0).all()


# ---- the header against the statement -----------------------------------------------------------------------------------------------------
def cases():
    """(name, xyz, cams, depth, K, rows, cols, params) of every scene the program is held to"""
    for name in ("ghost", "ghost_odd"):
        sc = cs.ghost_scene(name)
        for w in (0, 1, 2, 4):
            yield f"{name}_w{w}", cs.build(sc).extract()["xyz"], sc["cams"], sc["depth"], sc["K"], sc["rows"], sc["cols"], dict(dcr.DEFAULTS, window=w)
    for name in cs.EXACT:
        e = cs.exact_scene(name)
        yield name, cs.build(e["map"]).extract()["xyz"], e["cams_obs"], e["depth_obs"], e["K"], e["rows"], e["cols"], dict(dcr.DEFAULTS, **e["params"])


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan_ubsan"])
def test_carve_header_matches_the_statement(tmp_path, flags):
    exe = build_prog(tmp_path, "dense_carve_main", flags)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "dense_carve ok"
    seen = set()
    for name, xyz, cams, depth, K, rows, cols, p in cases():
        F, n = len(cams), len(xyz)
        path = tmp_path / f"{name}.txt"
        with open(path, "w") as fh:
            fh.write(f"{rows} {cols} {p['window']} {p['depth_scale']!r} {p['depth_min']!r} {p['depth_max']!r} {p['depth_tol']!r} {p['min_through']} "
                     f"{p['through_per_agree']} " + " ".join(repr(float(v)) for v in K) + f" {n} {F}\n")
            fh.write("\n".join(" ".join(repr(float(v)) for v in row) for row in xyz) + "\n")
            for f in range(F):
                fh.write(" ".join(repr(float(v)) for v in cams[f]) + "\n" + " ".join(str(int(v)) for v in depth[f].reshape(-1)) + "\n")
        out = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == F + n + 1, name
        cls = np.stack([dcr.observe(xyz, cams[f], K, rows, cols, depth[f], p) for f in range(F)])
        got = np.array([[int(v) for v in line.split()] for line in out[:F]], np.int64).reshape(F, n)
        assert np.array_equal(got, cls), name
        vox = np.stack([(cls == k).sum(axis=0) for k in range(4)], axis=-1)
        want = np.concatenate([vox, dcr.verdict(vox, p).astype(np.int64)[:, None]], axis=1)
        assert np.array_equal(np.array([[int(v) for v in line.split()] for line in out[F:F + n]], np.int64).reshape(n, 5), want), name
        seen |= set(np.unique(cls).tolist())
    assert seen == {0, 1, 2, 3, 4, 5}


# ---- what esl_dense_carve_frames refuses for its parameters (csrc/esl_dense_check.hpp), text by text and in order -------------------------
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
def test_carve_params_check_texts_and_order(tmp_path, flags):
    """dcv_params_check: every rung at its last accepted and first refused value, NaN and the infinities in every double, and the
    earlier rung's text when two fail."""
    exe = build_prog(tmp_path, "dense_carve_main", flags)
    defaults = dict(dcr.DEFAULTS)
    assert defaults["depth_max"] == 6.0 and defaults["window"] == 1 and defaults["apply"] == 0
    rungs = GATE_RUNGS + [
        ("window outside 0 .. 4", [dict(window=0), dict(window=4)], [dict(window=-1), dict(window=5)]),
        ("min_through < 1", [dict(min_through=1)], [dict(min_through=0)]),
        ("negative through_per_agree", [dict(through_per_agree=0)], [dict(through_per_agree=-1)]),
        ("apply not 0 or 1", [dict(apply=0), dict(apply=1)], [dict(apply=-1), dict(apply=2)]),
    ]
    fields = ["depth_scale", "depth_min", "depth_max", "depth_tol", "window", "min_through", "through_per_agree", "apply"]
    check_ladder(exe, fields, defaults, rungs)
