"""The adapter reads the config key Optimizer.Localization (1 = every ellipsoid fixed: vEllipsoid->setFixed(true) where the reference
hard-wires false, Optimizer.cpp:178): the Tracking-shaped replay of test_adapter_link.py, linked with a translation unit that sets
the key, must return what Context.optimize(..., obj_fixed=ones) returns -- the ellipsoids unchanged, in mapping mode (nothing moves)
and in SLAM mode (pose-only refinement; the adapter, like the reference, writes back the ellipsoids only) -- and print the counts
of the active bbox edges."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import test_adapter_link as tal


def build_localization(tmp_path):
    exe = str(tmp_path / "tracking_calls_localization")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror=return-type", "-DESL_BUILD_IN_REFERENCE_TREE", "-I", tal.STUBS,
           "-I", os.path.join(tal.ROOT, "include"), "-I", os.path.join(tal.ROOT, "adapter")]
    cmd += [os.path.join(tal.ROOT, "adapter", a) for a in tal.ADAPTERS]
    cmd += [os.path.join(tal.STUBS, "tracking_calls.cpp"), os.path.join(tal.STUBS, "localization_config.cpp")]
    cmd += ["-L", tal.CSRC, "-lesl_hip", "-Wl,-rpath," + tal.CSRC, "-pthread", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_adapter_with_localization_key_links(tmp_path):
    exe = build_localization(tmp_path)
    syms = subprocess.check_output(["nm", "-C", exe]).decode()
    assert "esl_optimize_fixed" in syms


@pytest.mark.gpu
def test_adapter_localization_replay_matches_c_abi(pkg, ctx, tmp_path):
    exe = build_localization(tmp_path)
    # the scene of test_adapter_link.py's replay
    g, c, o, _ = pkg.synth.make_graph(14, 4, 44, seed=5, frac_3d=0.5)
    sc = pkg.synth.make_depth_scene(n_objs=1, seed=5, size=(0.3, 0.35))
    K = pkg.synth.TUM3_K
    rows, cols = 480, 640
    ground = np.array([0.0, 0.0, 1.0, 0.0])
    Twc = np.array([tal._inv7(t) for t in c])
    meas = g.bbox_meas.reshape(-1, 4)
    lines = ["%r %r %r %r 5000.0 %d %d" % (K[0], K[1], K[2], K[3], rows, cols), " ".join(repr(float(v)) for v in ground), str(len(c))]
    for i in range(len(c)):
        lines.append(" ".join(repr(float(v)) for v in list(Twc[i]) + list(c[i])))
    lines.append(str(len(g.bbox_cam)))
    for i in range(len(g.bbox_cam)):
        lines.append("%d %d %s %r 0" % (g.bbox_cam[i], g.bbox_obj[i], " ".join(repr(float(v)) for v in meas[i]), float(g.bbox_weight[i])))
    e3 = g.e3d_meas.reshape(-1, 10)
    lines.append(str(len(g.e3d_cam)))
    for i in range(len(g.e3d_cam)):
        lines.append("%d %d %s %r" % (g.e3d_cam[i], g.e3d_obj[i], " ".join(repr(float(v)) for v in e3[i]), float(g.e3d_weight[i]) / 10000.0))
    raw = tmp_path / "depth.raw"
    sc["depth"].astype(np.uint16).tofile(str(raw))
    b = sc["bboxes"][0]
    lines.append("1 %d %d %s %r %r %r %r 28 %s" % (sc["depth"].shape[1], sc["depth"].shape[0], " ".join(repr(float(v)) for v in sc["Twc"]),
                                                  float(b[0]), float(b[1]), float(b[2]), float(b[3]), str(raw)))
    from test_plane import scene as floor_scene
    gdepth, _, _ = floor_scene(h=rows, w=cols, noise=2.0, seed=11)
    graw = tmp_path / "ground.raw"
    gdepth.astype(np.uint16).tofile(str(graw))
    lines.append("GROUNDDEPTH %d %d %s" % (cols, rows, str(graw)))
    scene = tmp_path / "scene.txt"
    scene.write_text("\n".join(lines) + "\n")
    out = subprocess.check_output([exe, str(scene)], cwd=str(tmp_path), stderr=subprocess.STDOUT).decode()
    rec = tal.parse(out)
    assert "LINK-OK" in rec

    # the ellipsoids the optimiser is given: the SVD initialisations the replay printed
    init = {int(r[0]): np.array([float(v) for v in r[1:]]) for r in rec["INIT"]}
    inst_of = sorted(init)
    objs = np.array([init[i] for i in inst_of])
    assert len(objs) >= 2
    remap = -np.ones(g.n_objs, dtype=int)
    remap[inst_of] = np.arange(len(inst_of))
    cnt = np.bincount(g.bbox_obj, minlength=g.n_objs)
    mb = (remap[g.bbox_obj] >= 0) & (cnt[g.bbox_obj] > 2)
    me = remap[g.e3d_obj] >= 0
    order_e = np.argsort(g.e3d_cam[me], kind="stable")
    ones = np.ones(len(objs), np.uint8)
    edges = (g.bbox_cam[mb], remap[g.bbox_obj[mb]], meas[mb], g.bbox_weight[mb], g.e3d_cam[me][order_e], remap[g.e3d_obj[me]][order_e],
             e3[me][order_e], g.e3d_weight[me][order_e], np.arange(len(objs)), ground, 100.0 ** 2)
    # mapping mode: nothing to optimise, nothing moves
    gg = pkg.Graph(K, len(c), len(objs), None, *edges)
    cm, om, repm = ctx.optimize(gg, c, objs, pkg.default_lm_params(), obj_fixed=ones)
    assert repm["stop_reason"] == 3 and np.array_equal(om, objs) and np.array_equal(cm, c)
    opt = {int(r[0]): np.array([float(v) for v in r[1:]]) for r in rec["OPT"]}
    # SLAM mode: the trajectory is refined against the map, the map is written back as it was
    from oracle import pyoracle as po
    fixed = np.zeros(len(c), np.uint8); fixed[0] = 1
    Tcw_in = np.array([po.se3_inv(t) for t in Twc])
    Z = np.array([po.se3_mul(Tcw_in[i], po.se3_inv(Tcw_in[i - 1])) for i in range(1, len(c))])
    gs = pkg.Graph(K, len(c), len(objs), fixed, *edges, odom_i=np.arange(len(c) - 1), odom_j=np.arange(1, len(c)), odom_meas=Z,
                   check_visibility=1, image_rows=rows, image_cols=cols)
    cs, os_, reps = ctx.optimize(gs, c, objs, pkg.default_lm_params(), obj_fixed=ones)
    assert ctx.lm_solver_used() == 3 and reps["iterations"] >= 1 and np.array_equal(os_, objs)
    assert np.abs(cs - c).max() > 1e-9                         # the C-ABI run did move the cameras
    opts = {int(r[0]): np.array([float(v) for v in r[1:]]) for r in rec["OPTSLAM"]}
    assert len(opt) == len(opts) == len(inst_of)
    for k, inst in enumerate(inst_of):
        np.testing.assert_allclose(opt[inst], om[k], rtol=0, atol=1e-9)      # (the tolerance of test_adapter_link.py:162)
        np.testing.assert_allclose(opts[inst], os_[k], rtol=0, atol=1e-9)
    # the graph summaries report the ACTIVE bbox edges: none in mapping mode, the anchored ones in SLAM mode
    counts = re.findall(r"2d Edges \[Valid/Invalid\] : (\d+) \[(\d+)/(\d+)\]", out)
    assert len(counts) == 2
    assert [int(v) for v in counts[0]] == [int(mb.sum()), repm["n_bbox_valid"], repm["n_bbox_dropped"]] and repm["n_bbox_valid"] == 0
    assert [int(v) for v in counts[1]] == [int(mb.sum()), reps["n_bbox_valid"], reps["n_bbox_dropped"]]
    assert reps["n_bbox_valid"] + reps["n_bbox_dropped"] == int((mb & (g.bbox_cam != 0)).sum())
