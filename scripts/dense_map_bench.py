#!/usr/bin/env python3
"""Time esl_dense_add_frames / esl_dense_extract on a synthetic room: 100 frames of 640 x 480, stride 1, leaf 0.01, with colour and
labels, for BOTH forms of k_dense_insert (ESL_DENSE_COMBINE=0: one probe and seven atomics per sample; 1: the in-wave run combine).

Recorded, not gated (profiles/dense_map_c4.json, DESIGN.md "The dense map"): there is no earlier implementation to compare with.  Two
clocks, after a warm-up map (buffers grown, kernels loaded): HIP events on the context's stream around the kernel launches
(esl_profile_enable(ctx, 2), kernel class 4), and the host clock around the C-ABI call, which adds the copies in and out.  Two
yardsticks beside them: the time to stream the call's inputs once at the measured HBM rate (9 bytes per pixel: depth 2, bgr 3, inst 4),
and the numpy statement (tests/dense_ref.py) on the first frames of the same data, on one core, scaled to all frames.

    python scripts/dense_map_bench.py --out profiles/dense_map_c4.json
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS, COLS = 480, 640
K = (525.0, 525.0, 319.5, 239.5)
HBM_MEASURED = 6.29e12          # bytes / s, a float4 copy on this part
BYTES_PER_PIXEL = 9
HALF = np.array([2.503, 1.507, 2.004])          # the room: |x| <= 2.503, |y| <= 1.507, |z| <= 2.004 m (no wall on a voxel boundary)


def stats_of(ms):
    ms = np.sort(np.asarray(ms))
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms[0]), ms_max=float(ms[-1]))


def room_frames(F, seed=0):
    """cameras on a circle of radius 0.5 m inside the room, turning about the vertical (y) axis; depth by ray casting the six walls,
    quantised; inst = the wall hit (the floor unlabelled); colour = a 10 cm checker of the world point"""
    import dense_ref as dr
    rng = np.random.default_rng(seed)
    cams = np.zeros((F, 7))
    depth = np.zeros((F, ROWS, COLS), np.uint16); inst = np.zeros((F, ROWS, COLS), np.int32); bgr = np.zeros((F, ROWS, COLS, 3), np.uint8)
    dx = (np.arange(COLS) - K[2]) / K[0]; dy = (np.arange(ROWS) - K[3]) / K[1]
    d_c = np.stack(np.broadcast_arrays(dx[None, :], dy[:, None], np.ones((ROWS, COLS))), axis=-1)
    for f in range(F):
        ang = 2 * np.pi * f / F
        q = np.array([0.0, np.sin(ang / 2), 0.0, np.cos(ang / 2)])          # Rcw: a turn about y
        cams[f, 3:] = q
        R, _ = dr.pose(cams[f])
        centre = np.array([0.5 * np.cos(ang), 0.1 * np.sin(3 * ang), 0.5 * np.sin(ang)])
        cams[f, :3] = -R @ centre          # p_c = R (p_w - centre)
        d_w = d_c @ R          # R^T d per pixel
        with np.errstate(divide="ignore", invalid="ignore"):
            t_pos = (HALF - centre) / d_w; t_neg = (-HALF - centre) / d_w
        t = np.where(d_w > 0, t_pos, np.where(d_w < 0, t_neg, np.inf))          # the exit distance per axis, in units of camera z
        ax = np.argmin(t, axis=-1)
        z = np.take_along_axis(t, ax[..., None], axis=-1)[..., 0]
        depth[f] = np.clip(np.rint(z * 5000.0), 0, 65535).astype(np.uint16)
        side = np.take_along_axis(d_w, ax[..., None], axis=-1)[..., 0] > 0
        wall = 2 * ax + side
        inst[f] = np.where(wall == 3, -1, wall)          # +y is the floor
        p_w = centre + z[..., None] * d_w
        chk = (np.floor(p_w / 0.1).astype(np.int64).sum(-1) & 1).astype(np.uint8)
        bgr[f] = (60 + 120 * chk[..., None] + 10 * wall[..., None] + rng.integers(0, 8, (ROWS, COLS, 3))).astype(np.uint8)
    return cams, depth, bgr, inst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--numpy-frames", type=int, default=2, help="frames of the numpy statement's cut (0: skip it)")
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    t0 = time.perf_counter()
    cams, depth, bgr, inst = room_frames(a.frames)
    print(f"scene built in {time.perf_counter() - t0:.1f} s", flush=True)
    F = a.frames
    n_pix = F * ROWS * COLS
    params = pkg.abi.default_dense_params(max_voxels=a.max_voxels)
    out = dict(config=dict(frames=F, rows=ROWS, cols=COLS, stride=1, leaf=0.01, with_color=1, with_inst=1, max_voxels=a.max_voxels,
                           calls=a.calls, K=list(K)),
               timing="kernel: HIP events around the launches (esl_profile, class 4); call: host clock around the C-ABI call (copies included)",
               yardsticks=dict(hbm_bytes_per_s=HBM_MEASURED, bytes_per_pixel=BYTES_PER_PIXEL,
                               stream_inputs_once_ms=n_pix * BYTES_PER_PIXEL / HBM_MEASURED * 1e3))
    ctx = pkg.Context(0)
    maps = {}
    for form, name in (("0", "plain"), ("1", "combined")):
        os.environ["ESL_DENSE_COMBINE"] = form          # read by esl_dense_begin
        ctx.dense_begin(params)
        ctx.dense_add_frames(cams, K, ROWS, COLS, depth, bgr, inst); ctx.dense_extract()          # warm-up
        ctx.profile_enable(2)
        prev = ctx.profile_get().get("reduce", dict(count=0, total_ms=0.0))
        rec = dict(add_kernel=[], add_call=[], extract_kernel=[], extract_call=[])
        for _ in range(a.calls):
            ctx.dense_begin(params)
            res = ctx.dense_add_frames(cams, K, ROWS, COLS, depth, bgr, inst)
            rec["add_call"].append(ctx.last_call_s * 1e3)
            pr = ctx.profile_get()["reduce"]; rec["add_kernel"].append(pr["total_ms"] - prev["total_ms"]); prev = pr
            ext = ctx.dense_extract()
            rec["extract_call"].append(ctx.last_call_s * 1e3)
            pr = ctx.profile_get()["reduce"]; rec["extract_kernel"].append(pr["total_ms"] - prev["total_ms"]); prev = pr
        ctx.profile_enable(0)
        info = ctx.dense_info()
        maps[name] = ext
        k_add = float(np.median(rec["add_kernel"]))
        out[name] = dict({k: stats_of(v) for k, v in rec.items()}, add_result=res, info=info,
                         samples_per_s_kernel=res["n_used"] / (k_add * 1e-3), input_bytes_per_s_kernel=n_pix * BYTES_PER_PIXEL / (k_add * 1e-3),
                         labelled_voxels=int((ext["inst"] >= 0).sum()))
        print(name, json.dumps(out[name]), flush=True)
    os.environ.pop("ESL_DENSE_COMBINE", None)
    out["forms_bit_identical"] = bool(all(maps["plain"][k].tobytes() == maps["combined"][k].tobytes() for k in ctx.DENSE_OUTPUTS))
    out["combined_over_plain_add_kernel"] = out["combined"]["add_kernel"]["ms_median"] / out["plain"]["add_kernel"]["ms_median"]
    if a.numpy_frames > 0:
        import dense_ref as dr
        n = min(a.numpy_frames, F)
        t0 = time.perf_counter()
        m = dr.DenseMap(max_voxels=a.max_voxels)
        radd = m.add_frames(cams[:n], K, ROWS, COLS, depth[:n], bgr[:n], inst[:n])
        ref = m.extract()
        secs = time.perf_counter() - t0
        ctx.dense_begin(params)
        dadd = ctx.dense_add_frames(cams[:n], K, ROWS, COLS, depth[:n], bgr[:n], inst[:n])
        dev = ctx.dense_extract()
        out["numpy_cut"] = dict(frames=n, seconds=secs, scaled_to_all_frames_s=secs * F / n, counts_equal=bool(dadd == radd),
                                outputs_equal={k: bool(dev[k].tobytes() == ref[k].tobytes()) for k in ctx.DENSE_OUTPUTS},
                                n_voxels=[int(dev["n_voxels"]), int(ref["n_voxels"])], smallest_margins=m.margins())
        print("numpy_cut", json.dumps(out["numpy_cut"]), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
