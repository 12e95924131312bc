#!/usr/bin/env python3
"""Time esl_init_quadrics on BASELINE configs[3] (synth.make_config("C4"): 10,000 frames, 2,000 ellipsoids, 200,000 boxes) against the
loop of esl_init_quadric calls over the same objects.

Recorded, not gated (profiles/init_batch_c4.json, DESIGN.md "SVD initialisation of many ellipsoids").  All clocks after warm-up calls
(buffers grown, kernels loaded, clocks up), median / min / p90 over the timed calls:
  kernel  HIP events on the context's stream around the launches (esl_profile_enable(ctx, 2), kernel class 4)
  call    the host clock around the C-ABI call: adds the grouping on the host, the copies of the poses and the list in and of the
          results out, and the synchronise the call ends with
  loop    the host clock around one esl_init_quadric call per object (each ends in a synchronise), over a sample of the objects (every
          --loop-stride-th, so that short and long ones are in it), scaled to all of them by the sample's share of the observations

    python scripts/init_batch_bench.py --out profiles/init_batch_c4.json
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

TILE, TILE_SMALL = 248, 96   # kInitTile, kInitTileSmall of csrc/esl_init.hip


def stats_of(ms):
    ms = np.sort(np.asarray(ms))
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms[0]), ms_p90=float(ms[int(0.9 * (len(ms) - 1))]))


def se3_inv(T):
    """Twc of Tcw, rows x y z qx qy qz qw"""
    q = T[:, 3:7] / np.linalg.norm(T[:, 3:7], axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                  2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    t = -np.einsum("nji,nj->ni", R, T[:, :3])
    return np.concatenate([t, -q[:, :3], q[:, 3:]], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-stride", type=int, default=10, help="the single-call loop runs every n-th object")
    ap.add_argument("--loop-passes", type=int, default=3)
    ap.add_argument("--faithful", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    g, cams, _, _ = pkg.synth.make_config(a.config)
    N = g.n_objs
    oc, oo, ob = np.asarray(g.bbox_cam, np.int32), np.asarray(g.bbox_obj, np.int32), np.ascontiguousarray(g.bbox_meas, dtype=np.float64)
    cnt = np.bincount(oo, minlength=N)
    ctx = pkg.Context(0)
    args = (cams, N, oc, oo, ob, g.K)
    kw = dict(rows=g.image_rows, cols=g.image_cols, faithful=a.faithful)
    for _ in range(a.warmup):
        ctx.init_quadrics(*args, **kw)
    call = []
    for _ in range(a.calls):          # profiler off: the call as a user times it
        ell, Q, err, st = ctx.init_quadrics(*args, **kw)
        call.append(ctx.last_call_s * 1e3)
    ctx.profile_enable(2)
    prev = ctx.profile_get().get("reduce", dict(count=0, total_ms=0.0))    # the counters run on: take differences
    kern, brackets = [], 0
    for _ in range(a.calls):
        ctx.init_quadrics(*args, **kw)
        pr = ctx.profile_get()["reduce"]
        kern.append(pr["total_ms"] - prev["total_ms"]); brackets = pr["count"] - prev["count"]
        prev = pr
    ctx.profile_enable(0)
    out = dict(config=dict(name=a.config, frames=int(g.n_cams), objects=int(N), observations=int(len(oo)), faithful=a.faithful, calls=a.calls,
                           warmup=a.warmup, tile=TILE, tile_small=TILE_SMALL),
               timing="kernel: HIP events around the launches (esl_profile, class 4); call, loop: host clock around the C-ABI calls",
               observations_per_object=dict(min=int(cnt.min()), median=float(np.median(cnt)), max=int(cnt.max())),
               status_counts=[int((st[:, 0] == k).sum()) for k in range(4)],
               objects_small_tile=int((cnt <= TILE_SMALL).sum()), objects_large_tile=int(((cnt > TILE_SMALL) & (cnt <= TILE)).sum()),
               spilled_objects=int(st[:, 3].sum()), spilled_share_of_observations=float(cnt[st[:, 3] == 1].sum() / max(1, cnt.sum())),
               event_brackets_per_call=int(brackets), kernel=stats_of(kern), call=stats_of(call))
    # the loop the batched call replaces: one esl_init_quadric per object, poses as Twc
    order = np.argsort(oo, kind="stable")
    off = np.concatenate([[0], np.cumsum(cnt)])
    sample = np.arange(0, N, a.loop_stride)
    parts = [(se3_inv(cams[oc[order[off[o]:off[o + 1]]]]), ob[order[off[o]:off[o + 1]]]) for o in sample]
    for Twc, boxes in parts[:20]:
        ctx.init_quadric(Twc, boxes, g.K, g.image_rows, g.image_cols, a.faithful)
    loop, worst = [], 0.0
    for _ in range(a.loop_passes):
        t0 = time.perf_counter()
        for Twc, boxes in parts:
            ctx.init_quadric(Twc, boxes, g.K, g.image_rows, g.image_cols, a.faithful)
        loop.append((time.perf_counter() - t0) * 1e3)
    for (Twc, boxes), o in zip(parts, sample):   # same answers, outside the timed window
        e1, _, ok1 = ctx.init_quadric(Twc, boxes, g.K, g.image_rows, g.image_cols, a.faithful)
        assert ok1 == (st[o, 0] == 0)
        if ok1:
            worst = max(worst, float(np.abs(e1 - ell[o]).max()))
    share = float(cnt[sample].sum() / cnt.sum())
    out["single_call_loop"] = dict(sampled_objects=int(len(sample)), sampled_share_of_observations=share, sample_ms=stats_of(loop),
                                   scaled_to_all_objects_ms=float(np.median(loop) / share),
                                   note="measured on the sample only and scaled by its share of the observations",
                                   max_abs_difference_of_ellipsoids=worst)
    out["ratio_loop_over_call"] = out["single_call_loop"]["scaled_to_all_objects_ms"] / out["call"]["ms_median"]
    out["ratio_loop_over_kernel"] = out["single_call_loop"]["scaled_to_all_objects_ms"] / out["kernel"]["ms_median"]
    ctx.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
