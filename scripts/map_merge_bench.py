#!/usr/bin/env python3
"""Time esl_map_merge on the map of BASELINE configs[3] (synth.make_config("C4"): 2,000 ellipsoids, 200,000 boxes) with 15 % of the
ellipsoids planted a second time.

A planted copy has its centre moved by up to 10 % of the smallest half-axis, its axes changed by +-10 % and its yaw by +-10 degrees; it
stands behind the originals and takes a random half of its original's list entries.  Labels: 20 classes, a copy has its original's.

Recorded, not gated (profiles/map_merge_c4.json, DESIGN.md "Map maintenance").  All clocks after warm-up calls (buffers grown, kernels
loaded, clocks up), median / min / p90 over the timed calls, once with the labels matched and once with match_labels = 0:
  kernel  HIP events on the context's stream around the launches (esl_profile_enable(ctx, 2), kernel class 4), summed over the call's
          brackets: the host's waits between them (candidate count, component rounds) are not in it
  call    the host clock around the C-ABI call: adds the copies of the map and the list in and of the results out, the argument
          checks over the list, and every synchronise

    python scripts/map_merge_bench.py --out profiles/map_merge_c4.json
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats_of(ms):
    ms = np.sort(np.asarray(ms))
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms[0]), ms_p90=float(ms[int(0.9 * (len(ms) - 1))]))


def yaw_quat(q, dyaw):
    """q (x, y, z, w) turned by dyaw about the world's z axis"""
    x, y, z, w = q
    s, c = np.sin(dyaw / 2), np.cos(dyaw / 2)
    return np.array([c * x - s * y, c * y + s * x, c * z + s * w, c * w - s * z])


def plant(objs, obs_obj, share, n_labels, rng):
    N = len(objs)
    copy_of = np.sort(rng.choice(N, int(round(share * N)), replace=False))
    copies = []
    for o in copy_of:
        v = objs[o].copy()
        smin = np.abs(v[7:]).min()
        d = rng.normal(size=3)
        v[:3] += d / np.linalg.norm(d) * rng.uniform(0, 0.1) * smin
        v[3:7] = yaw_quat(v[3:7], np.deg2rad(rng.uniform(-10, 10)))
        v[7:] *= rng.uniform(0.9, 1.1, 3)
        copies.append(v)
    labels = rng.integers(0, n_labels, N).astype(np.int32)
    index_of_copy = np.full(N, -1)
    index_of_copy[copy_of] = N + np.arange(len(copy_of))
    obj = obs_obj.copy()
    move = (index_of_copy[obs_obj] >= 0) & (rng.random(len(obs_obj)) < 0.5)
    obj[move] = index_of_copy[obs_obj[move]]
    identity = np.concatenate([np.arange(N), copy_of])
    return np.concatenate([objs, np.array(copies)]), np.concatenate([labels, labels[copy_of]]), obj.astype(np.int32), copy_of, identity


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--share", type=float, default=0.15)
    ap.add_argument("--labels", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    g, _, objs, _ = pkg.synth.make_config(a.config)
    objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    N = len(objs)
    rng = np.random.default_rng(a.seed)
    cam = np.asarray(g.bbox_cam, np.int32)
    mobjs, labels, obj, copy_of, identity = plant(objs, np.asarray(g.bbox_obj, np.int32), a.share, a.labels, rng)
    ctx = pkg.Context(0)
    out = dict(config=dict(name=a.config, objects=int(N), planted_copies=int(len(copy_of)), map=int(len(mobjs)), list_entries=int(len(obj)),
                           frames=int(g.n_cams), labels=a.labels, calls=a.calls, warmup=a.warmup, seed=a.seed),
               timing="kernel: HIP events around the launches (esl_profile, class 4), summed over a call's brackets; call: host clock "
                      "around the C-ABI call")
    for name, match in (("labels_matched", 1), ("labels_ignored", 0)):
        p = pkg.abi.default_merge_params(match_labels=match)
        for _ in range(a.warmup):
            ctx.map_merge(mobjs, labels, None, cam, obj, p)
        call = []
        for _ in range(a.calls):          # profiler off: the call as a user times it
            r = ctx.map_merge(mobjs, labels, None, cam, obj, p)
            call.append(ctx.last_call_s * 1e3)
        ctx.profile_enable(2)
        prev = ctx.profile_get().get("reduce", dict(count=0, total_ms=0.0))    # the counters run on: take differences
        kern, brackets = [], 0
        for _ in range(a.calls):
            ctx.map_merge(mobjs, labels, None, cam, obj, p)
            pr = ctx.profile_get()["reduce"]
            kern.append(pr["total_ms"] - prev["total_ms"]); brackets = pr["count"] - prev["count"]
            prev = pr
        ctx.profile_enable(0)
        group = r["group"]
        recovered = int((group[N:] == group[copy_of]).sum())
        # a false group joins two different objects of the map as it was before the planting
        false_groups = sum(1 for gid in np.unique(group) if len(np.unique(identity[group == gid])) > 1)
        live = r["obs_obj"] >= 0
        out[name] = dict(result=r["result"], planted_pairs_recovered=recovered, planted_pairs=int(len(copy_of)), false_groups=int(false_groups),
                         list_entries_kept=int(live.sum()), event_brackets_per_call=int(brackets), kernel=stats_of(kern), call=stats_of(call))
    ctx.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
