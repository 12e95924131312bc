#!/usr/bin/env python3
"""Time esl_associate_boxes at the shape of BASELINE configs[3] -- 10,000 frames x 2,000 ellipsoids x 20 detections per frame -- and at
one frame x 2,000 ellipsoids x 20 detections.

Recorded, not gated (profiles/assoc_c4.json, DESIGN.md "2-D data association").  Two clocks, both after warm-up calls (buffers grown,
kernel loaded, clocks up), median / min / p90 over the timed calls: HIP events on the context's stream around the kernel launches
(esl_profile_enable(ctx, 2), kernel class 4), and the host clock around the C-ABI call, which adds the copies of the poses, the map and
the detections in and of the results out.

    python scripts/assoc_bench.py --out profiles/assoc_c4.json
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, ROWS, COLS = (525.0, 525.0, 319.5, 239.5), 480, 640


def scene(F, M, D, n_labels, seed, half=20.0):
    """M ellipsoids standing on z = 0 in a room of 2 half x 2 half metres, F cameras 1.2 m up anywhere in it looking level in a random
    direction; D detections per frame: boxes around the projected centres of D objects in front of the camera (centre inside the
    image, 1.5 to 6 m away), sized from the mean half-axis, moved by up to 3 px"""
    import assoc2d_ref as ar
    import assoc2d_scenes as sc
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.15, 0.6, size=(M, 3))
    yaw = rng.uniform(-np.pi, np.pi, size=M)
    objs = np.zeros((M, 10))
    objs[:, :2] = rng.uniform(-half, half, size=(M, 2)); objs[:, 2] = s[:, 2]
    objs[:, 5] = np.sin(yaw / 2); objs[:, 6] = np.cos(yaw / 2); objs[:, 7:10] = s
    labels = rng.integers(0, n_labels, M).astype(np.int32)
    cams = np.zeros((F, 7)); off = [0]; boxes = []; labs = []
    r_mean = s.mean(axis=1)
    for f in range(F):
        pos = np.array([rng.uniform(-half, half), rng.uniform(-half, half), 1.2])
        a = rng.uniform(-np.pi, np.pi)
        cams[f] = sc.look_at(pos, pos + [np.cos(a), np.sin(a), -0.1])
        Tc = ar.pose_matrix(cams[f])
        pc = objs[:, :3] @ Tc[:3, :3].T + Tc[:3, 3]
        z = np.where(pc[:, 2] > 0, pc[:, 2], np.inf)
        u, v = K[0] * pc[:, 0] / z + K[2], K[1] * pc[:, 1] / z + K[3]
        ok = np.nonzero((pc[:, 2] > 1.5) & (pc[:, 2] < 6) & (u > 0) & (u < COLS) & (v > 0) & (v < ROWS))[0]
        pick = rng.choice(ok, size=min(D, len(ok)), replace=False)
        h = K[0] * r_mean[pick] / pc[pick, 2]
        b = np.stack([u[pick] - h, v[pick] - h, u[pick] + h, v[pick] + h], axis=1) + rng.uniform(-3, 3, size=(len(pick), 4))
        boxes.append(b); labs.append(labels[pick]); off.append(off[-1] + len(pick))
    return dict(cams=cams, objs=objs, obj_labels=labels, det_offsets=np.array(off, np.int32), det_boxes=np.concatenate(boxes).reshape(-1, 4),
                det_labels=np.concatenate(labs).astype(np.int32))


def stats_of(ms):
    ms = np.sort(np.asarray(ms))
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms[0]), ms_p90=float(ms[int(0.9 * (len(ms) - 1))]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--objects", type=int, default=2000)
    ap.add_argument("--detections", type=int, default=20)
    ap.add_argument("--labels", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    ctx = pkg.Context(0)
    out = dict(config=dict(M=a.objects, D=a.detections, labels=a.labels, calls=a.calls, warmup=a.warmup),
               timing="kernel: HIP events around the launches (esl_profile, class 4); call: host clock around the C-ABI call")
    for name, F in (("c4", a.frames), ("one_frame", 1)):
        sc = scene(F, a.objects, a.detections, a.labels, seed=0)
        args = (sc["cams"], sc["objs"], sc["obj_labels"], K, ROWS, COLS, sc["det_offsets"], sc["det_boxes"], sc["det_labels"])
        for _ in range(a.warmup):
            ctx.associate_boxes(*args)
        ctx.profile_enable(2)
        prev = ctx.profile_get().get("reduce", dict(count=0, total_ms=0.0))    # the counters run on: take differences
        kern, call, launches = [], [], 0
        for _ in range(a.calls):
            assoc, iou, st = ctx.associate_boxes(*args)
            call.append(ctx.last_call_s * 1e3)
            pr = ctx.profile_get()["reduce"]
            kern.append(pr["total_ms"] - prev["total_ms"]); launches = pr["count"] - prev["count"]
            prev = pr
        ctx.profile_enable(0)
        out[name] = dict(frames=F, detections=int(len(assoc)), assigned=int((assoc >= 0).sum()), event_brackets_per_call=launches,
                         eligible_per_frame=float(st[:, 0].mean()), occluded_per_frame=float(st[:, 1].mean()), spilled_frames=int(st[:, 3].sum()),
                         kernel=stats_of(kern), call=stats_of(call))
        print(name, json.dumps(out[name]))
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
