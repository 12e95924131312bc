#!/usr/bin/env python3
"""Time esl_init_quadrics_robust on BASELINE configs[3] (synth.make_config("C4"): 10,000 frames, 2,000 ellipsoids, 200,000 boxes) with
outlier boxes planted as tests/init_robust_ref.plant does (15 % of the boxes of every object of >= 15 observations moved 40-80 px),
default parameters, warm calls, beside the plain esl_init_quadrics on the same list.

Recorded, not gated (profiles/init_robust_c4.json, DESIGN.md "Consensus SVD initialisation").  Clocks as scripts/init_batch_bench.py:
  kernel  HIP events on the context's stream around the launches (esl_profile_enable(ctx, 2), kernel class 4), summed over a call
  call    the host clock around the C-ABI call
Stages.  The three passes are one kernel, so the profile's class total cannot tell them apart; they are separated by calls:
  hypotheses + winner   the kernel time of the call with refine = 0 (the winner pass is one more fit and score per object)
  refit                 the kernel time of esl_init_quadrics on the list with everything but the final winners' inliers skipped
  re-score              the kernel time of the full call minus the two above
The numpy statement (tests/init_robust_ref.reference) is timed on --ref-objects objects and scaled by their share of the observations.

    python scripts/init_robust_bench.py --out profiles/init_robust_c4.json
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


def stats_of(ms):
    ms = np.sort(np.asarray(ms))
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms[0]), ms_p90=float(ms[int(0.9 * (len(ms) - 1))]))


def timed(ctx, fn, calls):
    """(host ms per call, kernel ms per call, event brackets per call, last result)"""
    host, kern, brackets, out = [], [], 0, None
    for _ in range(calls):
        out = fn()
        host.append(ctx.last_call_s * 1e3)
    ctx.profile_enable(2)
    prev = ctx.profile_get().get("reduce", dict(count=0, total_ms=0.0))    # the counters run on: take differences
    for _ in range(calls):
        fn()
        pr = ctx.profile_get()["reduce"]
        kern.append(pr["total_ms"] - prev["total_ms"]); brackets = pr["count"] - prev["count"]
        prev = pr
    ctx.profile_enable(0)
    return stats_of(host), stats_of(kern), int(brackets), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--faithful", type=int, default=0)
    ap.add_argument("--ref-objects", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    import init_robust_ref as rr
    g, cams, _, _ = pkg.synth.make_config(a.config)
    N = g.n_objs
    s = rr.plant(dict(cams=cams, N=N, obs_cam=np.asarray(g.bbox_cam, np.int32), obs_obj=np.asarray(g.bbox_obj, np.int32),
                      obs_boxes=np.ascontiguousarray(g.bbox_meas, dtype=np.float64), K=g.K), np.random.default_rng(0))
    oc, oo, ob, planted = s["obs_cam"], s["obs_obj"], s["obs_boxes"], s["planted"]
    cnt = np.bincount(oo, minlength=N)
    ctx = pkg.Context(0)
    kw = dict(rows=g.image_rows, cols=g.image_cols, faithful=a.faithful)
    P = pkg.abi.default_init_robust_params

    def robust(**p):
        return lambda: ctx.init_quadrics_robust(cams, N, oc, oo, ob, g.K, params=P(**p), **kw)

    def plain(obj):
        return lambda: ctx.init_quadrics(cams, N, oc, obj, ob, g.K, **kw)
    for _ in range(a.warmup):
        robust()(); robust(refine=0)(); plain(oo)()
    full_call, full_kern, full_br, out = timed(ctx, robust(), a.calls)
    hw_call, hw_kern, hw_br, _ = timed(ctx, robust(refine=0), a.calls)
    plain_call, plain_kern, plain_br, pl = timed(ctx, plain(oo), a.calls)
    unre = robust(refine=0)()
    masked = np.where((unre["inliers"] == 1), oo, -1).astype(np.int32)
    refit_call, refit_kern, _, _ = timed(ctx, plain(masked), a.calls)
    st = out["stats"]
    has = np.bincount(oo[planted], minlength=N) > 0
    exact = int(sum(1 for o in np.nonzero(has)[0] if st[o, 0] == 0 and np.array_equal(out["inliers"][oo == o] == 1, ~planted[oo == o])))
    res = dict(config=dict(name=a.config, frames=int(g.n_cams), objects=int(N), observations=int(len(oo)), planted_boxes=int(planted.sum()),
                           planted_objects=int(has.sum()), faithful=a.faithful, calls=a.calls, warmup=a.warmup,
                           params=dict(sample_size=5, n_hypotheses=64, inlier_px=10.0, min_inliers=8, refine=1, seed=0)),
               timing="kernel: HIP events around the launches (esl_profile, class 4), summed over a call; call: host clock around the C-ABI call",
               observations_per_object=dict(min=int(cnt.min()), median=float(np.median(cnt)), max=int(cnt.max())),
               robust=dict(call=full_call, kernel=full_kern, event_brackets_per_call=full_br,
                           status_counts=[int((st[:, 0] == k).sum()) for k in range(6)], refined=int(st[:, 7].sum()),
                           spilled=int(st[:, 3].sum()), planted_objects_recovered_exactly=exact),
               robust_without_refine=dict(call=hw_call, kernel=hw_kern, event_brackets_per_call=hw_br),
               plain=dict(call=plain_call, kernel=plain_kern, event_brackets_per_call=plain_br,
                          status_counts=[int((pl[3][:, 0] == k).sum()) for k in range(4)]),
               stages_kernel_ms_median=dict(hypotheses_and_winner=hw_kern["ms_median"], refit=refit_kern["ms_median"],
                                            rescore=full_kern["ms_median"] - hw_kern["ms_median"] - refit_kern["ms_median"],
                                            note="one kernel runs all three passes: the stages are separated by calls (see the script's header)"),
               initialised=dict(plain=int((pl[3][:, 0] == 0).sum()), robust=int((st[:, 0] == 0).sum())))
    # the numpy statement on a few objects, scaled
    sample = np.arange(0, N, max(1, N // a.ref_objects))[:a.ref_objects]
    keep = np.isin(oo, sample)
    remap = np.full(N, -1, np.int32); remap[sample] = np.arange(len(sample), dtype=np.int32)
    t0 = time.perf_counter()
    ref = rr.reference(cams, len(sample), oc[keep], remap[oo[keep]], ob[keep], g.K, g.image_rows, g.image_cols, faithful=a.faithful)
    ref_s = time.perf_counter() - t0
    share = float(keep.sum() / len(oo))
    same = int(sum(np.array_equal(ref["inliers"][remap[oo[keep]] == j], out["inliers"][oo == o]) for j, o in enumerate(sample)))
    res["reference"] = dict(sampled_objects=int(len(sample)), sampled_share_of_observations=share, sample_s=ref_s,
                            scaled_to_all_objects_s=ref_s / share, objects_with_the_device_inlier_set=same,
                            note="measured on the sample only and scaled by its share of the observations")
    ctx.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
