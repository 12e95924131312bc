#!/usr/bin/env python3
"""Time esl_dense_carve_frames on the synthetic room of scripts/dense_map_bench.py (100 frames of 640 x 480, leaf 0.01): a box is planted
in the depth of the first 40 frames, the map is built from all frames, the last 60 frames observe and all frames own.

Recorded, not gated (profiles/dense_carve_c4.json, DESIGN.md "Carving the dense map"): there is no earlier implementation, the parent
cannot run the call.  Two clocks, medians of --calls calls after a warm-up call: HIP events on the context's stream around the launches
(esl_profile_enable(ctx, 2), kernel class 4) and the host clock around the C-ABI call, which adds the uploads and the copies of the
outputs.  The class-4 brackets hold whole groups of launches, so the split is taken by differences of three calls with apply = 0:
  list + gather + verdict            F_obs = 0, F_own = 0
  + observe                          F_obs = 60, F_own = 0
  + mark                             F_obs = 0, F_own = 100 (nothing is carved: the mark pass runs its lookups all the same)
and the removal as the call with apply = 1 (the map rebuilt before every call) less the call with apply = 0.  Beside them, asserted
nowhere: the numpy statement (tests/dense_carve_ref.py) on a cut of the voxels and one frame, scaled; esl_dense_render and
esl_dense_remove_frames on the same map and frames, measured in the same run; whether the carved map equals the map built from scratch
from the kept images.
    python scripts/dense_carve_bench.py --out profiles/dense_carve_c4.json
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import dense_map_bench as dmb          # noqa: E402

ROWS, COLS, K = dmb.ROWS, dmb.COLS, dmb.K
EXTRACT = ("key", "xyz", "count", "bgr", "inst", "votes")


def plant_box(cams, depth, inst, n_box, view):
    """a 0.4 x 1.0 x 0.4 m box on the floor (+y), 1.5 m in front of frame `view`, drawn into the depth of the first n_box frames"""
    import dense_carve_scenes as cs
    import dense_ref as dr
    R, t = dr.pose(cams[view])
    c = -R.T @ t + 1.5 * R[2]          # the camera centre plus 1.5 m along its forward axis
    lo = np.array([c[0] - 0.2, dmb.HALF[1] - 1.0, c[2] - 0.2]) + 0.003
    hi = lo + np.array([0.4, 1.0, 0.4])
    hit = np.zeros(depth.shape, bool)
    for f in range(n_box):
        zb = cs.box_hit(cams[f], K, ROWS, COLS, lo, hi)
        raw = np.clip(np.rint(np.where(np.isfinite(zb), zb, 0.0) * 5000.0), 1, 65535).astype(np.uint16)
        hit[f] = np.isfinite(zb) & (raw < depth[f])
        depth[f] = np.where(hit[f], raw, depth[f])
        inst[f] = np.where(hit[f], 7, inst[f])
    return hit


def build_map(pkg, ctx, cams, depth, bgr, inst, max_voxels):
    ctx.dense_begin(pkg.abi.default_dense_params(max_voxels=max_voxels))
    return ctx.dense_add_frames(cams, K, ROWS, COLS, depth, bgr, inst)


def kernel_ms(ctx, prev):
    pr = ctx.profile_get()["reduce"]
    return pr["total_ms"] - prev["total_ms"], pr


def timed(ctx, calls, fn, before=None):
    """warm-up, then `calls` calls: medians of the kernel time (class 4 brackets) and of the call time; the last result.  before: run
    ahead of every call, outside both clocks"""
    if before:
        before()
    first = fn()
    ctx.profile_enable(2)
    rec = dict(kernel=[], call=[])
    res = first
    for _ in range(calls):
        if before:
            before()
        prev = ctx.profile_get().get("reduce", dict(count=0, total_ms=0.0))
        res = fn()
        rec["call"].append(ctx.last_call_s * 1e3)
        rec["kernel"].append(kernel_ms(ctx, prev)[0])
    ctx.profile_enable(0)
    same = all(first[k].tobytes() == res[k].tobytes() for k in first if hasattr(first[k], "tobytes"))
    return dict({k: dmb.stats_of(v) for k, v in rec.items()}, runs_bit_identical=bool(same)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--box-frames", type=int, default=40)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    ap.add_argument("--numpy-voxels", type=int, default=20000, help="0: skip the numpy statement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    ctx = pkg.Context(0)
    t0 = time.perf_counter()
    cams, depth, bgr, inst = dmb.room_frames(a.frames)
    nb = min(a.box_frames, a.frames)
    hit = plant_box(cams, depth, inst, nb, min(2, nb - 1))          # in front of frame 2: the last frames of the turn look there again
    print(f"scene built in {time.perf_counter() - t0:.1f} s; box pixels {int(hit.sum())}", flush=True)
    F = len(cams)
    obs = slice(nb, F)
    Fo = F - nb
    P = pkg.abi.default_dense_carve_params
    rebuild = lambda: build_map(pkg, ctx, cams, depth, bgr, inst, a.max_voxels)          # noqa: E731
    add = rebuild()
    info = ctx.dense_info()
    n = info["n_voxels"]
    none = (np.zeros((0, 7)), np.zeros((0, ROWS, COLS), np.uint16))
    out = dict(config=dict(frames=F, box_frames=nb, observers=Fo, owners=F, rows=ROWS, cols=COLS, leaf=0.01, max_voxels=a.max_voxels, calls=a.calls,
                           params="defaults", box_pixels=int(hit.sum())),
               timing="kernel: HIP events around the launches (esl_profile, class 4); call: host clock around the C-ABI call",
               map=dict(add_result=add, info=info),
               not_measured=["real sequences: the room is synthetic", "leaves other than 0.01 m", "hardware counters of k_dcv_observe and k_dcv_mark",
                             "a cull of the voxels outside every observer's frustum ahead of the observe pass: not built",
                             "windows other than the default", "the add path: esl_dense.hip's kernels are not edited"])

    def carve(o, w, apply=0, want=("vox", "carved", "obs", "own")):
        co, do = (cams[o], depth[o]) if o is not None else none
        cw, dw, bw, iw = (cams, depth, bgr, inst) if w else (none[0], none[1], None, None)
        return ctx.dense_carve_frames(co, do, cw, dw, K, ROWS, COLS, bw, iw, P(apply=apply), want=want)
    runs = [("list_gather_verdict", None, False), ("observers_only", obs, False), ("owners_only", None, True), ("apply_0", obs, True)]
    for name, o, w in runs:
        t, res = timed(ctx, a.calls, lambda: carve(o, w))
        out[name] = dict(t, result=res["result"])
        print(name, json.dumps(out[name]), flush=True)
    t, res = timed(ctx, a.calls, lambda: carve(obs, True, want=("vox", "carved", "obs", "own", "depth_kept", "mask")))
    out["apply_0_with_images"] = dict(t, result=res["result"])
    t, res1 = timed(ctx, a.calls, lambda: carve(obs, True, apply=1, want=("vox", "carved", "obs", "own", "depth_kept")), before=rebuild)
    out["apply_1"] = dict(t, result=res1["result"], note="the map is rebuilt ahead of every call, outside both clocks")
    print("apply_1", json.dumps(out["apply_1"]), flush=True)
    k = {name: out[name]["kernel"]["ms_median"] for name in ("list_gather_verdict", "observers_only", "owners_only", "apply_0", "apply_1")}
    observe_ms = k["observers_only"] - k["list_gather_verdict"]
    out["split_kernel_ms"] = dict(list_gather_verdict=k["list_gather_verdict"], observe=observe_ms, mark=k["owners_only"] - k["list_gather_verdict"],
                                  removal=k["apply_1"] - k["apply_0"], how="differences of the medians above")
    out["voxel_frame_tests_per_s"] = dict(tests=n * Fo, of_observe_kernel_time=n * Fo / (observe_ms * 1e-3) if observe_ms > 0 else None,
                                          of_apply_0_call_time=n * Fo / (out["apply_0"]["call"]["ms_median"] * 1e-3))
    print("split", json.dumps(out["split_kernel_ms"]), json.dumps(out["voxel_frame_tests_per_s"]), flush=True)
    # the carved map against the map built from scratch from the kept images
    carved_map = ctx.dense_extract()
    carved_info = ctx.dense_info()
    build_map(pkg, ctx, cams, res1["depth_kept"], bgr, inst, a.max_voxels)
    fresh = ctx.dense_extract()
    out["carved_map_equals_map_of_kept_images"] = bool(carved_map["n_voxels"] == fresh["n_voxels"] and carved_info == ctx.dense_info()
                                                       and all(carved_map[x].tobytes() == fresh[x].tobytes() for x in EXTRACT))
    # yardsticks, measured in this run on the same map and frames
    rebuild()
    t, _ = timed(ctx, a.calls, lambda: ctx.dense_render(cams, K, ROWS, COLS, depth, want=("frame", "vox")))
    out["yardstick_esl_dense_render_all_frames_counts"] = t

    def remove_all():
        r = ctx.dense_remove_frames(cams, K, ROWS, COLS, depth, bgr, inst)
        return dict(n_used=np.array([r["n_used"]]))
    t, _ = timed(ctx, a.calls, remove_all, before=rebuild)
    out["yardstick_esl_dense_remove_frames_all_frames"] = t
    if a.numpy_voxels > 0:
        import dense_carve_ref as dcr
        rebuild()
        ext = ctx.dense_extract(want=("xyz",))
        cut = slice(0, n, max(1, n // a.numpy_voxels))          # an even cut of the list: in view as often as the whole map is
        xyz = np.ascontiguousarray(ext["xyz"][cut])
        m = len(xyz)
        t0 = time.perf_counter()
        cls = dcr.observe(xyz, cams[nb], K, ROWS, COLS, depth[nb], dcr.DEFAULTS)
        secs = time.perf_counter() - t0
        one = ctx.dense_carve_frames(cams[nb:nb + 1], depth[nb:nb + 1], None, None, K, ROWS, COLS, want=("vox",))
        want = np.stack([(cls == c) for c in range(4)], axis=-1).astype(np.int32)
        out["numpy_statement"] = dict(voxels=m, frames=1, in_view=int((cls <= dcr.NODATA).sum()), seconds=secs, tests_per_s=m / secs,
                                      scaled_to_the_call_s=n * Fo / (m / secs), equal=bool(np.array_equal(one["vox"][cut], want)))
        print("numpy_statement", json.dumps(out["numpy_statement"]), flush=True)
    ctx.close()
    print("RESULT " + json.dumps({x: out[x] for x in ("split_kernel_ms", "voxel_frame_tests_per_s", "carved_map_equals_map_of_kept_images")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
