#!/usr/bin/env python3
"""Time esl_render_map on the 2,000-ellipsoid map of BASELINE configs[3] at 640 x 480:
  (a) one frame, all outputs;
  (b) 100 frames, cover + cmp only, against a synthetic depth;
  (c) the numpy statement (tests/render_ref.py) on (a)'s frame, on one core, as the comparison.

Recorded, not gated (profiles/render_c4.json, DESIGN.md "Rendering the map").  Two clocks, both after warm-up calls (buffers grown,
kernels loaded, clocks up), median / min / p90 over the timed calls: HIP events on the context's stream around the kernel launches
(esl_profile_enable(ctx, 2), kernel class 4), and the host clock around the C-ABI call, which adds the copies in and out.  The
prepare kernel is timed by a call that asks for the flags alone (it launches nothing else); the tile kernel is the difference.
The work model is computed from the shapes and the device's own flags: a record is tested by every pixel of every tile its
pixel bounds touch, 256 tests per (tile, record), 18 flops per test (esl_render_ray.hpp render_hit_terms: 11 for alpha, 4 for beta, 3
for Delta; the square root and the division only on a hit that can win).

    python scripts/render_bench.py --out profiles/render_c4.json
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

ROWS, COLS, TILE = 480, 640, 16
FLOPS_PER_TEST = 18
FP64_VECTOR_PEAK = 78.6e12


def stats_of(ms):
    ms = np.sort(np.asarray(ms))
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms[0]), ms_p90=float(ms[int(0.9 * (len(ms) - 1))]))


def timed(ctx, calls, warmup, fn):
    """(kernel ms per call, call ms per call, event brackets per call, the last result)"""
    for _ in range(warmup):
        fn()
    ctx.profile_enable(2)
    prev = ctx.profile_get().get("reduce", dict(count=0, total_ms=0.0))    # the counters run on: take differences
    kern, call, brackets, res = [], [], 0, None
    for _ in range(calls):
        res = fn()
        call.append(ctx.last_call_s * 1e3)
        pr = ctx.profile_get()["reduce"]
        kern.append(pr["total_ms"] - prev["total_ms"]); brackets = pr["count"] - prev["count"]
        prev = pr
    ctx.profile_enable(0)
    return kern, call, brackets, res


def records_per_tile(pkg, cams, objs, K, flags):
    """(frames, tiles) array-free tally: the (tile, record) pairs of the frames, from the device's flags and the outline's boxes"""
    F, M = flags.shape
    ci, oi = np.repeat(np.arange(F), M), np.tile(np.arange(M), F)
    bb, _, _ = pkg.synth.project_bboxes(cams, objs, K, ci, oi)
    bb = bb.reshape(F, M, 4)
    tx, ty = (COLS + TILE - 1) // TILE, (ROWS + TILE - 1) // TILE
    bounded = (flags & 8) != 0
    whole = ((flags & 1) != 0) & ~bounded
    with np.errstate(invalid="ignore"):
        x0 = np.maximum(np.floor(bb[..., 0]) - 1, 0); x1 = np.minimum(np.ceil(bb[..., 2]) + 1, COLS - 1)
        y0 = np.maximum(np.floor(bb[..., 1]) - 1, 0); y1 = np.minimum(np.ceil(bb[..., 3]) + 1, ROWS - 1)
        seen = bounded & (x0 <= x1) & (y0 <= y1)
        nx = np.where(seen, x1 // TILE - x0 // TILE + 1, 0); ny = np.where(seen, y1 // TILE - y0 // TILE + 1, 0)
    pairs = float((nx * ny).sum() + whole.sum() * tx * ty)
    return pairs, tx * ty, int(seen.sum()), int(whole.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true", help="skip (c), the numpy statement on one frame (about a minute)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    g, cams, objs, _ = pkg.synth.make_config("C4")
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7); objs = np.asarray(objs, dtype=np.float64).reshape(-1, 10)
    K = g.K
    ctx = pkg.Context(0)
    out = dict(config=dict(M=len(objs), rows=ROWS, cols=COLS, calls=a.calls, warmup=a.warmup, K=list(K)),
               timing="kernel: HIP events around the launches (esl_profile, class 4); call: host clock around the C-ABI call",
               model=dict(flops_per_test=FLOPS_PER_TEST, fp64_vector_peak=FP64_VECTOR_PEAK))
    rng = np.random.default_rng(0)
    for name, F, want, with_depth in (("one_frame", 1, ("depth", "inst", "cover", "flags"), True), ("frames", a.frames, ("cover",), True)):
        cf = cams[:F]
        depth = rng.integers(5000, 30000, size=(F, ROWS, COLS)).astype(np.uint16)          # 1 .. 6 m, no structure
        flags = ctx.render_map(cf, objs, K, ROWS, COLS, want=("flags",))["flags"]
        k_prep, _, _, _ = timed(ctx, a.calls, a.warmup, lambda: ctx.render_map(cf, objs, K, ROWS, COLS, want=("flags",)))
        kern, call, brackets, res = timed(ctx, a.calls, a.warmup, lambda: ctx.render_map(cf, objs, K, ROWS, COLS, depth, None, want))
        pairs, tiles, n_bounded, n_whole = records_per_tile(pkg, cf, objs, K, flags)
        tests = pairs * TILE * TILE
        prep_ms = float(np.median(k_prep))
        tile_ms = float(np.median(kern)) - prep_ms
        cover = res["cover"]
        out[name] = dict(frames=F, outputs=sorted(res), event_brackets_per_call=brackets, kernel=stats_of(kern), call=stats_of(call),
                         prepare_kernel_ms_median=prep_ms, tile_kernel_ms_median=tile_ms,
                         records_bounded=n_bounded, records_whole_image=n_whole, records_per_tile_mean=pairs / (F * tiles),
                         pixel_object_tests=tests, tests_per_s=tests / (tile_ms * 1e-3),
                         share_of_fp64_vector_peak=tests * FLOPS_PER_TEST / (tile_ms * 1e-3) / FP64_VECTOR_PEAK,
                         bytes_in=int(cf.nbytes + objs.nbytes + depth.nbytes), bytes_out=int(sum(v.nbytes for v in res.values())),
                         objects_hit=int((cover[..., 0] > 0).sum()), objects_seen=int((cover[..., 1] > 0).sum()),
                         pixels_won=int(cover[..., 1].sum()), cmp_totals=[int(v) for v in res["cmp"].sum((0, 1))])
        print(name, json.dumps(out[name]), flush=True)
        if name == "one_frame" and not a.no_numpy:
            import render_ref as rr
            t0 = time.perf_counter()
            ref = rr.render(cf, objs, K, ROWS, COLS, depth, margins=False)
            secs = time.perf_counter() - t0
            fin = ~np.isnan(ref["depth"])
            out["numpy_one_frame"] = dict(seconds=secs, inst_equal=bool(np.array_equal(ref["inst"], res["inst"])),
                                          cover_equal=bool(np.array_equal(ref["cover"], res["cover"])),
                                          cmp_equal=bool(np.array_equal(ref["cmp"], res["cmp"])),
                                          flags_equal=bool(np.array_equal(ref["flags"], res["flags"])),
                                          nan_equal=bool(np.array_equal(fin, ~np.isnan(res["depth"]))),
                                          depth_max_abs_diff=float(np.abs(ref["depth"][fin] - res["depth"][fin]).max()) if fin.any() else 0.0,
                                          smallest_margins={k: float(v) for k, v in ref["margins"].items()})
            print("numpy_one_frame", json.dumps(out["numpy_one_frame"]), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
