#!/usr/bin/env python3
"""Time esl_dense_covis_frames on the synthetic room of scripts/dense_map_bench.py (100 frames of 640 x 480, leaf 0.01): the map is built
from all frames, then the first F of them are related through it.

Recorded, not gated (profiles/dense_covis_c4.json, DESIGN.md "Covisibility of the dense map"): there is no earlier implementation, the
parent cannot run the call.  Two clocks as in scripts/dense_carve_bench.py (its `timed`), medians of --calls calls after a warm-up
call: HIP events around the launches (esl_profile_enable(ctx, 2), kernel class 4) and the host clock around the C-ABI call, which adds
the upload of the depth images and the copies of the outputs.  Calls: F = 1, 10 and 100 with every output; F = 100 without pair_out (the
pair kernel does not run); F = 0 (the list and the gather alone); F = 100 with max_cull = 100.  The class-4 brackets hold whole groups
of launches, so the split is taken by differences of the medians:
  list + gather                      F = 0
  observe + mask + cover             F = 100 without pairs, less F = 0
  pairs                              F = 100 with pairs, less without
  cull rounds                        F = 100 with max_cull = 100, less with max_cull = 0
Beside them, asserted nowhere: the numpy statement (tests/dense_covis_ref.py's parts) on a cut of the voxels, scaled.
    python scripts/dense_covis_bench.py --out profiles/dense_covis_c4.json
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

import dense_carve_bench as dcb        # noqa: E402
import dense_map_bench as dmb          # noqa: E402

ROWS, COLS, K = dmb.ROWS, dmb.COLS, dmb.K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    ap.add_argument("--numpy-voxels", type=int, default=20000, help="0: skip the numpy statement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    ctx = pkg.Context(0)
    t0 = time.perf_counter()
    cams, depth, bgr, inst = dmb.room_frames(a.frames)
    print(f"scene built in {time.perf_counter() - t0:.1f} s", flush=True)
    F = len(cams)
    add = dcb.build_map(pkg, ctx, cams, depth, bgr, inst, a.max_voxels)
    info = ctx.dense_info()
    n = info["n_voxels"]
    P = pkg.abi.default_dense_covis_params
    out = dict(config=dict(frames=F, rows=ROWS, cols=COLS, leaf=0.01, max_voxels=a.max_voxels, calls=a.calls, params="defaults", words_per_row=(n + 63) // 64),
               timing="kernel: HIP events around the launches (esl_profile, class 4); call: host clock around the C-ABI call",
               map=dict(add_result=add, info=info),
               not_measured=["real sequences: the room is synthetic", "leaves other than 0.01 m", "F beyond 100: the pair kernel's tiles number F F / 2048",
                             "hardware counters of k_dco_observe and k_dco_pairs (LDS bank conflicts among them)",
                             "other tile edges, slab lengths and register blockings of k_dco_pairs", "windows other than the default",
                             "a per-voxel observer list with one atomic per pair: not built"])

    def covis(Fc, want=("vox", "frame", "pair"), **kw):
        return ctx.dense_covis_frames(cams[:Fc], depth[:Fc], K, ROWS, COLS, params=P(**kw), want=want)
    runs = [("frames_0", 0, ("vox", "frame"), {}), ("frames_1", min(1, F), ("vox", "frame", "pair"), {}), ("frames_10", min(10, F), ("vox", "frame", "pair"), {}),
            ("frames_100", F, ("vox", "frame", "pair"), {}), ("frames_100_no_pairs", F, ("vox", "frame"), {}),
            ("frames_100_max_cull_100", F, ("vox", "frame", "pair"), dict(max_cull=100))]
    last = {}
    for name, Fc, want, kw in runs:
        t, res = dcb.timed(ctx, a.calls, lambda: covis(Fc, want, **kw))
        out[name] = dict(t, frames=Fc, result=res["result"])
        last[name] = res
        print(name, json.dumps(out[name]), flush=True)
    full = last["frames_100"]
    k = {name: out[name]["kernel"]["ms_median"] for name, _, _, _ in runs}
    pairs_ms = k["frames_100"] - k["frames_100_no_pairs"]
    observe_ms = k["frames_100_no_pairs"] - k["frames_0"]
    culled = out["frames_100_max_cull_100"]["result"]["n_culled"]
    W = (n + 63) // 64
    out["split_kernel_ms"] = dict(list_gather=k["frames_0"], observe_mask_cover=observe_ms, pairs=pairs_ms,
                                  cull_rounds=k["frames_100_max_cull_100"] - k["frames_100"], rounds=culled, how="differences of the medians above")
    out["rates"] = dict(voxel_frame_tests=n * F, tests_per_s_of_observe=n * F / (observe_ms * 1e-3) if observe_ms > 0 else None,
                        word_pairs=F * (F + 1) // 2 * W, word_pairs_per_s_of_pairs=F * (F + 1) // 2 * W / (pairs_ms * 1e-3) if pairs_ms > 0 else None,
                        cull_round_call_ms=((out["frames_100_max_cull_100"]["call"]["ms_median"] - out["frames_100"]["call"]["ms_median"]) / culled) if culled else None)
    out["graph"] = dict(pairs_nonzero=int((np.triu(full["pair"], 1) > 0).sum()), pairs_total=F * (F - 1) // 2, seen_min=int(full["frame"][:, 3].min()),
                        seen_max=int(full["frame"][:, 3].max()), k_max=int(full["vox"].max()), k_mean=float(full["vox"].mean()),
                        redundant_at_defaults=int(sum(1 for s, c in full["frame"][:, 3:5].tolist() if s >= 1 and c * 10 >= 9 * s)),
                        culled_at_max_cull_100=culled)
    print("split", json.dumps(out["split_kernel_ms"]), json.dumps(out["rates"]), json.dumps(out["graph"]), flush=True)
    if a.numpy_voxels > 0:
        import dense_carve_ref as dcr
        import dense_covis_ref as dco
        ext = ctx.dense_extract(want=("xyz",))
        cut = slice(0, n, max(1, n // a.numpy_voxels))          # an even cut of the list: in view as often as the whole map is
        xyz = np.ascontiguousarray(ext["xyz"][cut])
        m, Fn = len(xyz), min(10, F)
        p = dict(dco.DEFAULTS)
        t0 = time.perf_counter()
        B = np.stack([dcr.observe(xyz, cams[f], K, ROWS, COLS, depth[f], p) == dcr.AGREE for f in range(Fn)])
        t_obs = time.perf_counter() - t0
        t0 = time.perf_counter()
        Bi = B.astype(np.int64)
        pair = Bi @ Bi.T
        t_pair = time.perf_counter() - t0
        ten = last["frames_10"] if Fn == 10 else covis(Fn)
        # on the cut the device's k of the same frames: equal bits give equal column sums
        out["numpy_statement"] = dict(voxels=m, frames=Fn, observe_seconds=t_obs, tests_per_s=m * Fn / t_obs, pair_product_seconds=t_pair,
                                      scaled_to_100_frames_s=dict(observe=n * F / (m * Fn / t_obs), pairs=t_pair * (n / m) * (F / Fn) ** 2),
                                      k_equal_on_the_cut=bool(np.array_equal(ten["vox"][cut], B.sum(axis=0))),
                                      pair_diagonal_at_most_the_call_s=bool((np.diag(pair) <= np.diag(ten["pair"])).all()))
        print("numpy_statement", json.dumps(out["numpy_statement"]), flush=True)
    ctx.close()
    print("RESULT " + json.dumps({x: out[x] for x in ("split_kernel_ms", "rates", "graph")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
