#!/usr/bin/env python3
"""Time esl_dense_objects on the synthetic room of scripts/dense_map_bench.py (100 frames of 640 x 480, leaf 0.01) with four tall ellipsoids
standing on its floor: their pixels carry esl_render_map's labels 0 .. 3, the walls the labels 4 .. 9 (the floor none), so the map holds
small objects and very large instances side by side.  Run for reach 1, 2 and 3.

Recorded, not gated (profiles/dense_objects_c4.json, DESIGN.md "Per-instance ellipsoids from the dense map"): there is no earlier
implementation to compare with.  Two clocks, medians of --calls calls after a warm-up call: HIP events on the context's stream around the
launches (esl_profile_enable(ctx, 2), kernel class 4: three brackets per call, the sorted list included) and the host clock around
the C-ABI call, which adds the three host round trips, the table's sort and the copies out.  Beside them: the component counts, the time
to read the voxel and pair tables once at the measured HBM rate, and the numpy statement (tests/dense_objects_ref.py) on the map of
the first frames, scaled by the number of voxels.  The profile's brackets are per class, not per kernel: the split per launch comes from
a second run of this script under the profiler, whose per-kernel table is merged into the record with --kernel-stats.

    rocprofv3 --kernel-trace --stats --output-format csv -d prof -- python scripts/dense_objects_bench.py --reaches 2 --numpy-frames 0
    python scripts/dense_objects_bench.py --kernel-stats prof/*/*_kernel_stats.csv --out profiles/dense_objects_c4.json
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
FLOOR_Y = float(dmb.HALF[1])
GROUND = (0.0, -1.0, 0.0, FLOOR_Y)          # the room's +y is down: height = FLOOR_Y - y
N_OBJECTS = 4
# x y z, identity rotation, half-axes: 1.4 m tall, standing on the floor near the walls, so that the cameras (at mid-height, looking
# level, 23 degrees of view upwards and downwards) see their upper part from most poses
BODIES = np.array([[1.9, FLOOR_Y - 0.70, 0.4, 0, 0, 0, 1, 0.35, 0.70, 0.20],
                   [-1.8, FLOOR_Y - 0.70, 1.0, 0, 0, 0, 1, 0.20, 0.70, 0.40],
                   [0.3, FLOOR_Y - 0.70, -1.6, 0, 0, 0, 1, 0.45, 0.70, 0.25],
                   [-1.0, FLOOR_Y - 0.70, -1.4, 0, 0, 0, 1, 0.15, 0.70, 0.30]])


def scene(ctx, F):
    cams, depth, bgr, inst = dmb.room_frames(F)
    inst = np.where(inst >= 0, inst + N_OBJECTS, -1).astype(np.int32)
    for f0 in range(0, F, 10):          # esl_render_map in slices: its outputs are F x rows x cols doubles
        sl = slice(f0, min(f0 + 10, F))
        ren = ctx.render_map(cams[sl], BODIES, K, ROWS, COLS, want=("depth", "inst"))
        z = np.where(np.isnan(ren["depth"]), np.inf, ren["depth"])
        front = z * 5000.0 < depth[sl]
        depth[sl] = np.where(front, np.clip(np.rint(z * 5000.0), 1, 65535), depth[sl]).astype(np.uint16)
        inst[sl] = np.where(front, ren["inst"], inst[sl])
    return cams, depth, bgr, inst


def launch_split(path, calls):
    """the dense map's kernels in the profiler's per-kernel table of a run with ONE reach (warm-up + --calls calls of esl_dense_objects)"""
    import csv
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            r = {k.strip().lower(): v for k, v in r.items()}
            name = r.get("name", "")
            if any(w in name for w in ("k_dobj_", "k_dense_", "rocprim", "radix")):
                rows.append(dict(kernel=name[:120], calls=int(float(r.get("calls", 0))), total_us=float(r.get("totaldurationns", 0)) / 1e3,
                                 avg_us=float(r.get("averagens", 0)) / 1e3))
    return dict(source="rocprofv3 --kernel-trace --stats, reach 2; esl_dense_objects ran %d times (k_dense_compact / _vote and the sort "
                       "also run in esl_dense_extract, which this script does not call)" % calls, kernels=sorted(rows, key=lambda r: -r["total_us"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--numpy-frames", type=int, default=2, help="frames of the numpy statement's cut (0: skip it)")
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    ap.add_argument("--reaches", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3's *_kernel_stats.csv of a run with --reaches 2: recorded as launch_split")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    ctx = pkg.Context(0)
    t0 = time.perf_counter()
    cams, depth, bgr, inst = scene(ctx, a.frames)
    print(f"scene built in {time.perf_counter() - t0:.1f} s", flush=True)
    N = N_OBJECTS + 6
    params = pkg.abi.default_dense_params(max_voxels=a.max_voxels)
    ctx.dense_begin(params)
    add = ctx.dense_add_frames(cams, K, ROWS, COLS, depth, bgr, inst)
    info = ctx.dense_info()
    H = 2
    while H < 2 * a.max_voxels:
        H *= 2
    table_bytes = H * (8 + 64) + 2 * H * (8 + 4)
    out = dict(config=dict(frames=a.frames, rows=ROWS, cols=COLS, leaf=0.01, max_voxels=a.max_voxels, table_slots=H, calls=a.calls, N=N,
                           ground_world=list(GROUND), bodies=BODIES.tolist(), params="defaults but reach"),
               timing="kernel: HIP events around the launches (esl_profile, class 4); call: host clock around the C-ABI call",
               map=dict(add_result=add, info=info),
               yardsticks=dict(hbm_bytes_per_s=dmb.HBM_MEASURED, table_bytes=table_bytes, read_tables_once_ms=table_bytes / dmb.HBM_MEASURED * 1e3,
                               same_address_atomic_ns=10.0))
    for reach in a.reaches:
        P = pkg.abi.default_dense_obj_params(reach=reach)
        first = ctx.dense_objects(N, GROUND, P)          # warm-up: buffers grown, kernels loaded
        ctx.profile_enable(2)
        prev = ctx.profile_get().get("reduce", dict(count=0, total_ms=0.0))
        rec = dict(kernel=[], call=[])
        for _ in range(a.calls):
            res = ctx.dense_objects(N, GROUND, P)
            rec["call"].append(ctx.last_call_s * 1e3)
            pr = ctx.profile_get()["reduce"]; rec["kernel"].append(pr["total_ms"] - prev["total_ms"]); prev = pr
        ctx.profile_enable(0)
        same = all(first[k].tobytes() == res[k].tobytes() for k in ("objs", "stats", "comp", "voxel_comp"))
        n_off = ((2 * reach + 1) ** 3 - 1) // 2
        out[f"reach_{reach}"] = dict({k: dmb.stats_of(v) for k, v in rec.items()}, result=res["result"], stats=res["stats"].tolist(),
                                     largest_components=res["comp"][:N].tolist(), objs=res["objs"][:N_OBJECTS].tolist(), runs_bit_identical=bool(same),
                                     neighbour_probes=int(res["result"]["n_kept"]) * n_off,
                                     probes_per_s_kernel=res["result"]["n_kept"] * n_off / (float(np.median(rec["kernel"])) * 1e-3))
        print(f"reach {reach}", json.dumps(out[f"reach_{reach}"]), flush=True)
    if a.numpy_frames > 0:
        import dense_objects_ref as dor
        import dense_ref as dr
        n = min(a.numpy_frames, a.frames)
        m = dr.DenseMap(max_voxels=a.max_voxels)
        m.add_frames(cams[:n], K, ROWS, COLS, depth[:n], bgr[:n], inst[:n])
        ext = m.extract()
        t0 = time.perf_counter()
        ref = dor.objects(ext, 0.01, N, GROUND)
        secs = time.perf_counter() - t0
        ctx.dense_begin(params)
        ctx.dense_add_frames(cams[:n], K, ROWS, COLS, depth[:n], bgr[:n], inst[:n])
        dev = ctx.dense_objects(N, GROUND)
        out["numpy_cut"] = dict(frames=n, n_voxels=int(ext["n_voxels"]), seconds=secs, scaled_by_voxels_s=secs * info["n_voxels"] / max(ext["n_voxels"], 1),
                                result_equal=bool(dev["result"] == ref["result"]),
                                ints_equal={k: bool(np.array_equal(dev[k], ref[k])) for k in ("stats", "comp", "voxel_comp")},
                                max_abs_objs_difference=float(np.abs(dev["objs"] - ref["objs"]).max()))
        print("numpy_cut", json.dumps(out["numpy_cut"]), flush=True)
    ctx.close()
    if a.kernel_stats:
        out["launch_split"] = launch_split(a.kernel_stats, a.calls + 1)
        print("launch_split", json.dumps(out["launch_split"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
