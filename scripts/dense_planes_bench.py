#!/usr/bin/env python3
"""Time esl_dense_planes on the synthetic room of scripts/dense_objects_bench.py (100 frames of 640 x 480, leaf 0.01, four tall ellipsoids near
the walls), with the defaults, up = the room's up (-y) and skip_labelled 0 and 1, and once with --small-hyp hypotheses (fewer than a
wave: scored by k_dpl_few, lane = voxel, not by k_dpl_score).  The cameras of
that room look level with 23 degrees of view up and down, so no frame shows the floor or the ceiling: the map holds the four walls
and the bodies, and the right answer to the ground question is "none" (ground_index -1).  Finding a ground at this size is NOT measured.

Recorded, not gated (profiles/dense_planes_c4.json, DESIGN.md "Dominant planes and the ground from the dense map"): there is no earlier
implementation to compare with.  Two clocks, medians of --calls calls after a warm-up call: HIP events on the context's stream around the
launches (esl_profile_enable(ctx, 2), kernel class 4: every bracket of the call, the sorted list included) and the host clock around the
C-ABI call, which adds the host round trips of every round, the hypotheses built on the host and the copies.  Beside them:
  - the plane tests of k_dpl_score (n_hypotheses x n_r per round started) per second of its own time, against the FP64 vector peak
    with the kernel's instructions per test read from its ISA;
  - the time to stream the list of 32-byte entries once at the measured HBM rate;
  - the numpy statement (tests/dense_planes_ref.py) timed on the map of the first frames with --numpy-hyp hypotheses per round and
    scaled by rounds x n_hypotheses x n_voxels -- and compared with the device on that cut, every integer output.
The profile's brackets are per class, not per kernel: the split per launch comes from a second run of this script under the profiler,
whose per-kernel table is merged into the record with --kernel-stats.

    rocprofv3 --kernel-trace --stats --output-format csv -d prof -- python scripts/dense_planes_bench.py --skips 0 --small-hyp 0 --numpy-frames 0
    python scripts/dense_planes_bench.py --kernel-stats prof/*/*_kernel_stats.csv --out profiles/dense_planes_c4.json
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
import dense_objects_bench as dob      # noqa: E402

ROWS, COLS, K = dmb.ROWS, dmb.COLS, dmb.K
UP = (0.0, -1.0, 0.0)          # the room's +y is down
# FLOP/s: AMD's published peak FP64 vector rate of the MI355X (half its FP32 vector rate), that is 39.3e12 FP64 instructions per lane and
# second.  Taken from the data sheet, not measured here.
FP64_VECTOR_PEAK = 78.6e12
ENTRY_BYTES = 32
# k_dpl_score's inner loop per test, from the ISA (hipcc -S, -O3 -ffp-contract=off): 3 v_mul_f64, 3 v_add_f64, 1 v_cmp_le_f64 with |.|;
# 3 v_cndmask_b32, 1 v_lshl_add_u64 and half a v_add3_u32; 2 ds_read_b128 (broadcast)
FP64_INSTR_PER_TEST = 7
OTHER_VALU_PER_TEST = 4.5


def rounds_n_r(res):
    """n_r of every round started: the eligible voxels minus those assigned before it"""
    left, out = res["result"]["n_eligible"], []
    for p in range(res["result"]["rounds"]):
        out.append(left)
        if p < res["result"]["n_planes"]:
            left -= int(res["stats"][p, 0])
    return out


def launch_split(path, calls):
    """esl_dense_planes' kernels in the profiler's per-kernel table of a run with ONE setting (warm-up + --calls calls)"""
    import csv
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            r = {k.strip().lower(): v for k, v in r.items()}
            name = r.get("name", "")
            if any(w in name for w in ("k_dpl_", "k_dense_", "rocprim", "radix", "select", "lookback")):
                rows.append(dict(kernel=name[:120], calls=int(float(r.get("calls", 0))), total_us=float(r.get("totaldurationns", 0)) / 1e3,
                                 avg_us=float(r.get("averagens", 0)) / 1e3))
    return dict(source="rocprofv3 --kernel-trace --stats, skip_labelled 0; esl_dense_planes ran %d times" % calls,
                kernels=sorted(rows, key=lambda r: -r["total_us"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--numpy-frames", type=int, default=2, help="frames of the numpy statement's cut (0: skip it)")
    ap.add_argument("--numpy-hyp", type=int, default=256, help="hypotheses per round of the numpy statement's run")
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    ap.add_argument("--skips", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--small-hyp", type=int, default=32, help="n_hypotheses of the extra run below one wave (0: skip it)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3's *_kernel_stats.csv of a run with --skips 0: recorded as launch_split")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    ctx = pkg.Context(0)
    t0 = time.perf_counter()
    cams, depth, bgr, inst = dob.scene(ctx, a.frames)
    print(f"scene built in {time.perf_counter() - t0:.1f} s", flush=True)
    params = pkg.abi.default_dense_params(max_voxels=a.max_voxels)
    ctx.dense_begin(params)
    add = ctx.dense_add_frames(cams, K, ROWS, COLS, depth, bgr, inst)
    info = ctx.dense_info()
    tile, group = ctx.dense_planes_layout()
    out = dict(config=dict(frames=a.frames, rows=ROWS, cols=COLS, leaf=0.01, max_voxels=a.max_voxels, calls=a.calls, up=list(UP),
                           params="defaults but up and skip_labelled", score_tile=tile, score_group=group),
               timing="kernel: HIP events around the launches (esl_profile, class 4); call: host clock around the C-ABI call",
               map=dict(add_result=add, info=info),
               yardsticks=dict(hbm_bytes_per_s=dmb.HBM_MEASURED, entry_bytes=ENTRY_BYTES,
                               stream_list_once_ms=info["n_voxels"] * ENTRY_BYTES / dmb.HBM_MEASURED * 1e3,
                               fp64_vector_peak_flops=FP64_VECTOR_PEAK, fp64_vector_peak_source="AMD's data sheet; not measured",
                               fp64_instr_per_test=FP64_INSTR_PER_TEST,
                               other_valu_per_test=OTHER_VALU_PER_TEST, lds_reads_per_test="2 ds_read_b128",
                               tests_per_s_at_fp64_issue_peak=FP64_VECTOR_PEAK / 2 / FP64_INSTR_PER_TEST),
               not_measured=["hardware counters of k_dpl_score (LDS stalls, VALU busy): no counter run was made",
                             "other forms of k_dpl_score (lane = voxel; scalar loads instead of LDS; two hypotheses per lane): not built",
                             "n_hypotheses other than the default and --small-hyp", "finding a ground at this size: the room's frames show no floor",
                             "real data: the thresholds are design choices"])
    runs = [(f"skip_labelled_{skip}", dict(skip_labelled=skip)) for skip in a.skips]
    if a.small_hyp > 0:
        runs.append((f"n_hypotheses_{a.small_hyp}", dict(n_hypotheses=a.small_hyp)))
    for name, over in runs:
        P = pkg.abi.default_dense_plane_params(up=UP, **over)
        first = ctx.dense_planes(P)          # warm-up: buffers grown, kernels loaded
        ctx.profile_enable(2)
        prev = ctx.profile_get().get("reduce", dict(count=0, total_ms=0.0))
        rec = dict(kernel=[], call=[])
        for _ in range(a.calls):
            res = ctx.dense_planes(P)
            rec["call"].append(ctx.last_call_s * 1e3)
            pr = ctx.profile_get()["reduce"]; rec["kernel"].append(pr["total_ms"] - prev["total_ms"]); prev = pr
        ctx.profile_enable(0)
        same = all(first[k].tobytes() == res[k].tobytes() for k in ("planes", "centroid", "stats", "samples", "ground", "voxel_plane"))
        n_r = rounds_n_r(res)
        tests = int(P.n_hypotheses) * sum(n_r)
        out[name] = dict({k: dmb.stats_of(v) for k, v in rec.items()}, result=res["result"], stats=res["stats"].tolist(),
                                            planes=res["planes"].tolist(), ground=res["ground"].tolist(), samples=res["samples"].tolist(),
                                            runs_bit_identical=bool(same), n_r=n_r, plane_tests=tests,
                                            plane_tests_per_s_of_all_kernel_time=tests / (float(np.median(rec["kernel"])) * 1e-3))
        print(name, json.dumps(out[name]), flush=True)
    if a.numpy_frames > 0:
        import dense_planes_ref as dpr
        import dense_ref as dr
        n = min(a.numpy_frames, a.frames)
        m = dr.DenseMap(max_voxels=a.max_voxels)
        m.add_frames(cams[:n], K, ROWS, COLS, depth[:n], bgr[:n], inst[:n])
        ext = m.extract()
        kw = dict(up=UP, n_hypotheses=a.numpy_hyp)
        t0 = time.perf_counter()
        ref = dpr.planes(ext, 0.01, **kw)
        secs = time.perf_counter() - t0
        ctx.dense_begin(params)
        ctx.dense_add_frames(cams[:n], K, ROWS, COLS, depth[:n], bgr[:n], inst[:n])
        dev = ctx.dense_planes(pkg.abi.default_dense_plane_params(**kw), hyp=True)
        work = max(ref["result"]["rounds"], 1) * a.numpy_hyp * max(ext["n_voxels"], 1)
        full = out.get("skip_labelled_0")
        out["numpy_cut"] = dict(frames=n, n_voxels=int(ext["n_voxels"]), n_hypotheses=a.numpy_hyp, rounds=ref["result"]["rounds"], seconds=secs,
                                seconds_per_round_hypothesis_voxel=secs / work,
                                scaled_to_the_full_call_s=(secs / work * full["result"]["rounds"] * 1024 * info["n_voxels"]) if full else None,
                                result_equal=bool(dev["result"] == ref["result"]),
                                ints_equal={k: bool(np.array_equal(dev[k], ref[k])) for k in ("stats", "samples", "voxel_plane", "hyp")},
                                max_abs_difference={k: float(np.abs(dev[k] - ref[k]).max()) if dev[k].shape == ref[k].shape and dev[k].size else None
                                                    for k in ("planes", "centroid", "ground")})
        print("numpy_cut", json.dumps(out["numpy_cut"]), flush=True)
    ctx.close()
    if a.kernel_stats:
        out["launch_split"] = launch_split(a.kernel_stats, a.calls + 1)
        score = [r for r in out["launch_split"]["kernels"] if "k_dpl_score" in r["kernel"]]
        full = out.get("skip_labelled_0")
        if score and full:
            per_call_s = score[0]["total_us"] * 1e-6 / (a.calls + 1)
            rate = full["plane_tests"] / per_call_s
            out["launch_split"]["k_dpl_score"] = dict(ms_per_call=per_call_s * 1e3, plane_tests_per_s=rate,
                                                      fraction_of_fp64_issue_peak=rate / (FP64_VECTOR_PEAK / 2 / FP64_INSTR_PER_TEST))
        print("launch_split", json.dumps(out["launch_split"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
