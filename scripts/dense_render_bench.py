#!/usr/bin/env python3
"""Time esl_dense_render on the synthetic room of scripts/dense_map_bench.py (100 frames of 640 x 480, leaf 0.01, about 4.3e5 voxels): the
map is built from the frames and then viewed from the frames' own poses, 1 frame and all of them, with and without the frames' depth
as depth_meas.

Recorded, not gated (profiles/dense_render_c4.json, DESIGN.md "Viewing the dense map"): there is no earlier implementation, the parent
cannot run the call.  Two clocks, medians of --calls calls after a warm-up call: HIP events on the context's stream around the launches
(esl_profile_enable(ctx, 2), kernel class 4: the sorted list and the gather included) and the host clock around the C-ABI call, which
adds the uploads, the clearing of the z-buffer and the copies of the outputs.  Timed with the counts alone (frame, vox) and, for one
frame, with every image.  Beside them:
  - the share of pixels without a winner at footprint 1.0 and 1.5;
  - the numpy statement (tests/dense_render_ref.py) on the first frame, from the device's own esl_dense_extract, timed and compared;
  - esl_render_map's 100-frame line of profiles/render_c4.json, as a yardstick of another kind of view (87 ellipsoids, not 4e5 voxels);
  - --ab N: the load-first test against an unconditional atomicMin (ESL_DRN_LOADFIRST=1 / 0), N processes per arm, alternated, each
    timing the 100-frame call with depth_meas; the outputs' SHA-1 of both arms;
  - --count-lib PATH: a build of the library with -DESL_DRN_COUNT (it prints the candidates formed and the atomicMins issued); run
    once per arm in a process of its own.
        make -C object-oriented-slam_amd/csrc   # then, for the counting build:
        cd object-oriented-slam_amd/csrc && hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -ffp-contract=off \\
            -DESL_DRN_COUNT -c esl_dense_render.hip -o /tmp/drn_count.o && hipcc --offload-arch=gfx950 -shared -fPIC \\
            -o libesl_hip_drncount.so $(ls *.o | grep -v esl_dense_render.o) /tmp/drn_count.o -ldl
    python scripts/dense_render_bench.py --ab 3 --count-lib object-oriented-slam_amd/csrc/libesl_hip_drncount.so --out profiles/dense_render_c4.json
"""
import argparse
import hashlib
import importlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import dense_map_bench as dmb          # noqa: E402

ROWS, COLS, K = dmb.ROWS, dmb.COLS, dmb.K
COUNTS = ("frame", "vox")
IMAGES = ("depth", "voxel", "bgr", "inst")


def load_scene(path, frames):
    if path and os.path.exists(path):
        z = np.load(path)
        return z["cams"], z["depth"], z["bgr"], z["inst"]
    s = dmb.room_frames(frames)
    if path:
        np.savez(path, cams=s[0], depth=s[1], bgr=s[2], inst=s[3])
    return s


def build_map(pkg, ctx, scene, max_voxels):
    cams, depth, bgr, inst = scene
    ctx.dense_begin(pkg.abi.default_dense_params(max_voxels=max_voxels))
    return ctx.dense_add_frames(cams, K, ROWS, COLS, depth, bgr, inst)


def timed(ctx, calls, fn):
    """warm-up, then `calls` calls: medians of the kernel time (class 4 brackets) and of the call time; the last result"""
    first = fn()
    ctx.profile_enable(2)
    prev = ctx.profile_get().get("reduce", dict(count=0, total_ms=0.0))
    rec = dict(kernel=[], call=[])
    res = first
    for _ in range(calls):
        res = fn()
        rec["call"].append(ctx.last_call_s * 1e3)
        pr = ctx.profile_get()["reduce"]; rec["kernel"].append(pr["total_ms"] - prev["total_ms"]); prev = pr
    ctx.profile_enable(0)
    same = all(first[k].tobytes() == res[k].tobytes() for k in first if k != "result")
    return dict({k: dmb.stats_of(v) for k, v in rec.items()}, runs_bit_identical=bool(same)), res


def digest(res):
    h = hashlib.sha1()
    for k in sorted(res):
        if k != "result":
            h.update(res[k].tobytes())
    return h.hexdigest()


def arm_main(a):
    """one arm of the A/B in this process: the 100-frame call with depth_meas, counts alone"""
    pkg = importlib.import_module("object-oriented-slam_amd")
    ctx = pkg.Context(0)
    scene = load_scene(a.scene, a.frames)
    build_map(pkg, ctx, scene, a.max_voxels)
    t, res = timed(ctx, a.calls, lambda: ctx.dense_render(scene[0], K, ROWS, COLS, scene[1], want=COUNTS))
    ctx.close()
    print("ARM " + json.dumps(dict(load_first=os.environ.get("ESL_DRN_LOADFIRST", "unset"), timing=t, sha1=digest(res),
                                   covered=int(res["frame"][:, 3].sum()))), flush=True)


def child(a, env_over, extra=()):
    env = dict(os.environ); env.update(env_over)
    cmd = [sys.executable, os.path.abspath(__file__), "--arm", "--scene", a.scene, "--frames", str(a.frames), "--calls", str(a.calls),
           "--max-voxels", str(a.max_voxels), *extra]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"an arm ended with status {p.returncode}: {p.stderr[-2000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ARM ")][-1]
    return json.loads(line[4:]), p.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    ap.add_argument("--numpy-frames", type=int, default=1, help="0: skip the numpy statement")
    ap.add_argument("--ab", type=int, default=0, help="processes per arm of the load-first A/B (0: skip it)")
    ap.add_argument("--count-lib", default=None, help="a -DESL_DRN_COUNT build of the library: candidates and atomicMins per arm")
    ap.add_argument("--scene", default=None, help="an .npz to keep the scene in between processes")
    ap.add_argument("--arm", action="store_true", help="(internal) time one arm and print it")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return arm_main(a)
    tmp = None
    if a.scene is None:
        tmp = tempfile.mkdtemp(prefix="drn_bench_")
        a.scene = os.path.join(tmp, "scene.npz")
    pkg = importlib.import_module("object-oriented-slam_amd")
    ctx = pkg.Context(0)
    t0 = time.perf_counter()
    scene = load_scene(a.scene, a.frames)
    cams, depth, bgr, inst = scene
    print(f"scene built in {time.perf_counter() - t0:.1f} s", flush=True)
    add = build_map(pkg, ctx, scene, a.max_voxels)
    info = ctx.dense_info()
    F, npix = len(cams), ROWS * COLS
    yard = json.load(open(os.path.join(ROOT, "profiles", "render_c4.json"))).get("frames", {})
    out = dict(config=dict(frames=F, rows=ROWS, cols=COLS, leaf=0.01, max_voxels=a.max_voxels, calls=a.calls, params="defaults",
                           load_first=os.environ.get("ESL_DRN_LOADFIRST", "unset (= 0)")),
               timing="kernel: HIP events around the launches (esl_profile, class 4); call: host clock around the C-ABI call",
               map=dict(add_result=add, info=info),
               yardsticks=dict(esl_render_map_100_frames=dict(kernel=yard.get("kernel"), call=yard.get("call"), outputs=yard.get("outputs"),
                                                              note="profiles/render_c4.json: 87 ellipsoids ray-cast into the same 100 frames; another kind of view"),
                               hbm_bytes_per_s=dmb.HBM_MEASURED,
                               clear_and_read_zbuf_once_ms=2 * 8 * F * npix / dmb.HBM_MEASURED * 1e3),
               not_measured=["real sequences: the room is synthetic and every voxel is seen", "leaves other than 0.01 m",
                             "a tile-binned form with the z-buffer in LDS: not built",
                             "hardware counters of k_drn_splat (atomic unit busy, L2 hit rate): no counter run was made",
                             "max_radius and min_count other than the defaults", "more than one chunk at this size"])
    runs = [("one_frame_counts", slice(0, 1), True, COUNTS), ("one_frame_counts_no_meas", slice(0, 1), False, COUNTS),
            ("one_frame_all_outputs", slice(0, 1), True, COUNTS + IMAGES),
            (f"frames_{F}_counts", slice(None), True, COUNTS), (f"frames_{F}_counts_no_meas", slice(None), False, COUNTS)]
    for name, fs, meas, want in runs:
        t, res = timed(ctx, a.calls, lambda: ctx.dense_render(cams[fs], K, ROWS, COLS, depth[fs] if meas else None, want=want))
        fr = res["frame"].astype(np.int64)
        n_f = len(fr)
        out[name] = dict(t, outputs=list(want), result=res["result"], frame_totals=dict(zip(("n_drawn", "n_depth_out", "n_outside", "covered", "agree",
                                                                                              "nearer", "farther", "nodata"), fr.sum(axis=0).tolist())),
                         share_of_pixels_without_a_winner=1.0 - float(fr[:, 3].sum()) / (n_f * npix),
                         voxel_frames_per_s_of_kernel_time=info["n_voxels"] * n_f / (t["kernel"]["ms_median"] * 1e-3),
                         voxels_seen_through=int((res["vox"][:, 3] > 0).sum()))
        print(name, json.dumps(out[name]), flush=True)
    for fp in (1.0, 1.5):
        res = ctx.dense_render(cams, K, ROWS, COLS, None, pkg.abi.default_dense_render_params(footprint=fp), want=("frame",))
        out[f"footprint_{fp}"] = dict(share_of_pixels_without_a_winner=1.0 - float(res["frame"][:, 3].astype(np.int64).sum()) / (F * npix),
                                      drawn=int(res["frame"][:, 0].astype(np.int64).sum()))
        print(f"footprint_{fp}", json.dumps(out[f"footprint_{fp}"]), flush=True)
    if a.numpy_frames > 0:
        import dense_render_ref as drr
        n = min(a.numpy_frames, F)
        ext = ctx.dense_extract()
        dev = ctx.dense_render(cams[:n], K, ROWS, COLS, depth[:n])
        t0 = time.perf_counter()
        ref = drr.render(ext, 0.01, cams[:n], K, ROWS, COLS, depth[:n])
        secs = time.perf_counter() - t0
        out["numpy_statement"] = dict(frames=n, seconds=secs, result_equal=bool(dev["result"] == ref["result"]),
                                      equal={k: bool(np.array_equal(dev[k], ref[k], equal_nan=(k == "depth"))) for k in COUNTS + IMAGES},
                                      smallest_margins=ref["margins"])
        print("numpy_statement", json.dumps(out["numpy_statement"]), flush=True)
    ctx.close()
    if a.ab > 0:
        arms = {"1": [], "0": []}
        for i in range(2 * a.ab):          # alternated
            lf = "1" if i % 2 == 0 else "0"
            arms[lf].append(child(a, dict(ESL_DRN_LOADFIRST=lf))[0])
        med = {lf: float(np.median([r["timing"]["kernel"]["ms_median"] for r in rs_])) for lf, rs_ in arms.items()}
        out["ab_load_first"] = dict(what=f"{F} frames with depth_meas, counts alone; kernel ms of class 4, median of --calls calls per process",
                                    load_first=arms["1"], unconditional=arms["0"], kernel_ms_median_of_processes=dict(load_first=med["1"], unconditional=med["0"]),
                                    unconditional_over_load_first=med["0"] / med["1"],
                                    same_bytes=len({r["sha1"] for rs_ in arms.values() for r in rs_}) == 1)
        print("ab_load_first", json.dumps(out["ab_load_first"]), flush=True)
    if a.count_lib:
        out["atomics"] = {}
        for lf in ("1", "0"):
            _, err = child(a, dict(ESL_DRN_LOADFIRST=lf, ESL_HIP_LIB=os.path.abspath(a.count_lib)), extra=())
            m = re.findall(r"esl_dense_render: candidates (\d+) atomics (\d+)", err)
            cand, atom = (int(v) for v in m[-1])
            out["atomics"]["load_first" if lf == "1" else "unconditional"] = dict(candidates=cand, atomic_mins=atom, share=atom / max(cand, 1))
        print("atomics", json.dumps(out["atomics"]), flush=True)
    if tmp:
        os.remove(a.scene); os.rmdir(tmp)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
