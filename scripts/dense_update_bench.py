#!/usr/bin/env python3
"""Time esl_dense_remove_frames / _move_frames / _purge on the room of scripts/dense_map_bench.py: 100 frames of 640 x 480, stride 1,
leaf 0.01, with colour and labels, the combined form of the kernels.

Recorded, not gated (profiles/dense_update_c4.json).  Two clocks, as in dense_map_bench.py, after a warm-up of
every call (buffers grown, kernels loaded): HIP events around the launches (esl_profile_enable(ctx, 2), kernel class 4) and the host
clock around the C-ABI call, which adds the copies in and out.  Every measured call starts from the same map: esl_dense_begin and one
add of all frames at the first poses, which is also the comparison -- the rebuild from scratch that an update replaces.
  remove_all     all frames removed in one call (removal kernel + audit)
  move_1/10/100  the first 1, 10, 100 frames moved by up to 4 mm and 2 to 5 mrad (removal kernel + audit, insert kernel + audit)
  audit          a removal of ONE frame whose depth is all zero: the removal kernel ends at the depth test, what remains is the audit
  purge          after the 100-frame move
With --add-parent / --add-this (outputs of scripts/dense_map_bench.py on the parent commit and on this one, same session, same card)
the add path's comparison is recorded too: the add kernel times must agree within the larger of 3 % and the parent's own spread.

    python scripts/dense_update_bench.py --out profiles/dense_update_c4.json
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import dense_map_bench as dmb          # noqa: E402


def second_poses(cams, seed=1):
    """every pose up to 4 mm and 2 to 5 mrad off"""
    rng = np.random.default_rng(seed)
    out = cams.copy()
    for f in range(len(out)):
        out[f, :3] += rng.uniform(-0.004, 0.004, 3)
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        ang = rng.uniform(0.002, 0.005)
        bx, by, bz, bw = np.concatenate([np.sin(ang / 2) * ax, [np.cos(ang / 2)]])
        x, y, z, w = out[f, 3:]
        out[f, 3:] = [w * bx + x * bw + y * bz - z * by, w * by - x * bz + y * bw + z * bx, w * bz + x * by - y * bx + z * bw,
                      w * bw - x * bx - y * by - z * bz]
    return out


def add_comparison(parent, this):
    """the add kernel's medians of both runs, form by form, and the margin the parent's own repetitions give"""
    out = dict(parent=parent, this=this, forms={})
    ok = True
    for form in ("plain", "combined"):
        p, t = parent[form]["add_kernel"], this[form]["add_kernel"]
        spread = (p["ms_max"] - p["ms_min"]) / p["ms_median"]
        margin = max(0.03, spread)
        rel = t["ms_median"] / p["ms_median"] - 1.0
        out["forms"][form] = dict(parent_ms_median=p["ms_median"], this_ms_median=t["ms_median"], relative_difference=rel,
                                  parent_spread=spread, margin=margin, within_margin=bool(abs(rel) <= margin))
        ok = ok and abs(rel) <= margin
    out["add_not_slower_within_margin"] = bool(ok)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    ap.add_argument("--add-parent", default=None, help="dense_map_bench.py's output on the parent commit")
    ap.add_argument("--add-this", default=None, help="dense_map_bench.py's output on this commit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    F, ROWS, COLS, K = a.frames, dmb.ROWS, dmb.COLS, dmb.K
    cams, depth, bgr, inst = dmb.room_frames(F)
    cams2 = second_poses(cams)
    params = pkg.abi.default_dense_params(max_voxels=a.max_voxels)
    os.environ["ESL_DENSE_COMBINE"] = "1"
    ctx = pkg.Context(0)
    ctx.profile_enable(2)
    clock = dict(prev=0.0)

    def timed(call):
        res = call()
        total = ctx.profile_get().get("reduce", dict(total_ms=0.0))["total_ms"]
        kernel, clock["prev"] = total - clock["prev"], total
        return res, kernel, ctx.last_call_s * 1e3

    def rebuild():
        ctx.dense_begin(params)
        return timed(lambda: ctx.dense_add_frames(cams, K, ROWS, COLS, depth, bgr, inst))

    def moved(n):
        c = cams.copy(); c[:n] = cams2[:n]
        return c

    zero = np.zeros((1, ROWS, COLS), np.uint16)
    cases = dict(
        remove_all=lambda: ctx.dense_remove_frames(cams, K, ROWS, COLS, depth, bgr, inst),
        move_1=lambda: ctx.dense_move_frames(cams, moved(1), K, ROWS, COLS, depth, bgr, inst),
        move_10=lambda: ctx.dense_move_frames(cams, moved(min(10, F)), K, ROWS, COLS, depth, bgr, inst),
        move_100=lambda: ctx.dense_move_frames(cams, moved(F), K, ROWS, COLS, depth, bgr, inst),
        audit=lambda: ctx.dense_remove_frames(cams[:1], K, ROWS, COLS, zero, bgr[:1], inst[:1]))
    out = dict(config=dict(frames=F, rows=ROWS, cols=COLS, stride=1, leaf=0.01, with_color=1, with_inst=1, max_voxels=a.max_voxels,
                           calls=a.calls, form="combined", K=list(K)),
               timing="kernel: HIP events around the launches (esl_profile, class 4); call: host clock around the C-ABI call (copies included)")
    rec = {k: dict(kernel=[], call=[]) for k in list(cases) + ["rebuild", "purge"]}
    last = {}
    for rep in range(a.calls + 1):          # round 0 is the warm-up
        for name, call in cases.items():
            _, k0, c0 = rebuild()
            res, k1, c1 = timed(call)
            slots = ctx.dense_slots()
            if name == "move_100":
                (before, after), k2, c2 = timed(ctx.dense_purge)
                last["purge"] = dict(before=before, after=after)
            if rep:
                rec["rebuild"]["kernel"].append(k0); rec["rebuild"]["call"].append(c0)
                rec[name]["kernel"].append(k1); rec[name]["call"].append(c1)
                if name == "move_100":
                    rec["purge"]["kernel"].append(k2); rec["purge"]["call"].append(c2)
            last[name] = dict(result=res, slots_after=slots, info_after=ctx.dense_info())
    for name, r in rec.items():
        out[name] = dict(kernel=dmb.stats_of(r["kernel"]), call=dmb.stats_of(r["call"]), **last.get(name, {}))
        print(name, json.dumps(out[name]), flush=True)
    # the contract, on this scene: the moved map equals the map built from scratch at the moved poses
    ctx.dense_begin(params)
    ctx.dense_add_frames(moved(F), K, ROWS, COLS, depth, bgr, inst)
    want = ctx.dense_extract()
    ctx.dense_begin(params)
    ctx.dense_add_frames(cams, K, ROWS, COLS, depth, bgr, inst)
    ctx.dense_move_frames(cams, moved(F), K, ROWS, COLS, depth, bgr, inst)
    got = ctx.dense_extract()
    out["moved_equals_from_scratch"] = bool(all(got[k].tobytes() == want[k].tobytes() for k in ctx.DENSE_OUTPUTS))
    print("moved_equals_from_scratch", out["moved_equals_from_scratch"], flush=True)
    ctx.close()
    if a.add_parent and a.add_this:
        out["add_path"] = add_comparison(json.load(open(a.add_parent)), json.load(open(a.add_this)))
        print("add_path", json.dumps(out["add_path"]["forms"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
