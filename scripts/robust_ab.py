"""A/B cost of a robust kernel (esl_lm_set_robust): C4 SLAM (bench.py's configuration) and C4 mapping, robust off and Huber on the
bbox edges, alternating A/B/A/B in one process.  Prints LM iterations per second of every round (a robust run may take another
number of iterations: the rate, not the step time, is the comparable figure) and the mean per setting.

  python scripts/robust_ab.py [--rounds 2] [--slam-steps 3] [--map-steps 20] [--delta 1.0]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rate(ctx, params, steps):
    ctx.restore_states(); ctx.optimize_resident(params)   # warm-up (first use of the robust instantiations / solver blobs)
    ctx.synchronize()
    t0 = time.perf_counter()
    iters = 0
    for _ in range(steps):
        ctx.restore_states()
        iters += ctx.optimize_resident(params)["iterations"]
    ctx.synchronize()
    return iters / (time.perf_counter() - t0), iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--slam-steps", type=int, default=3)
    ap.add_argument("--map-steps", type=int, default=20)
    ap.add_argument("--delta", type=float, default=1.0, help="Huber width on the bbox edges (pixels)")
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    ctx = pkg.Context(0)
    out = {}
    for mode, slam, steps in (("C4 SLAM", True, a.slam_steps), ("C4 mapping", False, a.map_steps)):
        g, c, o, _ = pkg.synth.make_config("C4", seed=0, slam=slam)
        ctx.upload_graph(g); ctx.upload_states(c, o); ctx.snapshot_states()
        params = pkg.default_lm_params(jacobian_mode=1)
        res = {"off": [], "huber_bbox": []}
        for r in range(a.rounds):
            for name in ("off", "huber_bbox"):
                ctx.set_robust(bbox=("huber", a.delta) if name == "huber_bbox" else None)
                v, it = rate(ctx, params, steps)
                res[name].append(v)
                print(f"{mode:11s} round {r} {name:10s} {v:8.3f} LM it/s ({it} iterations)", flush=True)
        ctx.set_robust()
        m = {k: sum(v) / len(v) for k, v in res.items()}
        out[mode] = dict(rounds=res, mean=m, huber_vs_off=m["huber_bbox"] / m["off"] - 1.0)
        print(f"{mode}: off {m['off']:.3f}, Huber on bbox {m['huber_bbox']:.3f} LM it/s ({100 * out[mode]['huber_vs_off']:+.2f} %)", flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
