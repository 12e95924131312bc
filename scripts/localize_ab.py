"""Localisation against a fixed map (esl_graph_upload_fixed with every ellipsoid fixed, ESL_SOLVER_CAMERA_CHAIN): throughput and the
A/B figures of DESIGN.md section 4.15, one process, every pair alternated A/B/A/B, a warm-up run before every timed window, host
clock after a device synchronisation.  Prints one JSON object.

  * C3 and C4 localisation, analytic and numeric Jacobians: LM iterations/s, ms per trial, esl_profile_get's split
  * C3 localisation: solver 3 (camera chain) against solver 1 (reduced camera system, dense order 2,994)
  * C3 joint SLAM (no flags) against C3 localisation

  python scripts/localize_ab.py [--rounds 2] [--c3-steps 10] [--c4-steps 3] [--no-c4]
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


def window(ctx, params, steps):
    """(LM iterations/s, ms per trial, iterations, trials) of `steps` runs from the snapshot, after one warm-up run"""
    ctx.restore_states(); ctx.optimize_resident(params)
    ctx.synchronize()
    t0 = time.perf_counter()
    iters = trials = 0
    for _ in range(steps):
        ctx.restore_states()
        rep = ctx.optimize_resident(params)
        iters += rep["iterations"]; trials += rep["total_trials"]
    ctx.synchronize()
    dt = time.perf_counter() - t0
    return iters / dt, 1e3 * dt / max(trials, 1), iters, trials


def profile(ctx, params):
    ctx.restore_states()
    ctx.profile_enable(2)
    ctx.optimize_resident(params)
    p = ctx.profile_get()
    ctx.profile_enable(0)
    return {k: dict(count=v["count"], ms=round(v["total_ms"], 4)) for k, v in p.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--c3-steps", type=int, default=10)
    ap.add_argument("--c4-steps", type=int, default=3)
    ap.add_argument("--no-c4", action="store_true")
    a = ap.parse_args()
    pkg = importlib.import_module("object-oriented-slam_amd")
    ctx = pkg.Context(0)
    out = {}
    for name, steps in (("C3", a.c3_steps),) + (() if a.no_c4 else (("C4", a.c4_steps),)):
        g, c, o, _ = pkg.synth.make_config(name, seed=0, slam=True)
        ones = np.ones(g.n_objs, np.uint8)
        ctx.upload_graph(g, obj_fixed=ones); ctx.upload_states(c, o); ctx.snapshot_states()
        res = {}
        for jac, tag in ((1, "analytic"), (0, "numeric")):
            p = pkg.default_lm_params(jacobian_mode=jac)
            rounds = [window(ctx, p, steps) for _ in range(a.rounds)]
            assert ctx.lm_solver_used() == 3
            res[tag] = dict(lm_it_per_s=[round(r[0], 3) for r in rounds], ms_per_trial=[round(r[1], 4) for r in rounds],
                            iterations=rounds[0][2], trials=rounds[0][3], profile=profile(ctx, p))
            print(f"{name} localisation {tag}: {res[tag]['lm_it_per_s']} LM it/s, {res[tag]['ms_per_trial']} ms per trial", flush=True)
        n_anch = int((g.cam_fixed[g.bbox_cam] == 0).sum()), int((g.cam_fixed[g.e3d_cam] == 0).sum())
        res["anchored_edges"] = dict(bbox=n_anch[0], e3d=n_anch[1], free_cameras=int((g.cam_fixed == 0).sum()))
        out[name + " localisation"] = res
        if name != "C3":
            continue
        # the reason the solver exists: the same graph through the dense reduced camera system
        ab = {"chain": [], "reduced_camera": []}
        for r in range(a.rounds):
            for tag, solver in (("chain", 3), ("reduced_camera", 1)):
                v = window(ctx, pkg.default_lm_params(jacobian_mode=1, linear_solver=solver), steps)
                assert ctx.lm_solver_used() == solver
                ab[tag].append(round(v[0], 3))
        out["C3 localisation, solver 3 vs solver 1"] = dict(lm_it_per_s=ab, chain_not_slower_in_every_pair=all(x >= y for x, y in zip(ab["chain"], ab["reduced_camera"])),
                                                            ratio=round(sum(ab["chain"]) / sum(ab["reduced_camera"]), 3))
        print("C3 solver 3 vs 1:", out["C3 localisation, solver 3 vs solver 1"], flush=True)
        # joint SLAM (no flags) against localisation, same process
        joint = pkg.Context(0)
        try:
            joint.upload_graph(g); joint.upload_states(c, o); joint.snapshot_states()
            jl = {"joint_slam": [], "localisation": []}
            p = pkg.default_lm_params(jacobian_mode=1)
            for r in range(a.rounds):
                jl["joint_slam"].append(round(window(joint, p, steps)[0], 3))
                jl["localisation"].append(round(window(ctx, p, steps)[0], 3))
            out["C3 joint SLAM vs localisation"] = dict(lm_it_per_s=jl, joint_solver=joint.lm_solver_used())
            print("C3 joint vs localisation:", out["C3 joint SLAM vs localisation"], flush=True)
        finally:
            joint.close()
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
