#!/usr/bin/env python
"""ESL_SOLVER_PCG against the direct forms on one MI355X -> profiles/pcg_c3_c4.json.

BASELINE configs C3 and C4 in SLAM mode, analytic Jacobians, full optimize(10) steps on the resident graph (states restored on the
device before every step), 20 timed steps after 5 warm-ups:
  - solver 4 (PCG) at rel_tol 1e-8 and 1e-10, solver AUTO (what the library picks without the request) on the same graphs;
  - the C4 graph with ONE added loop-closure odometry edge (cameras 3 -> 9999): solver 4, and solver 1 (the reduced camera system;
    solver 2 is refused on that graph) -- the dense form takes over a second per trial there, so it gets 2 steps after 1 warm-up;
  - a rocprofv3 --kernel-trace --stats run of the C4 PCG case (3 steps after 1 warm-up, no counters): its top five kernels.
Per run: ms per trial, LM iterations/s, PCG iterations per solve, final chi2.

Every GPU step is a child process of its own under its own `timeout -k 10`; the parent never opens the GPU, builds the graphs once
(numpy) and stops at the first step that fails.

  python scripts/measure_pcg.py [--out profiles/pcg_c3_c4.json] [--only c3|c4] [--no-rocprof]
"""
import argparse
import glob
import importlib
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = ("cam_fixed", "bbox_cam", "bbox_obj", "bbox_meas", "bbox_weight", "e3d_cam", "e3d_obj", "e3d_meas", "e3d_weight", "grav_obj",
          "odom_i", "odom_j", "odom_meas")


def save_graph(path, g, c, o):
    np.savez(path, K=np.array(g.K), n_cams=g.n_cams, n_objs=g.n_objs, grav_normal=np.array(g.grav_normal), grav_weight=g.grav_weight,
             cams=c, objs=o, **{f: getattr(g, f) for f in FIELDS})


def load_graph(pkg, path):
    z = np.load(path)
    g = pkg.Graph(tuple(z["K"]), int(z["n_cams"]), int(z["n_objs"]), z["cam_fixed"], z["bbox_cam"], z["bbox_obj"], z["bbox_meas"], z["bbox_weight"],
                  z["e3d_cam"], z["e3d_obj"], z["e3d_meas"], z["e3d_weight"], z["grav_obj"], tuple(z["grav_normal"]), float(z["grav_weight"]),
                  z["odom_i"], z["odom_j"], z["odom_meas"])
    return g, z["cams"], z["objs"]


def with_loop_closure(pkg, g, truth, i, j):
    from oracle import np_oracle as npo
    Z = npo.T_from7(truth["cams"][j]) @ npo.T_inv(npo.T_from7(truth["cams"][i]))   # Tcw_j Tcw_i^-1 of the true poses
    z7 = np.concatenate([Z[:3, 3], pkg.synth._R_to_quat(Z[None, :3, :3])[0]])
    return pkg.Graph(g.K, g.n_cams, g.n_objs, g.cam_fixed, g.bbox_cam, g.bbox_obj, g.bbox_meas, g.bbox_weight, g.e3d_cam, g.e3d_obj, g.e3d_meas,
                     g.e3d_weight, g.grav_obj, g.grav_normal, g.grav_weight, np.append(g.odom_i, i), np.append(g.odom_j, j),
                     np.concatenate([g.odom_meas.reshape(-1, 7), z7[None]]))


def child(a):
    pkg = importlib.import_module("object-oriented-slam_amd")
    g, c, o = load_graph(pkg, a.graph)
    ctx = pkg.Context(0)
    ctx.upload_graph(g); ctx.upload_states(c, o); ctx.snapshot_states()
    if a.solver == 4:
        ctx.set_pcg(rel_tol=a.rel_tol, check_every=a.check_every)
    p = pkg.default_lm_params(jacobian_mode=1, linear_solver=a.solver)
    for _ in range(a.warmup):
        ctx.restore_states(); ctx.optimize_resident(p)
    ctx.synchronize()
    its = trials = 0
    pcg_solves = pcg_iters = 0.0
    rep = None
    t0 = time.perf_counter()
    for _ in range(a.steps):
        ctx.restore_states()
        rep = ctx.optimize_resident(p)
        its += rep["iterations"]; trials += rep["total_trials"]
        if a.solver == 4:   # (one small read-back per step, inside the timed region: the counters restart with every run)
            st = ctx.lm_pcg_stats()
            pcg_solves += st["solves"]; pcg_iters += st["iterations_total"]
    ctx.synchronize()
    dt = time.perf_counter() - t0
    out = {"case": a.case, "linear_solver_requested": a.solver, "linear_solver_used": ctx.lm_solver_used(), "steps": a.steps, "warmup": a.warmup,
           "ms_per_trial": 1e3 * dt / max(trials, 1), "ms_per_optimize": 1e3 * dt / a.steps, "lm_iterations_per_s": its / dt,
           "lm_iterations_per_step": its / a.steps, "lm_trials_per_step": trials / a.steps, "chi2_initial": rep["chi2_initial"],
           "chi2_final": rep["chi2_final"], "stop_reason": rep["stop_reason"]}
    if a.solver == 4:
        st = ctx.lm_pcg_stats()
        out.update({"rel_tol": a.rel_tol, "check_every": a.check_every, "pcg_iterations_per_solve": pcg_iters / max(pcg_solves, 1),
                    "pcg_last_solve": {"iterations": st["iterations"], "rel_residual": st["rel_residual"], "converged": st["converged"]}})
    ctx.close()
    with open(a.result, "w") as f:
        json.dump(out, f)
    print(json.dumps(out))


def top_kernels(prof_dir, n=5):
    dbs = glob.glob(os.path.join(prof_dir, "**", "*_results.db"), recursive=True)
    if not dbs:
        return {"error": "no rocpd database under " + prof_dir}
    rows = sqlite3.connect(dbs[0]).execute("select name, total_calls, total_duration, average, percentage from top_kernels").fetchall()
    rows.sort(key=lambda r: -r[2])
    return [{"kernel": r[0].split("(")[0], "calls": r[1], "total_us": r[2], "average_us": r[3], "percent": r[4]} for r in rows[:n]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg_c3_c4.json"))
    ap.add_argument("--only", default=None, choices=["c3", "c4"])
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--steps", type=int, default=20); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--check-every", type=int, default=8)
    # child
    ap.add_argument("--child", action="store_true"); ap.add_argument("--case"); ap.add_argument("--graph"); ap.add_argument("--result")
    ap.add_argument("--solver", type=int, default=4); ap.add_argument("--rel-tol", type=float, default=1e-10)
    a = ap.parse_args()
    if a.child:
        return child(a)

    pkg = importlib.import_module("object-oriented-slam_amd")   # (numpy only: the parent never creates a context)
    tmp = tempfile.mkdtemp(prefix="measure_pcg_")
    runs = []
    result = {"device": "1 x MI355X", "jacobians": "analytic", "step": "optimize(10) on the resident graph", "runs": runs}
    try:
        plan = []
        for cfg in ("C3", "C4"):
            if a.only and a.only != cfg.lower():
                continue
            g, c, o, truth = pkg.synth.make_config(cfg, seed=0, slam=True)
            path = os.path.join(tmp, cfg + ".npz")
            save_graph(path, g, c, o)
            result[cfg.lower() + "_graph"] = {"cameras": g.n_cams, "ellipsoids": g.n_objs, "bbox_edges": len(g.bbox_cam), "e3d_edges": len(g.e3d_cam),
                                              "odometry_edges": len(g.odom_i)}
            budget = 120 if cfg == "C3" else 420
            plan += [(cfg.lower() + "_pcg_1e-8", path, 4, 1e-8, a.steps, a.warmup, budget), (cfg.lower() + "_pcg_1e-10", path, 4, 1e-10, a.steps, a.warmup, budget),
                     (cfg.lower() + "_auto", path, 0, 0.0, a.steps, a.warmup, budget)]
            if cfg == "C4":
                lp = os.path.join(tmp, "C4_loop.npz")
                save_graph(lp, with_loop_closure(pkg, g, truth, 3, g.n_cams - 1), c, o)
                plan += [("c4_loop_closure_pcg_1e-10", lp, 4, 1e-10, a.steps, a.warmup, budget), ("c4_loop_closure_reduced_camera", lp, 1, 0.0, 2, 1, 600)]
        me = os.path.abspath(__file__)
        for case, path, solver, tol, steps, warmup, budget in plan:
            res = os.path.join(tmp, case + ".json")
            cmd = ["timeout", "-k", "10", str(budget), sys.executable, me, "--child", "--case", case, "--graph", path, "--result", res, "--solver", str(solver),
                   "--rel-tol", str(tol or 1e-10), "--steps", str(steps), "--warmup", str(warmup), "--check-every", str(a.check_every)]
            print("[measure_pcg]", case, flush=True)
            rc = subprocess.call(cmd)
            if rc != 0:   # a failed or timed-out GPU step ends the measurement: nothing else is started on that GPU
                result["aborted"] = {"case": case, "exit_status": rc}
                break
            runs.append(json.load(open(res)))
        if "aborted" not in result and not a.no_rocprof and a.only != "c3" and shutil.which("rocprofv3"):
            pd = os.path.join(tmp, "rocprof")
            res = os.path.join(tmp, "rocprof_child.json")
            cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "-d", pd, "--", sys.executable, me, "--child", "--case", "c4_pcg_1e-10_traced",
                   "--graph", os.path.join(tmp, "C4.npz"), "--result", res, "--solver", "4", "--rel-tol", "1e-10", "--steps", "3", "--warmup", "1",
                   "--check-every", str(a.check_every)]
            print("[measure_pcg] rocprofv3 kernel trace of c4_pcg_1e-10", flush=True)
            rc = subprocess.call(cmd, stdout=subprocess.DEVNULL)
            result["c4_pcg_top_kernels"] = top_kernels(pd) if rc == 0 else {"error": "rocprofv3 run ended with status %d" % rc}
            result["c4_pcg_top_kernels_note"] = "rocprofv3 --kernel-trace --stats, a run of its own (1 warm-up + 3 steps, no counters): all kernels of those optimize calls"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("[measure_pcg] wrote", a.out)
    return 1 if "aborted" in result else 0


if __name__ == "__main__":
    sys.exit(main())
