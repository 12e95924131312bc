"""Helpers around tests/cf_plan_main.cpp, the host program that prints the layout plan of the camera-first elimination
(csrc/esl_cf_plan.hpp): the lists of a graph in the order slam_alloc (esl_slam.hip) produces them, the program's input file, its build
and its output as a dict.  Used by tests/test_cf_plan.py (CPU) and tests/test_gpu_cf_stride.py (the plan the device ran)."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = dict(sparse=-1, tperm_off=0, no_nd=0, nd_min=48, stride=0, os_kernel=1)


def lists(g):
    """slam_alloc's lists of an uploaded graph.  The upload sorts each edge class by ellipsoid (stable); u = position of a bounding-box
    edge, n_bbox + position of a 3-D edge.  Per ellipsoid: its edges at FREE cameras, ascending u; per free-camera slot: the same edges
    sorted by (ellipsoid, u).  A free camera has a slot when an active edge touches it (esl_graph_layout.hpp free_camera_slots)."""
    fixed = np.zeros(g.n_cams, bool) if g.cam_fixed is None else g.cam_fixed.astype(bool)
    touched = np.zeros(g.n_cams, bool)
    touched[g.bbox_cam] = True; touched[g.e3d_cam] = True
    live = ~(fixed[g.odom_i] & fixed[g.odom_j])
    touched[g.odom_i[live]] = True; touched[g.odom_j[live]] = True
    slot_of = np.where(~fixed & touched, np.cumsum(~fixed & touched) - 1, -1)
    nf = int((slot_of >= 0).sum())
    bb, e3 = np.argsort(g.bbox_obj, kind="stable"), np.argsort(g.e3d_obj, kind="stable")
    obj = np.concatenate([g.bbox_obj[bb], g.e3d_obj[e3]]).astype(np.int64)
    slot = slot_of[np.concatenate([g.bbox_cam[bb], g.e3d_cam[e3]])]
    u = np.arange(obj.size)
    keep = slot >= 0
    obj, slot, u = obj[keep], slot[keep], u[keep]
    by_obj = np.argsort(obj, kind="stable")               # (u ascends inside an ellipsoid: bounding boxes first)
    obj, slot, u = obj[by_obj], slot[by_obj], u[by_obj]
    by_slot = np.argsort(slot, kind="stable")             # the per-ellipsoid lists walked in order and dealt to the cameras
    si, sj = slot_of[g.odom_i], slot_of[g.odom_j]
    both = (si >= 0) & (sj >= 0)
    chain = bool((np.abs(si[both] - sj[both]) == 1).all())
    return dict(N=g.n_objs, nf=nf, EU=len(g.bbox_obj) + len(g.e3d_obj), chain_ok=int(chain and nf > 0 and g.n_objs > 0),
                ue_start=np.concatenate([[0], np.cumsum(np.bincount(obj, minlength=g.n_objs))]), ue_slot=slot, ue_obj=obj, ue_id=u,
                cu_start=np.concatenate([[0], np.cumsum(np.bincount(slot, minlength=nf))]), cu_obj=obj[by_slot], cu_id=u[by_slot])


def build(out_dir, sanitize=False):
    """compiles tests/cf_plan_main.cpp for the host; sanitize: with the address and undefined-behaviour sanitizers"""
    cxx = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"          # (the default of csrc/Makefile)
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        return None
    exe = os.path.join(str(out_dir), "cf_plan_main" + ("_san" if sanitize else ""))
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O2", "-Wall"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else [])
    p = subprocess.run(cmd + [os.path.join(ROOT, "tests", "cf_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr.strip(), p.stderr
    return exe


def run(exe, L, work_dir, comm=0, total_mem=288 << 30, **switches):
    """the plan of lists L at these switches: scalars as int (flops: float), arrays as int64"""
    sw = dict(SWITCHES, **switches)
    path = os.path.join(str(work_dir), "cf_plan_input.txt")
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d\n" % (L["N"], L["nf"], L["EU"], L["chain_ok"], comm, total_mem))
        f.write(" ".join(str(int(sw[k])) for k in SWITCHES) + "\n")
        for k in ("ue_start", "cu_start", "cu_obj", "cu_id"):
            f.write(" ".join(map(str, L[k].tolist())) + "\n")
    p = subprocess.run([exe, path], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr.strip(), (p.returncode, p.stderr[-2000:])
    out = {}
    for line in p.stdout.splitlines():
        name, *vals = line.split()
        if name.endswith("_flops"):
            out[name] = float(vals[0])
        elif name in SCALARS:
            out[name] = int(vals[0])
        else:
            out[name] = np.array(vals, dtype=np.int64)
    return out


SCALARS = ("sparse form tperm nd stride n_sep n_seg S nseg nw n_chunks n_list ldx ldt kpad kpad_s n_fwork n_twork xc_len p_blocks prhs_len y_len "
           "os_npairs os_offsets too_large").split()


def solver_stats(pl):
    """esl_lm_solver_stats (include/esl.h) as the plan gives them"""
    sp, f3 = pl["sparse"], pl["sparse"] and pl["form"] == 3
    return [pl["form"] if sp else 0, pl["stride"], pl["n_sep"], pl["n_seg"],
            0.0 if not sp else pl["os_flops"] if f3 else 2.0 * pl["sp_flops"],
            0.0 if not sp else 8.0 * pl["y_len"] if f3 else 8.0 * 81.0 * pl["p_blocks"] if pl["form"] == 1 else 0.0,
            8.0 * pl["xc_len"] if sp else 0.0, pl["kpad_s"] if sp else pl["kpad"], pl["upd_flops"] if pl["tperm"] else 0.0, float(pl["tperm"])]
