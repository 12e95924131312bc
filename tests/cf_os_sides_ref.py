"""Helpers around tests/cf_os_sides_main.cpp, the host program that prints what the layout plan (csrc/esl_cf_plan.hpp) makes of the
one-sided assembly's pair list -- twins merged, the shorter side per block and segment -- and the same numbers in numpy from the
definitions.  Used by tests/test_cf_os_sides.py (CPU) and tests/test_gpu_cf_os_sides.py (the list the device built)."""
import os
import shutil
import subprocess

import numpy as np

from tests import cf_plan_ref

ROOT = cf_plan_ref.ROOT


def build(out_dir, sanitize=False):
    """compiles tests/cf_os_sides_main.cpp for the host, a program of its own; sanitize: with the address and undefined-behaviour sanitizers"""
    cxx = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"          # (the default of csrc/Makefile)
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        return None
    exe = os.path.join(str(out_dir), "cf_os_sides_main" + ("_san" if sanitize else ""))
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O2", "-Wall"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else [])
    p = subprocess.run(cmd + [os.path.join(ROOT, "tests", "cf_os_sides_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr.strip(), p.stderr
    return exe


def run(exe, L, work_dir, os_list=1, **switches):
    """what the program prints for lists L (cf_plan_ref.lists) at these switches: scalars as int, flops as float, arrays as int64"""
    sw = dict(cf_plan_ref.SWITCHES, **switches)
    path = os.path.join(str(work_dir), "cf_os_sides_input.txt")
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d\n" % (L["N"], L["nf"], L["EU"], L["chain_ok"], 0, 288 << 30))
        f.write(" ".join(str(int(sw[k])) for k in cf_plan_ref.SWITCHES) + "\n")
        for k in ("ue_start", "cu_start", "cu_obj", "cu_id"):
            f.write(" ".join(map(str, L[k].tolist())) + "\n")
    p = subprocess.run([exe, path, str(int(os_list))], capture_output=True, text=True)
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


SCALARS = "sparse form S nseg n_list os_npairs os_offsets os_list osm_npairs osm_row_npairs os_list_npairs too_large".split()


def definitions(L, S):
    """From the lists alone.  A run = the entries of one ellipsoid at one slot; its head = the first of them in (slot, u) order.
    run[k] (entries per ellipsoid by (slot, u)): length of the run whose head is entry k, interior slots only, else 0;
    heads / ent [segment, ellipsoid]: run heads / entries at interior slots; T's order (unrank: stable by first free camera)."""
    slot, obj, u, N, nf = L["ue_slot"], L["ue_obj"], L["ue_id"], L["N"], L["nf"]
    by = np.lexsort((u, slot, obj))
    slot, obj = slot[by], obj[by]
    nseg = -(-nf // S)
    interior = slot % S != S - 1
    key = obj * (nf + 1) + slot
    head = np.concatenate([[True], key[1:] != key[:-1]]) if key.size else np.zeros(0, bool)
    group = np.cumsum(head) - 1
    size = np.bincount(group) if key.size else np.zeros(0, np.int64)
    run = np.where(head & interior, size[group] if key.size else 0, 0)
    heads, ent = np.zeros((nseg, N), np.int64), np.zeros((nseg, N), np.int64)
    np.add.at(heads, ((slot // S)[head & interior], obj[head & interior]), 1)
    np.add.at(ent, ((slot // S)[interior], obj[interior]), 1)
    first = np.full(N, nf, np.int64)
    np.minimum.at(first, obj, slot)
    return dict(run=run, heads=heads, ent=ent, unrank=np.argsort(first, kind="stable"))


def block_matrices(heads):
    """per block [t1, t2] of T (heads in T's order): pairs of the merged list with the shorter side, with the row side; the shared
    segments where the column side is walked, where the two sides tie, where the row side is strictly shorter"""
    N = heads.shape[1]
    both, row, swapped, ties, rowside = (np.zeros((N, N), np.int64) for _ in range(5))
    for h in heads:
        h1, h2 = h[:, None], h[None, :]
        shared = (h1 > 0) & (h2 > 0)
        both += np.minimum(h1, h2); row += h1 * (h2 > 0)
        swapped += shared & (h2 < h1); ties += shared & (h2 == h1); rowside += shared & (h1 < h2)
    return both, row, swapped, ties, rowside
