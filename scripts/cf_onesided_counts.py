"""Counts behind the one-sided assembly of T's interior part (esl_cf.hpp, form 3; profiles/cf_onesided_c4.md), on the CPU:
segments of 16 free-camera slots whose last slot is the separator; a list entry = one bbox or 3-D edge of an ellipsoid at a free
camera (slot = camera - 1: camera 0 is the fixed one).

    python scripts/cf_onesided_counts.py [C4]
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    pkg_synth = importlib.import_module("object-oriented-slam_amd.synth")
    name = sys.argv[1] if len(sys.argv) > 1 else "C4"
    g, _, _, _ = pkg_synth.make_config(name, slam=True)
    cam = np.concatenate([g.bbox_cam, g.e3d_cam]).astype(np.int64)
    obj = np.concatenate([g.bbox_obj, g.e3d_obj]).astype(np.int64)
    free = cam > 0
    slot, obj = cam[free] - 1, obj[free]
    interior = slot % 16 != 15
    seg = slot // 16
    nseg = int((g.n_cams - 1 + 15) // 16)
    key = seg[interior] * g.n_objs + obj[interior]
    uniq, n_ent = np.unique(key, return_counts=True)             # live (segment, ellipsoid) and its interior entries
    per_seg = np.bincount(uniq // g.n_objs, minlength=nseg).astype(np.float64)
    pair_segments = float((per_seg * (per_seg + 1) / 2).sum())   # blocks on and below the diagonal, per shared segment
    # entry-products: every entry of o1 meets every o2 of the segment at or below it in T's order; the mean over the triangle is
    # entries x (count + 1) / 2 up to the order inside the segment
    ent_seg = np.bincount(uniq // g.n_objs, weights=n_ent, minlength=nseg)
    entry_products = float((ent_seg * (per_seg + 1) / 2).sum())
    same_cam = np.unique(slot[interior] * g.n_objs + obj[interior]).size
    print(f"{name}: cameras {g.n_cams}, ellipsoids {g.n_objs}, list entries {slot.size} ({int(interior.sum())} interior)")
    print(f"  segments {nseg}, live (ellipsoid, segment) {uniq.size}, live ellipsoids per segment {per_seg.mean():.1f}")
    print(f"  entries per live (ellipsoid, segment): mean {n_ent.mean():.3f}, max {n_ent.max()}; "
          f"distinct (ellipsoid, camera) {same_cam} of {int(interior.sum())} interior entries")
    print(f"  interior entries per ellipsoid {interior.sum() / g.n_objs:.1f} on {uniq.size / g.n_objs:.1f} segments")
    print(f"  pair-segments {pair_segments:.4g}, entry-products {entry_products:.4g} "
          f"({entry_products / pair_segments:.3f} per pair-segment), Y reads {entry_products * 432 / 1e9:.1f} GB, "
          f"Y {uniq.size * 15 * 432 / 1e9:.2f} GB")


if __name__ == "__main__":
    main()
