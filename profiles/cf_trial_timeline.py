#!/usr/bin/env python
"""One camera-first trial's reduced-system build as a timeline (rocprofv3 --kernel-trace, rocpd sqlite output): every launch between
a k_cf_gather_B and the end of the build -- the k_cf_T_gather that follows it (stored products) or, with the one-sided assembly
(k_cf_T_onesided), the k_chol_update_v that follows it --, start / end in us from the trial's first launch, and which pairs ran
side by side.  python profiles/cf_trial_timeline.py <results.db> [trial index, default: the middle one]"""
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
rows = db.execute("select name, grid_x, start, end from kernels order by start").fetchall()
rows = [(n.split("(")[0].replace("void ", "").replace("esl::", ""), g, s / 1e3, e / 1e3) for n, g, s, e in rows]
onesided = any(r[0].startswith("k_cf_T_onesided") for r in rows)
anchor_name, last_name = ("k_cf_T_onesided", "k_chol_update_v") if onesided else ("k_cf_seg_syrk", "k_cf_T_gather")
anchor = [i for i, r in enumerate(rows) if r[0].startswith(anchor_name)]
if not anchor:
    sys.exit("no k_cf_seg_syrk or k_cf_T_onesided launch in this trace")
longest = max(rows[i][3] - rows[i][2] for i in anchor)
live = [i for i in anchor if rows[i][3] - rows[i][2] > 0.25 * longest]   # (the small graphs of the other records run the same kernels)
pick = live[int(sys.argv[2]) if len(sys.argv) > 2 else len(live) // 2]
b = pick
while b > 0 and not rows[b][0].startswith("k_cf_gather_B"):
    b -= 1
e = pick
while e + 1 < len(rows) and not rows[e][0].startswith(last_name):
    e += 1
t0 = rows[b][2]
print("trial %d of %d with a full-size %s; us from the start of its k_cf_gather_B\n" % (live.index(pick), len(live), anchor_name))
print("| kernel | grid (threads) | start us | end us | us |")
print("|---|---|---|---|---|")
for n, g, s, t in rows[b:e + 1]:
    print("| `%s` | %d | %.1f | %.1f | %.1f |" % (n, g, s - t0, t - t0, t - s))
print("\nbuild, first start to last end: %.1f us\n" % (max(r[3] for r in rows[b:e + 1]) - t0))


def find(prefix, grid=None):
    return [r for r in rows[b:e + 1] if r[0].startswith(prefix) and (grid is None or r[1] == grid)]


def overlap(a, c):
    return max(0.0, min(a[3], c[3]) - max(a[2], c[2]))


if onesided:
    pairs = ((("k_cf_chain", 64), ("k_cf_forward<2", None)), (("k_cf_forward<1", None), ("k_cf_T_onesided", None)),
             (("k_cf_sep_rhs", None), ("k_cf_seg_back", None)), (("k_chol_update_v", None), ("k_cf_T_onesided", None)))
else:
    pairs = ((("k_cf_chain", 64), ("k_cf_forward<2", None)), (("k_cf_forward<1", None), ("k_cf_seg_syrk", None)),
             (("k_chol_update_v", None), ("k_cf_seg_syrk", None)), (("k_chol_update_v", None), ("k_cf_T_gather", None)))
for (pa, ga), (pc, gc) in pairs:
    for a in find(pa, ga):
        for c in find(pc, gc):
            print("%s [%.1f, %.1f] against %s [%.1f, %.1f]: %.1f us side by side" % (
                a[0], a[2] - t0, a[3] - t0, c[0], c[2] - t0, c[3] - t0, overlap(a, c)))
