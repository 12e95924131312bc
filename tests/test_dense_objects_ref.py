"""The numpy statement of esl_dense_objects (tests/dense_objects_ref.py) held against independent checks, and csrc/esl_dense_obj.hpp --
the header the kernels and the host side compile -- held to hand-computed cases and to the statement (tests/dense_obj_main.cpp).  No GPU."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as dr                # noqa: E402
import dense_objects_ref as dor       # noqa: E402
import dense_scenes as sc             # noqa: E402
from dense_prog import build_prog          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = (0.0, 0.0, 1.0, 0.0)


def map_of(keys, leaf, labels, repeat=None, shuffle=0):
    """the statement's map of a voxel set placed through 1 x 1 frames (dense_objects_ref.voxel_frames), frames in a shuffled order"""
    s = dor.voxel_frames(keys, leaf, labels, repeat)
    idx = np.random.default_rng(shuffle).permutation(len(s["cams"]))
    m = dr.DenseMap(leaf=leaf, max_voxels=65536)
    m.add_frames(s["cams"][idx], s["K"], 1, 1, s["depth"][idx], s["bgr"][idx], s["inst"][idx])
    sc.check_conditions(m, two_frames=False)
    return m


def block(n, origin=(0, 0, 0)):
    k = np.stack(np.meshgrid(*[np.arange(c) for c in n], indexing="ij"), axis=-1).reshape(-1, 3)
    return k + np.array(origin)


def test_axis_aligned_block():
    """12 x 8 x 6 voxels at leaf 0.05 on the ground z = 0, plane_dist 0: centre, half-axes and yaw known in closed form"""
    keys = block((12, 8, 6))
    m = map_of(keys, 0.05, np.zeros(len(keys), int))
    e = m.extract()
    assert e["n_voxels"] == 576 and (e["key"] == keys[np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))]).all()
    r = dor.objects(e, 0.05, 1, FLOOR, plane_dist=0.0)
    assert r["result"] == dict(status=0, n_voxels=576, n_in_range=576, n_gated=576, n_kept=576, n_components_all=1, n_components=1, n_ok=1)
    assert r["stats"].tolist() == [[0, 576, 1, 0, 576, 576]] and r["comp"].tolist() == [[0, 576, 576, 0, 0, 0]]
    assert (r["voxel_comp"] == 0).all() and len(r["voxel_comp"]) == 576
    o = r["objs"][0]
    assert np.abs(o[:3] - [0.30, 0.20, 0.15]).max() <= 1e-12 and np.abs(o[7:] - [0.30, 0.20, 0.15]).max() <= 1e-12
    assert np.abs(o[3:7] - [0, 0, 0, 1]).max() <= 1e-12          # yaw 0
    assert r["margins"]["anisotropy"][0] > 0.3
    # plane_dist 0.05 drops the lowest layer (centres at 0.025): five layers, the centre moves up by half a voxel
    r = dor.objects(e, 0.05, 1, FLOOR)
    assert r["result"]["n_kept"] == 480 and np.abs(r["objs"][0][[2, 9]] - [0.175, 0.125]).max() <= 1e-12
    # the same block turned: 8 x 12 x 6, the long axis is y; x = -u = (0, 1, 0) or u = (0, -1, 0): yaw +-90 degrees
    keys = block((8, 12, 6), origin=(-20, 5, 0))
    r = dor.objects(map_of(keys, 0.05, np.zeros(len(keys), int)).extract(), 0.05, 1, FLOOR, plane_dist=0.0)
    o = r["objs"][0]
    assert np.abs(o[:3] - [-1.0 + 0.2, 0.25 + 0.3, 0.15]).max() <= 1e-12 and np.abs(o[7:] - [0.30, 0.20, 0.15]).max() <= 1e-12
    assert np.abs(np.abs(o[3:7]) - [0, 0, np.sqrt(0.5), np.sqrt(0.5)]).max() <= 1e-12 and o[6] > 0


def bfs_components(keys, lab, reach):
    """an independent labelling: breadth-first search over a dict of keys, all (2 reach + 1)^3 - 1 neighbours"""
    at = {tuple(k): i for i, k in enumerate(keys.tolist())}
    offs = [(x, y, z) for x in range(-reach, reach + 1) for y in range(-reach, reach + 1) for z in range(-reach, reach + 1) if (x, y, z) != (0, 0, 0)]
    comp = [-1] * len(keys)
    for s0 in range(len(keys)):
        if comp[s0] >= 0:
            continue
        comp[s0] = s0; todo = [s0]
        while todo:
            i = todo.pop()
            k = keys[i]
            for o in offs:
                j = at.get((k[0] + o[0], k[1] + o[1], k[2] + o[2]))
                if j is not None and comp[j] < 0 and lab[j] == lab[i]:
                    comp[j] = s0; todo.append(j)
    return np.array(comp)


@pytest.mark.parametrize("reach", [1, 2, 3])
@pytest.mark.parametrize("seed", [0, 1])
def test_components_against_breadth_first_search(seed, reach):
    rng = np.random.default_rng(seed)
    span = (14, 14, 10) if reach == 1 else (22, 22, 14) if reach == 2 else (30, 30, 18)
    keys = np.unique(rng.integers(-np.array(span) // 2, np.array(span) // 2, (700, 3)), axis=0)          # sorted lexicographically, negative keys too
    lab = rng.integers(0, 3, len(keys))
    root = dor.components(keys, lab, reach)
    want = bfs_components(keys, lab, reach)          # started in index order: the label IS the smallest index
    assert (root == want).all()
    sizes = np.unique(root, return_counts=True)[1]
    assert 5 < len(sizes) < len(keys) and sizes.max() >= 20          # neither dust nor one lump
    assert len(dor.half_offsets(reach)) == ((2 * reach + 1) ** 3 - 1) // 2 == {1: 13, 2: 62, 3: 171}[reach]
    offs = dor.half_offsets(reach)
    assert not set(offs) & {(-x, -y, -z) for x, y, z in offs}          # every pair from one side


@functools.lru_cache(maxsize=None)
def random_labelled_extract():
    """the extract of a map of four blocks and dust with three labels, unlabelled voxels and labels beyond N = 4; shared, not changed"""
    rng = np.random.default_rng(5)
    keys = np.unique(np.concatenate([block((9, 5, 4), (0, 0, 2)), block((4, 4, 4), (20, 0, 2)), block((4, 4, 4), (-20, 3, 2)),
                                     block((2, 2, 2), (0, 20, 2)), rng.integers(-30, 30, (60, 3))]), axis=0)
    lab = np.where(keys[:, 1] >= 15, 2, np.where(np.abs(keys[:, 0]) >= 15, 1, 0))
    lab[rng.random(len(keys)) < 0.05] = -1
    lab[-3:] = 7          # beyond N
    return map_of(keys, 0.05, lab).extract()


def test_statement_on_a_random_labelled_map():
    """the whole statement against the independent labelling: table order, statuses 0, 1, 2, voxel rows, caps, status 3"""
    e = random_labelled_extract()
    N = 4
    r = dor.objects(e, 0.05, N, FLOOR, reach=1, min_component=20)
    h = (e["key"][:, 2] + 0.5) * 0.05
    kept = (e["inst"] >= 0) & (e["inst"] < N) & (h >= 0.05)
    assert r["result"]["n_kept"] == kept.sum() and r["result"]["n_in_range"] == ((e["inst"] >= 0) & (e["inst"] < N)).sum()
    kc = bfs_components(e["key"].astype(np.int64)[kept], e["inst"][kept], 1)
    roots, size = np.unique(kc, return_counts=True)
    assert r["result"]["n_components_all"] == len(roots) and r["result"]["n_components"] == (size >= 20).sum() == len(r["comp"])
    t = r["comp"]
    assert (np.lexsort((dr.pack(t[:, 3:]), -t[:, 1], t[:, 0])) == np.arange(len(t))).all()          # label, size descending, key
    assert sorted(t[:, 1].tolist()) == sorted(size[size >= 20].tolist())
    assert r["stats"][:, 0].tolist() == [0, 0, 2, 1] and r["result"]["n_ok"] == 2          # label 2: eight voxels and dust; label 3: none
    assert r["stats"][1, 2] == 2 and r["stats"][1, 3] == 1 and r["stats"][0, 3] == 0 and t[:, 0].tolist() == [0, 1, 1] and t[1, 1] >= t[2, 1] >= 50
    assert (r["objs"][2:] == 0).all() and (r["objs"][:2, 7:] > 0).all()
    vc = r["voxel_comp"]
    assert ((vc == -1) == ~kept).all() and (vc == -2).sum() == size[size < 20].sum()
    for row in range(len(t)):
        assert (vc == row).sum() == t[row, 1] and (e["inst"][vc == row] == t[row, 0]).all()
        assert dr.pack(e["key"][vc == row]).min() == dr.pack(t[row, 3:])
    small = dor.objects(e, 0.05, N, FLOOR, reach=1, min_component=20, comp_cap=1, voxel_cap=10)
    assert small["comp"].tolist() == t[:1].tolist() and small["voxel_comp"].tolist() == vc[:10].tolist() and (small["objs"] == r["objs"]).all()
    over = dor.objects(e, 0.05, N, FLOOR, reach=1, min_component=20, max_components=len(t) - 1)
    assert over["result"] == dict(r["result"], status=3, n_ok=0)
    assert not over["objs"].any() and not over["stats"].any() and not over["comp"].any() and (over["voxel_comp"] == -1).all()
    assert len(over["comp"]) == len(t)
    assert dor.objects(dict(n_voxels=-1), 0.05, N, FLOOR)["result"] == dict(dict.fromkeys(dor.RESULT, 0), status=3, n_voxels=-1)


def test_guard_in_python_integers():
    assert dor.guard(1, 1 << 31) and not dor.guard(1, (1 << 31) - 1) and dor.guard(1 << 22, 1 << 20) and not dor.guard((1 << 22) - 1, 1 << 20)


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_listed_exported_and_struct_sizes(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esl.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+esl_dense_objects\s*\(", txt) and re.search(r"\}\s*esl_dense_obj_params\s*;", txt)
    assert re.search(r"\}\s*esl_dense_obj_result\s*;", txt)
    assert {"esl_dense_obj_params_default", "esl_dense_objects"} <= set(pkg.lib.EXPORTS)
    L = pkg.lib.load()
    assert hasattr(L, "esl_dense_objects")
    assert ctypes.sizeof(pkg.abi.EslDenseObjParams) == 32 and ctypes.sizeof(pkg.abi.EslDenseObjResult) == 32
    p = pkg.abi.EslDenseObjParams()
    L.esl_dense_obj_params_default(ctypes.byref(p))          # host code: runs without a device
    d = pkg.abi.default_dense_obj_params()
    for k, _ in pkg.abi.EslDenseObjParams._fields_:
        if k != "pad":
            assert getattr(p, k) == getattr(d, k) == dor.DEFAULTS[k], k
    assert callable(pkg.Context.dense_objects)


# ---- the header against hand-computed cases and the statement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan_ubsan"])
def test_obj_header_matches_the_statement(tmp_path, flags):
    exe = build_prog(tmp_path, "dense_obj_main", flags)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "dense_obj ok"
    # the guard's predicate around its boundary, against Python's integers
    cases = []
    for span in (1, 2, 3, 1000, (1 << 20) - 1, 1 << 20, (1 << 21) + 1, 46341, (1 << 31) - 1, 1 << 31):
        edge = -(-dor.GUARD // (span * span))          # the smallest n with n span^2 >= 2^62
        cases += [(n, span) for n in (1, edge - 1, edge, edge + 1, 1 << 26) if n >= 1]
    out = subprocess.run([exe, "guard"], input="".join(f"{n} {s}\n" for n, s in cases), capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [int(dor.guard(n, s)) for n, s in cases] and 0 < sum(int(x) for x in out) < len(cases)
    # frames and rows of random components on a tilted plane
    rng = np.random.default_rng(3)
    ground, leaf = (0.1, -0.2, 1.0, 0.3), 0.05
    pl = dor.plane(ground)
    lines, want = [], []
    for _ in range(40):
        k = np.unique(rng.integers(-40, 40, (rng.integers(1, 60), 3)) * rng.integers(1, 4, 3), axis=0).astype(np.int64)
        _, _, mom = dor.moments(k)
        x, y, z, _ = dor.frame(pl, len(k), mom)
        pc = dor.centers(k, leaf)
        mn = [float(dor.proj(a, pc).min()) for a in (x, y, z)]; mx = [float(dor.proj(a, pc).max()) for a in (x, y, z)]
        c = [(mn[a] + mx[a]) / 2 for a in range(3)]
        t = [(x[a] * c[0] + y[a] * c[1]) + z[a] * c[2] for a in range(3)]
        q = dor.quat([x[0], y[0], z[0], x[1], y[1], z[1], x[2], y[2], z[2]])
        want.append(x + y + z + t + q + [(mx[a] - mn[a]) / 2 + leaf / 2 for a in range(3)])
        lines.append(" ".join([str(len(k))] + [str(v) for v in mom] + [repr(v) for v in mn + mx]))
    head = " ".join(repr(float(v)) for v in ground) + f" {leaf!r} {len(lines)}\n"
    out = subprocess.run([exe, "frames"], input=head + "\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    got = np.array([[float(v) for v in ln.split()] for ln in out.strip().split("\n")])
    assert got.shape == (40, 19) and np.abs(got - np.array(want)).max() <= 1e-13


# ---- steps 3 and 4 on the host: dobj_choose and dobj_status on a component table as the device leaves it -----------------------------------------
NO_BOX = [2**31 - 1] * 3 + [-2**31] * 3          # the box of an object without a chosen component, as the entry initialises it


def run_table(exe, N, labkept, table, kbox, comp_cap):
    """-> the program's output lines as {name: [ints]} and the list of its comp rows"""
    text = f"{len(table)} {N} {comp_cap}\n" + "".join(" ".join(str(int(v)) for v in row) + "\n" for row in [labkept] + list(table) + list(kbox))
    out = {"comp": []}
    for ln in subprocess.run([exe, "table"], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n"):
        name, *vals = ln.split()
        if name == "comp":
            out["comp"].append([int(v) for v in vals])
        else:
            out[name] = [int(v) for v in vals]
    return out


def device_table(e, N, reach, min_component, shuffle):
    """what k_dobj_table leaves and what k_dobj_box adds, from the independent labelling: rows (label, size, samples, the root's index in
    the sorted list, its key, 0) in a shuffled order, the kept voxels per label, and per label the box of its largest component"""
    kept = (e["inst"] >= 0) & (e["inst"] < N) & ((e["key"][:, 2] + 0.5) * 0.05 >= 0.05)
    ki = np.flatnonzero(kept)
    keys = e["key"].astype(np.int64)
    kc = bfs_components(keys[ki], e["inst"][ki], reach)
    rows, box = [], {}
    for root in np.unique(kc):
        mem = ki[kc == root]
        if len(mem) >= min_component:
            rows.append([int(e["inst"][ki[root]]), len(mem), int(e["count"][mem].sum()), int(ki[root]), *keys[ki[root]].tolist(), 0])
            box[int(ki[root])] = keys[mem].min(axis=0).tolist() + keys[mem].max(axis=0).tolist()
    labkept = [int((e["inst"][ki] == o).sum()) for o in range(N)]
    kbox = []
    for o in range(N):
        mine = [t for t in rows if t[0] == o]
        kbox.append(box[min(mine, key=lambda t: (-t[1], t[3]))[3]] if mine else NO_BOX)
    return [rows[i] for i in np.random.default_rng(shuffle).permutation(len(rows))], labkept, kbox


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan_ubsan"])
def test_table_choice_and_statuses_match_the_statement(tmp_path, flags):
    exe = build_prog(tmp_path, "dense_obj_main", flags)
    # the random labelled map: the component table and the per-object stats of the statement
    e, N = random_labelled_extract(), 4
    r = dor.objects(e, 0.05, N, FLOOR, reach=1, min_component=20)
    table, labkept, kbox = device_table(e, N, 1, 20, shuffle=11)
    R = len(table)
    assert R == len(r["comp"]) == 3 and [t[3] for t in table] != sorted(t[3] for t in table)          # handed over out of order
    got = run_table(exe, N, labkept, table, kbox, comp_cap=R)
    assert got["comp"] == r["comp"].tolist()
    st = r["stats"]
    assert got["status"] == st[:, 0].tolist() == [0, 0, 2, 1] and labkept == st[:, 1].tolist()
    assert got["nrows"] == st[:, 2].tolist() and got["chosen"] == st[:, 3].tolist()
    srt = [table[i] for i in got["order"]]
    assert [[t[0], t[1], t[2], *t[4:7]] for t in srt] == r["comp"].tolist() and got["rowroot"] == [t[3] for t in srt]
    assert [srt[c][1:3] if c >= 0 else [0, 0] for c in got["chosen"]] == st[:, 4:6].tolist()
    assert got["rowobj"] == [t[0] if got["chosen"][t[0]] == i else -1 for i, t in enumerate(srt)]
    assert (dr.pack(e["key"].astype(np.int64)[got["rowroot"]]) == dr.pack(r["comp"][:, 3:])).all()          # a row's root IS its key's voxel
    assert run_table(exe, N, labkept, table, kbox, comp_cap=1)["comp"] == r["comp"][:1].tolist()
    # a hand-built table of six rows, N = 6, comp_cap 4 < R.  Label 0: two rows of 50 voxels (the lower root, 7, wins over 40) and one of
    # 30; label 1: kept voxels, no row; label 2: nothing kept; labels 3 and 4: the box spans 2^21 keys, so 2^20 voxels trip the guard
    # (2^20 2^42 = 2^62) and 2^20 - 1 do not; label 5: an ordinary row
    big = 1 << 20
    table = [[5, 25, 60, 90, 1, 2, 3, 0], [0, 50, 70, 40, 4, 4, 4, 0], [3, big, big, 11, -5, 0, 0, 0], [0, 30, 30, 3, 0, 0, 1, 0],
             [0, 50, 55, 7, 0, 1, 1, 0], [4, big - 1, 2 * big, 12, 9, 9, 9, 0]]
    wide = [-big, 0, 0, big - 1, 5, 5]
    assert dor.guard(big, 2 * big) and not dor.guard(big - 1, 2 * big)
    got = run_table(exe, 6, [130, 5, 0, big, big - 1, 25], table, [[0, 0, 0, 9, 9, 9], NO_BOX, NO_BOX, wide, wide, [1, 2, 3, 4, 5, 6]], comp_cap=4)
    assert got == dict(order=[4, 1, 3, 2, 5, 0], rowroot=[7, 40, 3, 11, 12, 90], rowobj=[0, -1, -1, 3, 4, 5], chosen=[0, -1, -1, 3, 4, 5],
                       nrows=[3, 0, 0, 1, 1, 1], status=[0, 2, 1, 6, 0, 0],
                       comp=[[0, 50, 55, 0, 1, 1], [0, 50, 70, 4, 4, 4], [0, 30, 30, 0, 0, 1], [3, big, big, -5, 0, 0]])
    # no row at all (R = 0): kept labels have status 2; and no object at all (N = 0)
    got = run_table(exe, 3, [4, 0, 2], [], [NO_BOX] * 3, comp_cap=5)
    assert got == dict(order=[], rowroot=[], rowobj=[], chosen=[-1, -1, -1], nrows=[0, 0, 0], status=[2, 1, 2], comp=[])
    assert run_table(exe, 0, [], [], [], comp_cap=0) == dict(order=[], rowroot=[], rowobj=[], chosen=[], nrows=[], status=[], comp=[])
