"""The layout rules of csrc/esl_graph_layout.hpp (chunk table, slice capacities, free-camera slots, camera-side lists, edge
records) on the CPU: tests/graph_layout_main.cpp is compiled against the header with a plain C++ compiler -- the header
includes no HIP -- and what it prints is compared with the same rules restated here in numpy (a plain loop for the chunks,
a stable argsort for the lists).  esl_graph_upload, esl_graph_append and esl_graph_upload_fixed all lay their arrays out
with these helpers (csrc/esl_graph.hip); tests/test_gpu_streaming.py holds the three paths against each other on the device.

The graph is the smallest that reaches every boundary: three ellipsoids with 0 / 64 / 65 bbox edges and 0 / 32 / 33 3-D edges
(no chunk, exactly one full chunk, one full chunk + one edge)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BB_CNT, E3_CNT = [0, 64, 65], [0, 32, 33]
F = 5


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layout") / "graph_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "graph_layout_main.cpp"), "-o", exe])
    out = {}
    for ln in subprocess.check_output([exe]).decode().splitlines():
        name, _, vals = ln.partition(":")
        out[name] = [float(v) if "." in v else int(v) for v in vals.split()]
    return out


def slice_capacity(cnt, chunk):
    """doubled, + one chunk, rounded up to whole chunks"""
    return -(-(2 * cnt + chunk) // chunk) * chunk


def slices():
    bb_begin = np.concatenate([[0], np.cumsum([slice_capacity(n, 64) for n in BB_CNT])])
    e3_begin = np.concatenate([[0], np.cumsum([slice_capacity(n, 32) for n in E3_CNT])])
    return bb_begin, e3_begin   # (last entry: the extent of the arrays)


def chunk_table(bb_ranges, e3_ranges):
    obj, typ, beg, end, ostart, ids_bb, ids_e3 = [], [], [], [], [], [], []
    for o, ((b0, b1), (e0, e1)) in enumerate(zip(bb_ranges, e3_ranges)):
        ostart.append(len(obj))
        for t, lo, hi, step, ids in ((0, b0, b1, 64, ids_bb), (1, e0, e1, 32, ids_e3)):
            for b in range(lo, hi, step):
                ids.append(len(obj)); obj.append(o); typ.append(t); beg.append(b); end.append(min(b + step, hi))
    ostart.append(len(obj))
    return dict(obj=obj, type=typ, begin=beg, end=end, ostart=ostart, ids_bb=ids_bb, ids_e3=ids_e3)


def check_chunks(printed, tag, bb_ranges, e3_ranges, n_bbox, n_e3d):
    want = chunk_table(bb_ranges, e3_ranges)
    for k, v in want.items():
        assert printed[f"{tag}_{k}"] == [int(x) for x in v], (tag, k)
    cap = printed[f"{tag}_capacity"][0]
    assert cap == n_bbox // 64 + n_e3d // 32 + 2 * 3 + 2
    assert len(want["obj"]) <= cap
    return want


def test_chunk_table_compact_and_with_slack(printed):
    bs, es = np.concatenate([[0], np.cumsum(BB_CNT)]), np.concatenate([[0], np.cumsum(E3_CNT)])
    compact = check_chunks(printed, "compact", list(zip(bs[:-1], bs[1:])), list(zip(es[:-1], es[1:])), int(bs[-1]), int(es[-1]))
    # ellipsoid 0: nothing; 1: one full chunk of each type; 2: a full chunk + a chunk of one edge, bbox chunks first
    assert compact["ostart"] == [0, 0, 2, 6]
    assert compact["ids_bb"] == [0, 2, 3] and compact["ids_e3"] == [1, 4, 5]
    assert [e - b for b, e in zip(compact["begin"], compact["end"])] == [64, 32, 64, 1, 32, 1]
    bb_begin, e3_begin = slices()
    assert printed["bb_begin"] == list(bb_begin[:-1]) and printed["e3_begin"] == list(e3_begin[:-1])
    slack = check_chunks(printed, "slack", [(b, b + n) for b, n in zip(bb_begin, BB_CNT)], [(b, b + n) for b, n in zip(e3_begin, E3_CNT)],
                         int(bb_begin[-1]), int(e3_begin[-1]))
    # the same table: only the positions of the slices differ
    for k in ("obj", "type", "ostart", "ids_bb", "ids_e3"):
        assert slack[k] == compact[k], k
    assert [e - b for b, e in zip(slack["begin"], slack["end"])] == [e - b for b, e in zip(compact["begin"], compact["end"])]


def test_slice_capacity_rule(printed):
    want = []
    for n in (0, 1, 32, 33):
        want += [slice_capacity(n, 64), slice_capacity(n, 32)]
    assert want == [64, 32, 128, 64, 128, 96, 192, 128]   # (by hand)
    assert printed["slice_capacity"] == want


def camera_arrays():
    """the cameras of the edges at their slots of the slack layout (slack slots: -1), as graph_layout_main.cpp sets them"""
    bb_begin, e3_begin = slices()
    bb_cam, e3_cam = np.full(bb_begin[-1], -1), np.full(e3_begin[-1], -1)
    for o in range(3):
        for k in range(BB_CNT[o]):
            bb_cam[bb_begin[o] + k] = 0 if (k * 7 + o) % 3 == 0 else 1
        for k in range(E3_CNT[o]):
            e3_cam[e3_begin[o] + k] = 1 if (k * 5 + o) % 4 == 0 else 0
    return bb_cam, e3_cam


def csr(keys, values, n_keys):
    order = np.argsort(keys, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=n_keys))])
    return [int(x) for x in start], [int(x) for x in np.asarray(values)[order]]


def test_free_camera_slots(printed):
    # camera 0 fixed; 1 free with bbox / 3-D edges; 2 free, touched by the odometry edge (0, 2); 3 free without an edge; 4 free,
    # touched only through the extra flags; the odometry edge (0, 0) joins fixed cameras and touches nothing
    assert printed["slot"] == [-1, 0, 1, -1, 2] and printed["n_free"] == [3]
    assert printed["slot_no_extra"] == [-1, 0, 1, -1, -1] and printed["n_free_no_extra"] == [2]
    bb_cam, e3_cam = camera_arrays()
    fixed, touched = np.array([1, 0, 0, 0, 0], bool), np.zeros(F, bool)
    touched[bb_cam[bb_cam >= 0]] = True
    touched[e3_cam[e3_cam >= 0]] = True
    for i, j in ((0, 2), (0, 0)):
        if not (fixed[i] and fixed[j]):
            touched[[i, j]] = True
    touched[4] = True
    live = ~fixed & touched
    assert printed["slot"] == [int(x) for x in np.where(live, np.cumsum(live) - 1, -1)]


def test_camera_side_lists(printed):
    bb_cam, e3_cam = camera_arrays()
    for cam, sname, ename in ((bb_cam, "cbb_start", "cbb_edge"), (e3_cam, "ce3_start", "ce3_edge")):
        at = np.flatnonzero(cam >= 0)            # positions of the edges, ascending: ellipsoids ascend, arrival order inside one
        start, edge = csr(cam[at], at, F)
        assert printed[sname] == start and printed[ename] == edge
        assert all(edge[a:b] == sorted(edge[a:b]) for a, b in zip(start[:-1], start[1:]))
    od = np.array([[0, 2], [0, 0]])
    start, edge = csr(od.reshape(-1), np.arange(od.size), F)   # entry = edge * 2 + side
    assert printed["cod_start"] == start and printed["cod_edge"] == edge == [0, 2, 3, 1]


def test_csr_by_key_copy_edge_and_align(printed):
    key = np.array([2, 0, 2, 1, 0, 2, 2])
    start, perm = csr(key, np.arange(key.size), 3)
    assert printed["key_start"] == start and printed["key_perm"] == perm and printed["key_forms_agree"] == [1]
    for width in (4, 10):   # edge 2 of the source into slot 1: camera, ellipsoid, weight, `width` measurements; slot 0 untouched
        assert printed[f"copy_{width}"] == [7, 3, 0.125] + [-1] * width + list(range(2 * width, 3 * width))
    assert printed["align_up"] == [0, 256, 256]
