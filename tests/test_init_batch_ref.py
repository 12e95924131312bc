"""esl_init_quadrics without a device: the conditions that make the device comparison of tests/test_gpu_init_batch.py a fair demand,
the numpy statement's grouping and plane counts (tests/init_batch_ref.py), the exported symbol, and the host-side grouping header
(csrc/esl_init_group.hpp) under AddressSanitizer / UBSan in a stand-alone program."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_batch_ref as ib                      # noqa: E402
from test_init_quadric import K as K1            # noqa: E402

ROOT = ib.ROOT


def object_parts(s, o):
    sel = ib.group(s["obs_obj"], s["N"])[o]
    return s["cams"][s["obs_cam"][sel]], s["obs_boxes"][sel]


@pytest.mark.parametrize("name", list(ib.SCENES) + list(ib.LONG))
def test_scene_conditions(po, name):
    """Per object: sigma_10 / sigma_9 <= 0.1, shape-matrix eigenvalue ratio >= 1e-3, Q*^-1 eigenvalue ratio >= 1e-5 (1,000 times the
    1e-8 parity tolerance); and the numpy rows, built from Tcw directly, reproduce the oracle's Q* (which inverts Twc).  Bound of the
    latter: eps * kappa / (1 - sigma_10 / sigma_9) ~ 2.2e-16 * 6e3 / 0.9 = 1.5e-12 for the null vector, held with two orders of
    margin at 1e-10 of the largest entry."""
    s = ib.scene(name)
    _, Q, _, st = ib.scene_reference(name, 0)
    worst = [0.0, np.inf, np.inf]
    for o in range(s["N"]):
        Tcw, boxes = object_parts(s, o)
        A = ib.plane_rows(Tcw, boxes, s["K"])
        assert len(A) == st[o, 2] and len(Tcw) == st[o, 1]
        c = ib.assert_conditions(A, Q[o], (name, o))
        worst = [max(worst[0], c[0]), min(worst[1], c[1]), min(worst[2], c[2])]
        q = np.linalg.svd(A)[2][-1]
        q = q * np.sign(q[9])
        assert np.abs(q - ib.qhat(Q[o])).max() <= 1e-10 * np.abs(q).max(), (name, o)
    print(name, "worst sigma10/sigma9 %.3g, shape ratio %.3g, Q*^-1 ratio %.3g" % tuple(worst))


@pytest.mark.parametrize("i", range(len(ib.BOUNDARY)))
def test_boundary_lists_meet_the_conditions(i):
    one, refs, _ = ib.boundary_case(i)
    for f in (0, 1):
        _, Q, _, st = refs[f]
        assert list(st[0]) == [0, ib.BOUNDARY[i][3], 4 * ib.BOUNDARY[i][3]]   # initialised, every line kept
        ib.assert_conditions(ib.plane_rows(one["cams"][one["obs_cam"]], one["obs_boxes"], one["K"]), Q[0], ib.BOUNDARY[i])


def test_scene_facts():
    """what tests/test_gpu_init_batch.py relies on: observation counts, and that exactly object 12 of scene B is rejected, by both
    decompositions"""
    for name, lo, hi in (("A0", 12, 43), ("A1", 12, 43), ("B", 34, 162), ("L600", 141, 418), ("L1600", 519, 665)):
        for faithful in (0, 1):
            st = ib.scene_reference(name, faithful)[3]
            assert lo <= st[:, 1].min() and st[:, 1].max() <= hi, (name, st[:, 1].min(), st[:, 1].max())
            bad = [12] if name == "B" else []
            assert list(np.nonzero(st[:, 0])[0]) == bad and (st[bad, 0] == 3).all(), (name, faithful, st[:, 0])
    n1 = ib.scene_reference("A1", 1)[3][:, 1]
    assert (n1 < 15).any() and (n1 >= 15).any()   # min_observations = 15 splits scene A1


def test_grouping_is_stable_and_ignores_interleaving():
    s = ib.scene("A0")
    rng = np.random.default_rng(5)
    n = len(s["obs_obj"])
    base = ib.group(s["obs_obj"], s["N"])
    assert sorted(np.concatenate(base)) == list(range(n))
    for sel in base:
        assert (np.diff(sel) > 0).all()
    # deal the objects' entries out in another interleaving, each object's own order kept
    owner = rng.permutation(s["obs_obj"])
    nxt = {o: iter(sel) for o, sel in enumerate(base)}
    perm = np.array([next(nxt[o]) for o in owner])
    assert not np.array_equal(perm, np.arange(n))
    obj2 = s["obs_obj"][perm]
    assert np.array_equal(obj2, owner)
    for o, sel in enumerate(ib.group(obj2, s["N"])):
        assert np.array_equal(perm[sel], base[o])
    # skipped entries belong to nobody
    obj3 = s["obs_obj"].copy(); obj3[::3] = -1
    g3 = ib.group(obj3, s["N"])
    assert sum(len(x) for x in g3) == int((obj3 >= 0).sum())
    for o, sel in enumerate(g3):
        assert np.array_equal(sel, base[o][base[o] % 3 != 0])


def test_plane_counts_follow_the_border_rules(po):
    cases = ib.box_edit_cases()
    cams = np.concatenate([c[0] for c in cases])
    boxes = np.concatenate([c[1] for c in cases])
    obj = np.concatenate([np.full(len(c[0]), i) for i, c in enumerate(cases)])
    _, Q, err, st = ib.reference(cams, len(cases), np.arange(len(cams)), obj, boxes, K1)
    for i, (Tcw, B, m, ok) in enumerate(cases):
        assert len(ib.plane_rows(Tcw, B, K1)) == m == st[i, 2]
        assert ok == (m >= 9) and st[i, 0] == (0 if ok else 2) and st[i, 1] == len(B)
        assert Q[i].any() == ok
    # min_observations comes first and leaves the plane count at zero
    st = ib.reference(cams, len(cases), np.arange(len(cams)), obj, boxes, K1, min_observations=3)[3]
    assert list(st[:, 0]) == [1, 0, 0, 2, 2] and list(st[:, 2]) == [0, 12, 11, 8, 8]


def test_symbol_declared_listed_exported_and_null_ctx(pkg):
    txt = open(os.path.join(ROOT, "include", "esl.h")).read()
    assert re.search(r"\bint\s+esl_init_quadrics\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert "esl_init_quadrics" in pkg.lib.EXPORTS
    L = pkg.lib.load()
    assert hasattr(L, "esl_init_quadrics")
    assert L.esl_abi_version() == 5
    K = (ctypes.c_double * 4)(*K1)
    out = (ctypes.c_double * 10)()
    rc = L.esl_init_quadrics(None, None, ctypes.c_int32(0), ctypes.c_int32(1), None, None, None, ctypes.c_int64(0), K, ctypes.c_int32(480),
                             ctypes.c_int32(640), ctypes.c_int32(1), ctypes.c_int32(0), out, None, None, None)
    assert rc == 2   # ESL_ERR_INVALID


# ---- csrc/esl_init_group.hpp in a stand-alone program under the sanitizers ---------------------------------------------------------
@pytest.fixture(scope="module")
def group_prog(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/init_group_main.cpp"
    exe = str(tmp_path_factory.mktemp("init_group") / "init_group_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", exe,
                           os.path.join(ROOT, "tests", "init_group_main.cpp")])
    return exe


def run_group(exe, N, F, tile, min_obs, cam, obj):
    text = f"{N} {F} {tile} {min_obs} {len(cam)}\n" + "".join(f"{c} {o}\n" for c, o in zip(cam, obj))
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    rc, bad = (int(v) for v in lines[0].split()[1:])
    if rc:
        return rc, bad
    ints = lambda l: [int(v) for v in l.split()[1:]]   # noqa: E731
    return dict(offsets=ints(lines[1]), idx=ints(lines[2]), slab=ints(lines[3])[0], order=[ints(l) for l in lines[4:]])


def check_group(exe, N, F, tile, min_obs, cam, obj):
    got = run_group(exe, N, F, tile, min_obs, cam, obj)
    ref = ib.group(np.asarray(obj, int), N)
    cnt = [len(x) for x in ref]
    assert got["offsets"] == [0] + [int(v) for v in np.cumsum(cnt)]
    assert got["idx"] == [int(i) for sel in ref for i in sel]
    # the launch list: falling count, ties by rising index; the slab's rows in that order
    want = sorted(range(N), key=lambda o: (-cnt[o], o))
    assert [e[0] for e in got["order"]] == want
    at = 0
    for o, first, n, spill in got["order"]:
        assert first == got["offsets"][o] and n == cnt[o]
        if n > tile and n >= min_obs:
            assert spill == at
            at += n
        else:
            assert spill == -1
    assert got["slab"] == at
    return got


def test_group_header_matches_numpy(group_prog):
    rng = np.random.default_rng(11)
    check_group(group_prog, 0, 0, 4, 0, [], [])                                 # nothing at all
    check_group(group_prog, 5, 3, 4, 0, [], [])                                 # an empty list
    check_group(group_prog, 5, 3, 4, 0, [0, 1, 2, 7, -4], [-1, -1, -2, -1, -1])   # all skipped: their frames are not looked at
    check_group(group_prog, 4, 9, 4, 0, list(range(9)), [2] * 9)                # one object holds every entry
    got = check_group(group_prog, 4, 9, 4, 10, list(range(9)), [2] * 9)         # ... and is below min_observations: no slab
    assert got["slab"] == 0
    for _ in range(5):
        N, F, n = int(rng.integers(1, 40)), int(rng.integers(1, 30)), int(rng.integers(0, 400))
        obj = rng.integers(-3, N, n)
        check_group(group_prog, N, F, int(rng.integers(1, 12)), int(rng.integers(0, 6)), rng.integers(0, F, n), obj)
    s = ib.scene("B")
    check_group(group_prog, s["N"], len(s["cams"]), 96, 0, s["obs_cam"], s["obs_obj"])


def test_group_header_rejects_bad_indices(group_prog):
    assert run_group(group_prog, 3, 2, 4, 0, [0, 1, 2], [0, 1, 2]) == (1, 2)     # obs_cam >= F
    assert run_group(group_prog, 3, 2, 4, 0, [0, -1, 1], [0, 1, 2]) == (1, 1)    # obs_cam < 0
    assert run_group(group_prog, 3, 2, 4, 0, [0, 1, 1], [0, 3, 2]) == (2, 1)     # obs_obj >= N
    assert isinstance(run_group(group_prog, 3, 2, 4, 0, [5, 1], [-1, 2]), dict)  # a skipped entry's frame is not checked
