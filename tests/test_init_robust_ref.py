"""esl_init_quadrics_robust without a device: the sampler (Python against csrc/esl_init_sample.hpp in a stand-alone program, plain and
under AddressSanitizer / UBSan), the numpy statement (tests/init_robust_ref.py) on the planted scenes -- it recovers exactly the planted
sets, where the plain initialisation rejects objects --, its visibility predicate against tests/assoc2d_ref.py, and the exported symbol."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc2d_ref as a2            # noqa: E402
import init_batch_ref as ib         # noqa: E402
import init_robust_ref as rr        # noqa: E402

ROOT = ib.ROOT
SCENES = ("A0", "A1", "B")
RECOVERED = {"A0": 12, "A1": 11, "B": 24}   # planted objects, every one recovered exactly


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------
def test_sampler_indices_distinct_in_range_and_repeatable():
    for seed in (0, 1, 0xDEADBEEFCAFEF00D):
        for s in (3, 5, 16):
            for n in (1, 2, s - 1, s, s + 1, s + 2, 17, 100, 1000):
                if n <= s:
                    assert rr.n_hypotheses(n, s, 64) == 1
                    assert rr.sample(seed, 0, n, s) == list(range(n))
                    continue
                assert rr.n_hypotheses(n, s, 64) == 64
                for h in (0, 1, 63, 1023):
                    loc = rr.sample(seed, h, n, s)
                    assert len(loc) == s == len(set(loc)) and loc == sorted(loc) and 0 <= loc[0] and loc[-1] < n
                    assert loc == rr.sample(seed, h, n, s)
    # the stream is (seed, h, k) alone, and different hypotheses differ
    assert rr.mix(0, 0, 0) == rr.mix(0, 0, 0) != rr.mix(0, 0, 1) != rr.mix(0, 1, 0) != rr.mix(1, 0, 0)
    assert len({tuple(rr.sample(0, h, 40, 5)) for h in range(64)}) > 60
    # every index can be drawn: Floyd's sampling is uniform over the subsets
    seen = set()
    for h in range(1024):
        seen.update(rr.sample(0, h, 30, 5))
    assert seen == set(range(30))


def build_sample_prog(tmp, flags):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/init_sample_main.cpp"
    exe = str(tmp / "init_sample_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", *flags, "-o", exe, os.path.join(ROOT, "tests", "init_sample_main.cpp")])
    return exe


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan_ubsan"])
def test_sample_header_matches_python(tmp_path, flags):
    exe = build_sample_prog(tmp_path, flags)
    for seed, s, H, ns in ((0, 5, 64, [0, 1, 4, 5, 6, 7, 15, 43, 300]), (2 ** 64 - 1, 16, 7, [3, 16, 17, 18, 64, 2 ** 31 - 1]),
                           (12345678901234567890, 3, 1024, [4, 9])):
        r = subprocess.run([exe], input=f"{seed} {s} {H} {len(ns)}\n" + " ".join(map(str, ns)) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        want = []
        for n in ns:
            for h in range(rr.n_hypotheses(n, s, H)):
                loc = rr.sample(seed, h, n, s)
                want.append(" ".join(map(str, [n, h, len(loc)] + loc)))
            want.append(f"mix {n} {rr.mix(seed, n, 0)}")
        assert r.stdout.splitlines() == want, (seed, s, H)


# ---- the numpy statement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES + ("LONG",))
def test_reference_recovers_the_planted_set(name):
    s, ref = rr.planted_scene(name), rr.scene_reference(name)
    done = 0
    for o, sel in enumerate(ib.group(s["obs_obj"], s["N"])):
        if not s["planted"][sel].any():
            assert len(sel) < 15
            continue
        done += 1
        assert ref["stats"][o, 0] == 0, (name, o, ref["stats"][o])
        assert np.array_equal(ref["inliers"][sel] == 1, ~s["planted"][sel]), (name, o)
        assert ref["stats"][o, 4] == int((~s["planted"][sel]).sum())
    print(name, "planted objects recovered exactly:", done)
    assert done == (1 if name == "LONG" else RECOVERED[name])
    if name == "LONG":
        assert ref["stats"][0].tolist()[:5] == [0, 300, ref["stats"][0, 2], 1, 255] and ref["stats"][0, 7] == 1


def test_the_plain_initialisation_fails_on_the_planted_lists():
    counts = {}
    for name in SCENES:
        s = rr.planted_scene(name)
        st = ib.reference(s["cams"], s["N"], s["obs_cam"], s["obs_obj"], s["obs_boxes"], s["K"], faithful=0)[3]
        counts[name] = int((st[:, 0] == 3).sum())
    print("objects the plain SVD initialisation rejects:", counts)
    assert counts["A0"] >= 3


def test_visibility_restatement_equals_assoc2d_ref(po):
    """init_robust_ref.visible is assoc2d_ref.visible over all rows at once: compared on every entry of scene A0 under each object's
    reference ellipsoid and under ellipsoids moved so that the predicate fails in each of its ways"""
    s, ref = rr.planted_scene("A0"), rr.scene_reference("A0")
    seen = set()
    for o, sel in enumerate(ib.group(s["obs_obj"], s["N"])):
        Tcw = np.array(s["cams"][s["obs_cam"][sel]])
        for e in (ref["ellipsoids"][o], np.concatenate([ref["ellipsoids"][o][:7], [30.0, 30.0, 30.0]]),
                  np.concatenate([ref["ellipsoids"][o][:3] + [40.0, 0, 0], ref["ellipsoids"][o][3:]])):
            bb = np.array([a2.raw_box(T, e, s["K"]) for T in Tcw])
            got = rr.visible(Tcw, e, s["K"], bb)
            want = np.array([a2.visible(T, e, s["K"], ib.ROWS, ib.COLS, []) for T in Tcw])
            assert np.array_equal(got, want), o
            seen.update(want.tolist())
            ob = np.array([po.project_bbox(T, e, s["K"]) for T in Tcw])
            fin = np.isfinite(bb).all(axis=1)
            assert np.array_equal(fin, np.isfinite(ob).all(axis=1))
            assert np.allclose(ob[fin], bb[fin], rtol=1e-9, atol=1e-9)
    assert seen == {True, False}


def test_statuses_of_the_reference():
    s = rr.planted_scene("A0")
    sel = ib.group(s["obs_obj"], s["N"])[2]
    one = dict(cams=s["cams"], N=1, obs_cam=s["obs_cam"][sel], obs_obj=np.zeros(len(sel), np.int32), obs_boxes=s["obs_boxes"][sel], K=s["K"])
    call = lambda d, **kw: rr.reference(d["cams"], d["N"], d["obs_cam"], d["obs_obj"], d["obs_boxes"], d["K"], **kw)   # noqa: E731
    assert call(one, min_observations=len(sel) + 1)["stats"][0].tolist() == [1, len(sel), 0, 0, 0, 0, -1, 0]
    assert call(one, p=dict(min_inliers=len(sel) + 1))["stats"][0, 0] == 5
    b = one["obs_boxes"][:12].copy(); b[:, 1:] = -5.0           # one kept line per entry: 12 planes, no sample of 5 reaches 9
    four = dict(one, obs_cam=one["obs_cam"][:12], obs_obj=one["obs_obj"][:12], obs_boxes=b)
    assert call(four)["stats"][0].tolist() == [4, 12, 12, 0, 0, 0, -1, 0]
    two = dict(one, obs_cam=one["obs_cam"][:2], obs_obj=one["obs_obj"][:2], obs_boxes=one["obs_boxes"][:2])
    assert call(two)["stats"][0].tolist() == [2, 2, 8, 0, 0, 0, -1, 0]


# ---- the symbol ------------------------------------------------------------------------------------------------------------------------
def test_symbol_declared_listed_exported_and_struct_size(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esl.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+esl_init_quadrics_robust\s*\(", txt) and re.search(r"\}\s*esl_init_robust_params\s*;", txt)
    assert {"esl_init_quadrics_robust", "esl_init_robust_params_default"} <= set(pkg.lib.EXPORTS)
    L = pkg.lib.load()
    assert hasattr(L, "esl_init_quadrics_robust") and L.esl_abi_version() == 5
    assert ctypes.sizeof(pkg.abi.EslInitRobustParams) == 32
    p = pkg.abi.EslInitRobustParams(sample_size=-1, n_hypotheses=-1, inlier_px=-1, min_inliers=-1, refine=-1, seed=99)
    L.esl_init_robust_params_default(ctypes.byref(p))
    d = pkg.abi.default_init_robust_params()
    assert [(getattr(p, f), getattr(d, f)) for f, _ in p._fields_] == [(v, v) for v in (5, 64, 10.0, 8, 1, 0)]
    K = (ctypes.c_double * 4)(500, 500, 320, 240)
    out = (ctypes.c_double * 10)()
    rc = L.esl_init_quadrics_robust(None, None, ctypes.c_int32(0), ctypes.c_int32(1), None, None, None, ctypes.c_int64(0), K,
                                    ctypes.c_int32(480), ctypes.c_int32(640), ctypes.c_int32(1), ctypes.c_int32(0), None, out, None, None,
                                    None, None, None, None)
    assert rc == 2   # ESL_ERR_INVALID: no context
