"""The numpy statement of esl_relocalize (tests/reloc_ref.py) on the CPU: it must find the true pose and the true association on
the synthetic frames, behave as the interface says on the small hand-made rooms, and the scenes the device tests reuse must be
well conditioned -- no compared quantity within 1e-9 (relative) of its threshold, the winner ahead of the runner-up in the inlier
count or by more than 1e-9 (relative) in cost -- so that exact agreement of the integers is a fair demand on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reloc_ref as rr        # noqa: E402
import reloc_scenes as rs     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(sc, **over):
    p = dict(sc["params"]); p.update(over)
    return rr.relocalize(sc["map"], sc["map_labels"], sc["ground_world"], sc["det"], sc["det_labels"], sc["ground_cam"], p)


def pose_error(sc, Twc):
    R = rs._quat_to_R(Twc[3:7])
    ang = np.arccos(np.clip((np.trace(R.T @ sc["Rwc"]) - 1) / 2, -1, 1))
    return float(np.linalg.norm(Twc[:3] - sc["twc"])), float(ang)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("refine", [0, 1])
def test_synth_frames_recovered(pkg, seed, refine):
    sc = rs.synth_scene(pkg, seed)
    r = run(sc, refine=refine)
    rs.check_conditions(r)
    D = len(sc["det"])
    terr, aerr = pose_error(sc, r["Twc"])
    print(f"seed {seed} refine {refine}: D {D} P {r['n_candidates']} hypotheses {r['n_hypotheses']} inliers {r['n_inliers']} "
          f"translation error {terr * 100:.2f} cm rotation error {np.degrees(aerr):.3f} deg margin {r['margin']:.2e} "
          f"runner gap {r['runner_gap']:.2e}")
    assert r["status"] == 0 and r["n_inliers"] == D and r["refined"] == refine
    assert terr < rr.DEFAULTS["center_tol"]
    assert aerr < 0.1
    assert np.array_equal(r["assoc"], sc["true_obj"])


def test_gravity_frame_is_a_rotation_and_picks_the_smallest_axis():
    for axis, k in (("z", 0), ("y", 2), ("x", 1)):
        n = np.array(rs.TILTS[axis])
        A, d = rr.gravity_frame(np.concatenate([3 * n, [1.5]]))
        assert np.allclose(A @ A.T, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(A), 1)
        assert np.allclose(A[2], n / np.linalg.norm(n)) and np.isclose(d, 0.5 / np.linalg.norm(n))
        assert int(np.argmin(np.abs(n))) == k and abs(A[0, k]) < 1e-15   # u = e_k x n has no e_k component
    assert int(np.argmin(np.abs(np.array([0.0, 0.0, 1.0])))) == 0        # ties: lowest k


def test_small_rooms():
    sc = rs.room_scene(3, [1, 1], [0, 1])
    r = run(sc, min_inliers=2)
    assert (r["status"], r["n_candidates"], r["n_hypotheses"], r["best_key"], r["n_inliers"], r["refined"]) == (0, 2, 1, 1, 2, 0)
    assert run(sc)["status"] == 2                                  # two inliers, three wanted
    one = rs.room_scene(3, [1, 1], [0])
    assert run(one)["status"] == 1 and run(one)["n_candidates"] == 1
    none = rs.room_scene(3, [1, 1], [])
    assert run(none)["status"] == 1
    dis = dict(sc); dis["det_labels"] = sc["det_labels"] + 7
    r = run(dis)
    assert r["status"] == 1 and r["n_candidates"] == 0 and np.all(r["assoc"] == -1) and np.array_equal(r["Twc"], [0, 0, 0, 0, 0, 0, 1])

    sc = rs.decoy_scene()
    r = run(sc)
    rs.check_conditions(r)
    assert r["status"] == 0 and r["n_candidates"] == 4 and r["n_hypotheses"] >= 4 and r["n_inliers"] == 3
    assert np.array_equal(r["assoc"], [0, 1, 2]) and pose_error(sc, r["Twc"])[0] < 0.05
    assert run(sc, min_inliers=4)["status"] == 2
    r3 = run(sc, max_candidates=3)
    assert r3["status"] == 3 and r3["n_candidates"] == 4 and r3["n_hypotheses"] == 0 and r3["best_key"] == -1

    sc = rs.repeated_scene()
    r = run(sc)
    rs.check_conditions(r)
    assert r["status"] == 0 and list(r["assoc"]) == [0, -1, 2, 4] and r["n_inliers"] == 3

    sc = rs.open_gates_scene()
    r = run(sc)
    rs.check_conditions(r)
    assert r["status"] == 0 and np.array_equal(r["assoc"], sc["true_obj"]) and r["n_candidates"] > len(sc["det"])
    assert r["n_candidates"] > run(sc, match_labels=1)["n_candidates"]


@pytest.mark.parametrize("P", [63, 64, 65])
def test_candidate_count_scenes(P):
    sc = rs.p_scene(P)
    r = run(sc)
    rs.check_conditions(r)
    assert r["status"] == 0 and r["n_candidates"] == P and np.array_equal(r["assoc"], sc["true_obj"])


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_tilted_ground(axis):
    sc = rs.tilted_scene(axis)
    r = run(sc)
    rs.check_conditions(r)
    terr, aerr = pose_error(sc, r["Twc"])
    assert r["status"] == 0 and np.array_equal(r["assoc"], sc["true_obj"]) and terr < 0.05 and aerr < 0.02


def test_library_defaults_match_the_reference(pkg):
    """esl_reloc_params_default needs no device: the library, the ctypes mirror and the numpy statement agree on the defaults"""
    import ctypes
    p = pkg.abi.EslRelocParams()
    pkg.lib.load().esl_reloc_params_default(ctypes.byref(p))
    d = pkg.abi.default_reloc_params()
    assert ctypes.sizeof(p) == 48 and ctypes.sizeof(pkg.abi.EslRelocResult) == 120
    for k, _ in pkg.abi.EslRelocParams._fields_:
        assert getattr(p, k) == getattr(d, k) == rr.DEFAULTS[k], k


def test_key_header_under_sanitizers(tmp_path):
    """csrc/esl_reloc_key.hpp (pair decode, winner order) is host-compilable: walk its boundaries under ASan + UBSan"""
    exe = str(tmp_path / "reloc_key")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "reloc_key_main.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert "reloc_key ok" in out, out
