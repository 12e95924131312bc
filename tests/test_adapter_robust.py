"""The adapter reads the robust-kernel config keys (Optimizer.Edges.2D.RobustKernel / RobustDelta, the knob for the line
Optimizer.cpp:224 leaves commented out): the Tracking-shaped replay of test_adapter_link.py, linked with a translation unit that
sets Optimizer.Edges.2D.RobustKernel = 1 (Huber), delta 1, must return what the C-ABI returns after set_robust(bbox=("huber", 1.0))
-- in mapping and in SLAM mode -- and what it returns without the kernel differs."""
import os
import subprocess

import numpy as np
import pytest

from tests import test_adapter_link as tal


def build_robust(tmp_path):
    exe = str(tmp_path / "tracking_calls_robust")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror=return-type", "-DESL_BUILD_IN_REFERENCE_TREE", "-I", tal.STUBS,
           "-I", os.path.join(tal.ROOT, "include"), "-I", os.path.join(tal.ROOT, "adapter")]
    cmd += [os.path.join(tal.ROOT, "adapter", a) for a in tal.ADAPTERS]
    cmd += [os.path.join(tal.STUBS, "tracking_calls.cpp"), os.path.join(tal.STUBS, "robust_config.cpp")]
    cmd += ["-L", tal.CSRC, "-lesl_hip", "-Wl,-rpath," + tal.CSRC, "-pthread", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_adapter_with_robust_keys_links(tmp_path):
    exe = build_robust(tmp_path)
    syms = subprocess.check_output(["nm", "-C", exe]).decode()
    assert "esl_lm_set_robust" in syms and "esl_edge_chi2" in syms


@pytest.mark.gpu
def test_adapter_robust_keys_replay_matches_c_abi(pkg, ctx, tmp_path, monkeypatch):
    # the replay of test_adapter_link.py, its binary built with the robust keys set and its C-ABI side driven with the same kernel
    monkeypatch.setattr(tal, "build", build_robust)
    ran = {}
    real_optimize = type(ctx).optimize

    def optimize_robust(self, graph, cams, objs, params=None):
        self.set_robust(bbox=("huber", 1.0))
        try:
            out = real_optimize(self, graph, cams, objs, params)
            ran.setdefault("weights", []).append(self.edge_chi2("bbox")[1])
            plain = pkg.Context(0)
            try:
                ran.setdefault("plain", []).append(real_optimize(plain, graph, cams, objs, params)[1])
            finally:
                plain.close()
            ran.setdefault("robust", []).append(out[1])
            return out
        finally:
            self.set_robust()
    monkeypatch.setattr(type(ctx), "optimize", optimize_robust)
    tal.test_adapters_replay_tracking_sequence_on_gpu(pkg, ctx, tmp_path)
    assert len(ran["robust"]) == 2                              # mapping and SLAM mode
    for w in ran["weights"]:
        assert np.any(w < 1.0)                                  # the kernel down-weighted something ...
    for a, b in zip(ran["robust"], ran["plain"]):
        assert np.abs(a - b).max() > 1e-9                       # ... and the adapter's answer (equal to the robust one) is not the plain one
