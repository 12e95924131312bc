"""The stand-alone host programs of the dense map's headers (tests/dense_*_main.cpp), built for the tests/test_dense*_ref.py files: one
compiler search and one set of flags.  Nothing is preloaded into Python: the sanitizer build is a program of its own."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the two builds every header test runs in, for pytest.mark.parametrize("flags", BUILDS, ids=BUILD_IDS)
BUILDS = [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")]
BUILD_IDS = ["plain", "asan_ubsan"]


def build_prog(tmp, name, flags):
    """tests/<name>.cpp compiled into the directory `tmp`; the path of the program"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, f"a C++ compiler is needed to build tests/{name}.cpp"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, "-o", exe, os.path.join(ROOT, "tests", name + ".cpp")])
    return exe


NONFINITE = [float("nan"), float("inf"), float("-inf")]


def ladder_cases(defaults, rungs):
    """What a check function (csrc/esl_dense_check.hpp) is held to, as (values, expected text) pairs.  rungs: its refusals in the
    entry's order, each (text, accepted, refused): lists of updates of `defaults`, the accepted ones the last values that still pass, the
    refused ones the first that do not (refused[0] must still be refused with this text when a later rung's refused[0] is laid under it).
    The defaults pass; every accepted update passes; every refused one gives its text; with two rungs refused at once the earlier
    rung's text comes out, which pins the order."""
    cases = [(dict(defaults), "ok")]
    for text, accepted, refused in rungs:
        assert refused
        cases += [({**defaults, **a}, "ok") for a in accepted]
        cases += [({**defaults, **r}, text) for r in refused]
    for i, (text, _, refused) in enumerate(rungs):
        cases += [({**defaults, **later[0], **refused[0]}, text) for _, _, later in rungs[i + 1:]]
    return cases


def check_ladder(exe, fields, defaults, rungs, mode="check"):
    """mode "check" of a stand-alone program: one set of parameter values per line in (`fields` in the program's order; a float as
    its repr, which scanf reads back to the same double, "nan" and "inf" included), the refusal text or "ok" per line out"""
    cases = ladder_cases(defaults, rungs)
    lines = [" ".join(repr(v[f]) for f in fields) for v, _ in cases]
    out = subprocess.run([exe, mode], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[-1] == "" and len(out) == len(cases) + 1
    for (v, want), line, got in zip(cases, lines, out):
        assert got == want, (line, got, want)
