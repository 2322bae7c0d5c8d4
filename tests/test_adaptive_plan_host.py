"""Adaptive sampling on the CPU (no GPU needed): tests/native/adaptive_plan_check.cpp
asks host/render_adaptive.hpp where the passes end -- (min, window, max) = (4, 4,
32), (2, 1, 2), (5, 7, 20), (4, 4, 4) -- how a pass is cut into sub-passes under
a small partial_max, which arguments are rejected, and the stop rule on hand
cases: zero variance at tolerance 0, q - m*m slightly negative, n = 2, a mean
below the 2^-16 floor, NaN and +-inf sums.  Every case of the rule it evaluates
is printed and compared here with a numpy restatement (tests/adaptive_rule.py),
which the other adaptive tests use as their reference."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_rule as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_adaptive_plan_and_rule(tmp_path):
    exe = str(tmp_path / "adaptive_plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "adaptive_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("\n0 wrong")
    rules = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("RULE ")]
    lumas = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("LUMA ")]
    assert len(rules) > 300 and len(lumas) == 2
    seen = set()
    for s1, s2, n, tol, got in rules:
        s1, s2, tol = (np.float64(float.fromhex(v)) for v in (s1, s2, tol))
        want = bool(A.settled(s1, s2, int(n), tol))
        assert want == bool(int(got)), (s1, s2, n, tol, got)
        seen.add(want)
    assert seen == {True, False}
    # the library's pass ends against the restatement's (the cases of the issue among them)
    ends = {tuple(map(int, ln.split()[1:4])): list(map(int, ln.split()[4:]))
            for ln in r.stdout.splitlines() if ln.startswith("ENDS ")}
    assert {(4, 32, 4), (2, 2, 1), (5, 20, 7), (4, 4, 4)} <= set(ends)
    for (mn, mx, win), got in ends.items():
        if len(got) < 64:
            assert got == A.pass_ends(mn, mx, win), (mn, mx, win)
    for r_, g, b, y in lumas:
        rgb = np.array([float.fromhex(v) for v in (r_, g, b)])
        assert A.luma(rgb) == float.fromhex(y)

