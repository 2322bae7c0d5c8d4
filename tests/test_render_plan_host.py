"""The render plan and the task list on the CPU (no GPU needed):
tests/native/plan_check.cpp stages scenes with host/stage_scene.cpp and asks
host/render_plan.cpp what a render of them would launch -- the world kernel,
its BVH width, stack and LDS, the chunk -- for scenes::simple at the defaults
and under the tuning keys that pick another kernel, a 64-light scene with the
light grid and with the light BVH, a textured scene, the 63 / 64 sphere
threshold of RTW_ACCEL_AUTO and a BVH deeper than the kernels' stack -- and
the kernel variant each launches (its option bits and the dynamic LDS the
launch passes) for those and for quad, cuboid and emissive scenes, the f32
option keys, forced brute force, with a sweep of the keys that must only ever
name a variant that exists; and
checks the invariants of the longest-tiles-first task list (every (tile,
chunk) once, in order, 12-bit chunk counts, costliest tiles first) over tile
counts, chunk counts, fixed groups and both sizing rules."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_UNITS = ("render_plan", "stage_scene", "bvh", "rtw_host")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@functools.lru_cache(maxsize=None)
def plan_check_exe():
    """tests/native/plan_check.cpp, compiled once per test run."""
    out = tempfile.mkdtemp(prefix="plan_check_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "plan_check.cpp"),
                    *[os.path.join(CSRC, "host", u + ".cpp") for u in HOST_UNITS], "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


@needs_hipcc
def test_plan_known_answers_and_task_list_invariants():
    r = subprocess.run([plan_check_exe()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("\n0 wrong")
