"""The render plan and the task list on the CPU (no GPU needed):
tests/native/plan_check.cpp stages scenes with host/stage_scene.cpp and asks
host/render_plan.cpp what a render of them would launch -- the world kernel,
its BVH width, stack and LDS, the chunk -- for scenes::simple at the defaults
and under the tuning keys that pick another kernel, a 64-light scene with the
light grid and with the light BVH, a textured scene, the 63 / 64 sphere
threshold of RTW_ACCEL_AUTO and a BVH deeper than the kernels' stack; and
checks the invariants of the longest-tiles-first task list (every (tile,
chunk) once, in order, 12-bit chunk counts, costliest tiles first) over tile
counts, chunk counts, fixed groups and both sizing rules."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_UNITS = ("render_plan", "stage_scene", "bvh", "rtw_host")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_plan_known_answers_and_task_list_invariants(tmp_path):
    exe = str(tmp_path / "plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "plan_check.cpp"),
                    *[os.path.join(CSRC, "host", u + ".cpp") for u in HOST_UNITS], "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("\n0 wrong")
