"""plan_windows on the CPU (no GPU needed): tests/native/window_plan_check.cpp
asks host/render_plan.cpp how a render is cut into sample windows -- window 0
is plan_chunk's one-shot plan for the BASELINE shapes, an explicit window is
rounded to a chunk multiple, the windows cover [0, spp) with only the last one
short, the auto window of a C4 share over 4 ranks keeps one sample per item
within the chunk-sum budget in both precisions, and no samples or no tiles
divide by nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_window_plans(tmp_path):
    exe = str(tmp_path / "window_plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "window_plan_check.cpp"),
                    os.path.join(CSRC, "host", "render_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("\n0 wrong")
