"""The task-order state machine and a pass's kernel parameters on the CPU (no
GPU needed): tests/native/lpt_state_check.cpp drives host/lpt_state.hpp through
tables of renders -- a cold context counts, reads back, then stays cached; each
key field recounts; a pilot; a dealt split's costs; a failed launch or
read-back recounts; when the task list is stale; which windows share a key --
and checks host/render_pass.hpp pass_params for one pass of each kind.  The
second build runs the same program under the address and undefined-behaviour
sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("sanitize", [False, True])
def test_lpt_state_and_pass_params(tmp_path, sanitize):
    exe = str(tmp_path / "lpt_state_check")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
             "-g"] if sanitize else []
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", *flags,
                    "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "lpt_state_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().split("\n")[-1] == "0 wrong"
