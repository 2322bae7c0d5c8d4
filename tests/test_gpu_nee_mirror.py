"""The C++ host mirror's occluded / light_sample (host/ray_queries.cpp) against
the Python mirror on the same rays and origins: tests/native/nee_check.cpp,
linked with librtw.so, prints its questions and answers in hex floats."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_cpp_mirror_equals_the_python_mirror(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "nee_check")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "nee_check.cpp"), "-o", exe,
                    "-L", _capi.LIB_DIR, "-lrtw", "-Wl,-rpath," + _capi.LIB_DIR],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("ray ")]
    assert len(rows) == 96
    fl = float.fromhex
    rays = np.array([[fl(x) for x in r[1:7]] for r in rows])
    t_max = np.array([fl(r[8]) for r in rows])
    occ = np.array([[int(r[10]), int(r[11])] for r in rows], np.uint8)
    origins = np.array([[fl(x) for x in r[13:16]] for r in rows])
    dirs = np.array([[fl(x) for x in r[17:20]] for r in rows])
    pdf = np.array([fl(r[21]) for r in rows])
    light = np.array([int(r[23]) for r in rows], np.int32)
    soa, _ = rtw.scenes.simple_soa(0x5EED0001, 11)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        want_occ, want_inf = r.occluded(rays, t_max), r.occluded(rays)
        want_d, want_p, want_l = r.light_sample(origins, 7, 100, 2)
    assert 10 <= want_inf.sum() <= 86 and want_occ.sum() < want_inf.sum()
    assert np.array_equal(occ[:, 0], want_occ) and np.array_equal(occ[:, 1], want_inf)
    assert np.array_equal(light, want_l) and len(set(light.tolist())) >= 10
    for got, want in ((dirs, want_d), (pdf, want_p)):
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
