"""The C++ host mirror's hit_rays / light_pdf (host/ray_queries.cpp) against
the Python mirror on the same rays: tests/native/ray_queries_check.cpp, linked
with librtw.so, prints its rays and answers in hex floats."""
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


def test_cpp_mirror_queries_equal_the_python_mirror(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "ray_queries_check")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "ray_queries_check.cpp"), "-o", exe,
                    "-L", _capi.LIB_DIR, "-lrtw", "-Wl,-rpath," + _capi.LIB_DIR],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("ray ")]
    assert len(rows) == 96
    fl = float.fromhex
    rays = np.array([[fl(x) for x in r[1:7]] for r in rows])
    ids = np.array([[int(x) for x in r[8:12]] for r in rows], np.int32)
    hits = np.array([[fl(x) for x in r[12:21]] for r in rows])
    pdf = np.array([fl(r[22]) for r in rows])
    soa, _ = rtw.scenes.simple_soa(0x5EED0001, 11)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        want_h, want_i = r.hit_rays(rays)
        bounce = np.concatenate([want_h[:, 1:4], want_h[:, 4:7] + [0.0, 0.25, 0.0]], 1)
        want_p = r.light_pdf(bounce)
    assert (want_i[:, 0] >= 0).sum() >= 10 and (want_i[:, 0] < 0).sum() >= 10
    assert np.array_equal(ids, want_i)
    assert np.array_equal(hits, want_h)
    assert np.array_equal(np.isnan(pdf), np.isnan(want_p)) and np.array_equal(pdf[~np.isnan(pdf)], want_p[~np.isnan(want_p)])
