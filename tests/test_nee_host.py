"""The any-hit and light-sample queries on the CPU (no GPU needed): the entry
points are declared, bound and exported with the ABI unchanged, refuse a NULL
context before any HIP call, exist on the Python and C++ surfaces; the plan
they launch from (tests/native/nee_plan_check.cpp) names kernels that exist,
and the kernel table is exactly the occlusion_kernel / light_sample_kernel
instantiations of the built gfx950 code objects."""
import atexit
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_UNITS = ("query_plan", "render_plan", "stage_scene", "bvh", "rtw_host")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
NEE_ENTRIES = ("rtw_occluded_rays", "rtw_occluded_rays_device", "rtw_light_sample", "rtw_light_sample_device")


@functools.lru_cache(maxsize=None)
def nee_plan_check_exe():
    """tests/native/nee_plan_check.cpp, compiled once per test run."""
    out = tempfile.mkdtemp(prefix="nee_plan_check_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "nee_plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "nee_plan_check.cpp"),
                    *[os.path.join(CSRC, "host", u + ".cpp") for u in HOST_UNITS], "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


@needs_hipcc
def test_every_query_plan_names_kernels_that_exist():
    r = subprocess.run([nee_plan_check_exe()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("\n0 wrong")


def _symbol(kind, prec, a, robust):
    name = {"occlusion": "16occlusion_kernel", "sample": "19light_sample_kernel"}[kind]
    return f"_ZN3rtw3dev{name}I{'f' if prec == 'f32' else 'd'}Li{a}ELb{robust}EEEvNS_7NParamsIT_EE"


@needs_hipcc
def test_kernel_table_is_the_library_occlusion_and_light_sample_kernels():
    """nee_kernels.h occlusion_kernel_exists / light_sample_kernel_exists -- what
    the launcher's tables hold -- name exactly the kernels of the built library;
    their names stay out of the closest-hit and light-pdf kernels' count."""
    from ray_tracing_weekend_amd import isa
    out = subprocess.run([nee_plan_check_exe(), "kernels"], capture_output=True, text=True, timeout=60,
                         check=True).stdout
    assert not re.findall(r"^(hit|light) (f32|f64) (-?\d+) (\d)$", out, flags=re.M)
    table = {_symbol(k, p, int(a), int(r))
             for k, p, a, r in re.findall(r"^(occlusion|sample) (f32|f64) (-?\d+) (\d)$", out, flags=re.M)}
    built = {k for co in isa.gfx950_code_objects() for k in isa.kernel_bytes(co)
             if "occlusion_kernel" in k or "light_sample_kernel" in k}
    assert len(table) == 30
    assert table == built, (sorted(table - built), sorted(built - table))
    assert not any("hit_rays_kernel" in k or "light_pdf_rays_kernel" in k or "render_kernel" in k for k in built)


def test_entry_points_are_declared_bound_and_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtw.h")).read()
    bound = {p[0] for p in _capi.PROTOTYPES}
    for name in NEE_ENTRIES:
        assert hasattr(lib, name), name
        assert name in bound, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert re.search(r"#define RTW_ABI_VERSION 10\b", header) and _capi.ABI_VERSION == 10
    assert C.sizeof(_capi.rtw_query_stats) == 56      # the stats keep their layout
    # the header states the semantics and the stream convention
    for text in ("t_min <= t && t <= t_max", "first_stream + k", "hittable_list.rs:414-419", "sphere.rs:72-80"):
        assert text in header, text


def test_refusals_without_a_device():
    """A NULL context is RTW_E_INVALID from every entry point, before any HIP
    call (there is no GPU here)."""
    lib = rtw._lib
    inv = _capi.RTW_E_INVALID
    rays, t_max, occ = np.zeros((2, 6)), np.ones(2), np.zeros(2, np.uint8)
    dirs, pdf, light = np.zeros((2, 3)), np.zeros(2), np.zeros(2, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.rtw_occluded_rays(None, vp(rays), 2, 0.0, vp(t_max), vp(occ)) == inv
    assert lib.rtw_occluded_rays(None, None, 0, 0.0, None, None) == inv
    assert lib.rtw_occluded_rays_device(None, vp(rays), 2, 0.0, vp(t_max), 16, vp(occ), 2, None) == inv
    assert lib.rtw_light_sample(None, vp(dirs), 2, 7, 0, 0, vp(dirs), vp(pdf), vp(light)) == inv
    assert lib.rtw_light_sample_device(None, vp(dirs), 2, 7, 0, 0, vp(dirs), 48, vp(pdf), 16, vp(light), 8, None) == inv


def test_python_and_cpp_mirrors_have_the_surface():
    for name in ("occluded", "light_sample"):
        assert callable(getattr(rtw.Renderer, name))
    assert callable(rtw.HittableList.occluded) and callable(rtw.HittableList.random)
    hpp = open(os.path.join(CSRC, "host", "rtw_host.hpp")).read()
    cpp = open(os.path.join(CSRC, "host", "ray_queries.cpp")).read()
    for name, entry in (("occluded", "rtw_occluded_rays"), ("light_sample", "rtw_light_sample")):
        assert re.search(r"\b" + name + r"\(const HittableList& world", hpp), name
        assert re.search(r"\b" + entry + r"\(ctx,", cpp), entry
