"""The batched ray queries on the CPU (no GPU needed): the query plan
(tests/native/query_plan_check.cpp: the query's world is the render plan's for
the same tuning, its LDS fits, a tree too big for LDS falls back to the
while-while world, the light path flips at 63 / 64 lights and with light_grid
0, no plan names a kernel the library lacks), the kernel table against the
library's symbols, and the refusals the C-ABI makes before it touches a
device."""
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
QUERY_ENTRIES = ("rtw_hit_rays", "rtw_hit_rays_device", "rtw_light_pdf_rays", "rtw_light_pdf_rays_device",
                 "rtw_get_query_stats")


@functools.lru_cache(maxsize=None)
def query_plan_check_exe():
    """tests/native/query_plan_check.cpp, compiled once per test run."""
    out = tempfile.mkdtemp(prefix="query_plan_check_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "query_plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "query_plan_check.cpp"),
                    *[os.path.join(CSRC, "host", u + ".cpp") for u in HOST_UNITS], "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


@needs_hipcc
def test_query_plan_known_answers_and_sweep():
    r = subprocess.run([query_plan_check_exe()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("\n0 wrong")


@functools.lru_cache(maxsize=None)
def query_grid_check_exe(sanitize=False):
    """tests/native/query_grid_check.cpp over the header's grid function, compiled once per test run."""
    out = tempfile.mkdtemp(prefix="query_grid_check_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "query_grid_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", *flags, "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "query_grid_check.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    return exe


@needs_hipcc
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_query_grid_is_the_smallest_of_blocks_resident_and_cap(sanitize):
    """Tuning "query_grid": cap 0 (off) at blocks above, equal to and below the
    resident count, cap 1, cap > blocks, a huge cap, never 0 for blocks > 0; the
    same stand-alone host program also under the address and undefined-behaviour
    sanitizers."""
    r = subprocess.run([query_grid_check_exe(sanitize)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("\n0 wrong")
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_query_grid_key_is_in_the_header_key_list():
    """The key is documented next to "persist" in rtw.h's key list, and a NULL
    context refuses it before any HIP call.  (A context needs a device:
    tests/test_gpu_query_grid.py sets the key, sees -1 refused and the value
    clamped and sets it on a virtual-rank context.)"""
    header = open(os.path.join(ROOT, "include", "rtw.h")).read()
    keys = header[header.index("scheduling knobs"):header.index("int rtw_set_tuning")]
    assert '"query_grid"' in keys and '"persist"' in keys
    assert rtw._lib.rtw_set_tuning(None, b"query_grid", 1) == _capi.RTW_E_INVALID


def _symbol(kind, prec, a, robust):
    name = {"hit": "15hit_rays_kernel", "light": "21light_pdf_rays_kernel"}[kind]
    return f"_ZN3rtw3dev{name}I{'f' if prec == 'f32' else 'd'}Li{a}ELb{robust}EEEvNS_7QParamsIT_EE"


@needs_hipcc
def test_query_kernel_table_is_the_library_query_kernels():
    """query_kernels.h hit_kernel_exists / light_kernel_exists -- what the
    query plan may pick and the launcher's tables hold -- name exactly the
    query kernels of the built library, and none of them is a render kernel
    by name (tests/test_capi_host.py counts those)."""
    from ray_tracing_weekend_amd import isa
    out = subprocess.run([query_plan_check_exe(), "kernels"], capture_output=True, text=True, timeout=60,
                         check=True).stdout
    table = {_symbol(k, p, int(a), int(r))
             for k, p, a, r in re.findall(r"^(hit|light) (f32|f64) (-?\d+) (\d)$", out, flags=re.M)}
    built = {k for co in isa.gfx950_code_objects() for k in isa.kernel_bytes(co)
             if "hit_rays_kernel" in k or "light_pdf_rays_kernel" in k}
    assert len(table) == 30
    assert table == built, (sorted(table - built), sorted(built - table))
    assert not any("render_kernel" in k for k in built)


def test_query_entry_points_are_declared_bound_and_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtw.h")).read()
    bound = {p[0] for p in _capi.PROTOTYPES}
    for name in QUERY_ENTRIES:
        assert hasattr(lib, name), name
        assert name in bound, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert re.search(r"#define RTW_ABI_VERSION 10\b", header)


def test_query_refusals_without_a_device():
    """A NULL context is RTW_E_INVALID from every query entry point, before
    any HIP call (there is no GPU here)."""
    lib = rtw._lib
    inv = _capi.RTW_E_INVALID
    rays = np.zeros((2, 6))
    hits, ids, pdf = np.zeros((2, 9)), np.zeros((2, 4), np.int32), np.zeros(2)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.rtw_hit_rays(None, vp(rays), 2, 0.0, vp(hits), vp(ids)) == inv
    assert lib.rtw_hit_rays(None, None, 0, 0.0, None, None) == inv
    assert lib.rtw_hit_rays_device(None, vp(rays), 2, 0.0, vp(hits), hits.nbytes, vp(ids), ids.nbytes, None) == inv
    assert lib.rtw_light_pdf_rays(None, vp(rays), 2, vp(pdf)) == inv
    assert lib.rtw_light_pdf_rays_device(None, vp(rays), 2, vp(pdf), pdf.nbytes, None) == inv
    st = _capi.rtw_query_stats()
    assert lib.rtw_get_query_stats(None, C.byref(st)) == inv
    assert C.sizeof(_capi.rtw_query_stats) == 56


def test_python_mirror_has_the_query_surface():
    for name in ("hit_rays", "light_pdf", "get_query_stats"):
        assert callable(getattr(rtw.Renderer, name))
    assert callable(rtw.HittableList.hit) and callable(rtw.HittableList.pdf_value)
    assert (_capi.RTW_PRIM_PLANE, _capi.RTW_PRIM_QUAD, _capi.RTW_PRIM_CUBOID, _capi.RTW_PRIM_SPHERE) == (0, 1, 2, 3)
