"""The direct-lighting query on the CPU (no GPU needed): the entry points are
declared, bound and exported with the ABI unchanged, refuse a NULL context
before any HIP call, exist on the Python and C++ surfaces; the argument checks
and the launch plan (tests/native/direct_plan_check.cpp: the size and alignment
table, the refusals, the n * S limit, the LDS of every plan); the kernel table
is exactly the direct_light_kernel instantiations of the built gfx950 code
objects; and the conditions of the case file (tests/direct_cases.py) that are
asserted before any GPU answer is compared."""
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

import direct_cases as D
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_UNITS = ("direct_plan", "query_plan", "render_plan", "stage_scene", "bvh", "rtw_host")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
ENTRIES = ("rtw_direct_light", "rtw_direct_light_device")
# the substrings other host tests select kernel families by
TAKEN = ("render_kernel", "hit_rays_kernel", "light_pdf_rays_kernel", "occlusion_kernel", "light_sample_kernel",
         "camera_rays_kernel", "shade_rays_kernel", "primary_features_kernel", "denoise_", "path_begin",
         "path_advance", "path_fold", "PathBegin", "PathAdvance", "PathFold")


@functools.lru_cache(maxsize=None)
def direct_plan_check_exe():
    """tests/native/direct_plan_check.cpp, compiled once per test run."""
    out = tempfile.mkdtemp(prefix="direct_plan_check_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "direct_plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "direct_plan_check.cpp"),
                    *[os.path.join(CSRC, "host", u + ".cpp") for u in HOST_UNITS], "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


@needs_hipcc
def test_sizes_refusals_and_every_plan():
    r = subprocess.run([direct_plan_check_exe()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("\n0 wrong")


def _symbol(prec, world, robust):
    return f"_ZN3rtw3dev19direct_light_kernelI{'f' if prec == 'f32' else 'd'}Li{world}ELb{robust}EEEvNS_7DParamsIT_EE"


@needs_hipcc
def test_kernel_table_is_the_library_direct_light_kernels():
    """direct_kernels.h direct_kernel_exists -- what the launcher's table holds --
    names exactly the kernels of the built library, and none of them counts as
    another family's kernel by name."""
    from ray_tracing_weekend_amd import isa
    out = subprocess.run([direct_plan_check_exe(), "kernels"], capture_output=True, text=True, timeout=60,
                         check=True).stdout
    table = {_symbol(p, int(w), int(r)) for p, w, r in re.findall(r"^direct (f32|f64) (-?\d+) (\d)$", out, flags=re.M)}
    built = {k for co in isa.gfx950_code_objects() for k in isa.kernel_bytes(co) if "direct_light_kernel" in k}
    assert len(table) == 18
    assert table == built, (sorted(table - built), sorted(built - table))
    assert not any(t in k for k in built for t in TAKEN)
    # one code object per precision holds them, and nothing else
    homes = [set(isa.kernel_bytes(co)) for co in isa.gfx950_code_objects()]
    assert sorted(len(h) for h in homes if h & built) == [6, 12] and all(h <= built for h in homes if h & built)


def test_entry_points_are_declared_bound_and_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtw.h")).read()
    bound = {p[0] for p in _capi.PROTOTYPES}
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in bound, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert re.search(r"#define RTW_ABI_VERSION 10\b", header) and _capi.ABI_VERSION == 10
    assert C.sizeof(_capi.rtw_query_stats) == 56      # the stats keep their layout
    # the header states the law, the estimator and the stats value
    for text in ("first_stream + k", "hittable_list.rs:414-419", "material.rs:372-375", "camera.rs:480-521",
                 "term_c = (Le_c * spdf) / pdf", "exactly (0, 0, 0)", "light list's lobe alone",
                 "is_light_pdf = 8", "8 direct lighting"):
        assert text in header, text
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert re.search(r"\bfn " + name + r"\(", integration), name


def test_refusals_without_a_device():
    """A NULL context is RTW_E_INVALID from both entry points, before any HIP
    call (there is no GPU here)."""
    lib = rtw._lib
    inv = _capi.RTW_E_INVALID
    pts, direct = np.zeros((2, 6)), np.zeros((2, 3))
    samples, ids = np.zeros((4, 12)), np.zeros((4, 4), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.rtw_direct_light(None, vp(pts), 2, 7, 0, 0, 2, 0.0, 0, vp(direct), vp(samples), vp(ids)) == inv
    assert lib.rtw_direct_light(None, None, 0, 7, 0, 0, 1, 0.0, 0, None, None, None) == inv
    assert lib.rtw_direct_light_device(None, vp(pts), pts.nbytes, 2, 7, 0, 0, 2, 0.0, 0, vp(direct), direct.nbytes,
                                       vp(samples), samples.nbytes, vp(ids), ids.nbytes, None) == inv
    assert lib.rtw_direct_light_device(None, None, 0, 0, 7, 0, 0, 1, 0.0, 0, None, 0, None, 0, None, 0, None) == inv


def test_python_and_cpp_mirrors_have_the_surface():
    for name in ("direct_light", "render_direct"):
        assert callable(getattr(rtw.Renderer, name))
    assert callable(rtw.HittableList.direct_light)
    hpp = open(os.path.join(CSRC, "host", "rtw_host.hpp")).read()
    cpp = open(os.path.join(CSRC, "host", "ray_queries.cpp")).read()
    assert re.search(r"\bdirect_light\(const HittableList& world, const HittableList& lights", hpp)
    assert re.search(r"\brtw_direct_light\(ctx,", cpp)


@pytest.mark.parametrize("name", list(D.CASES))
def test_case_file_conditions(name):
    """What tests/direct_cases.py asserts about a case before a GPU answer is
    compared (enough non-zero terms, none non-finite), and what the restated
    law implies for its records."""
    soa, pts, S, exp = D.case(name)
    n = len(pts)
    assert pts.shape == (n, 6) and exp.samples.shape == (n * S, 12) and exp.ids.shape == (n * S, 4)
    assert {"cornell_box": 163, "simple_light": 44, "simple": 206, "lights64_emissive": 128, "checker": 44}[name] == n
    if D.CASES[name] is not None:
        assert exp.nonzero_terms >= D.CASES[name]
    assert np.isfinite(exp.term).all() and np.isfinite(exp.direct).all()
    added = exp.ids[:, 3] != 0
    assert not exp.term[~added].any() and (exp.ids[added, 1] >= 0).all()
    assert (exp.samples[added, 3] > 0).all() and (exp.samples[added, 5] > 0).all()
    assert np.array_equal(D.fold(np.zeros((n, 3)), exp.term, added, S), exp.direct)
    if name == "cornell_box":        # a mixed list: the quad light is met at t ~ 1, and a sphere is drawn too
        assert list(soa.light_kinds) == [1, 0] and set(exp.ids[:, 0]) == {0, 1}
        quad = (exp.ids[:, 0] == 0) & (exp.samples[:, 6] > 0)
        assert quad.sum() >= 100 and np.allclose(exp.samples[quad, 4], 1.0, rtol=0, atol=1e-9)


def test_closed_form_on_the_cpu():
    """One sphere light above a point: the mean of the restated terms is Le r^2 /
    D^2 within six standard errors of a derived sigma bound; with an opaque
    sphere in between the sum is exactly 0."""
    _, exp = D.closed_form(False)
    assert abs(D.CLOSED_EXPECT - 0.1875) < 1e-15 and 2.7e-4 < D.CLOSED_BOUND < 2.9e-4
    lo, hi = D.CLOSED_TERM_RANGE
    assert (exp.ids[:, 3] == 1).all()
    assert (exp.term >= lo * (1 - 1e-12)).all() and (exp.term <= hi * (1 + 1e-12)).all()
    assert (np.abs(exp.direct[0] / D.CLOSED_S - D.CLOSED_EXPECT) <= D.CLOSED_BOUND).all()
    _, exp = D.closed_form(True)
    assert (exp.direct == 0.0).all() and (exp.ids[:, 1] == 1).all() and not exp.term.any()
