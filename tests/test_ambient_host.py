"""The ambient-occlusion query on the CPU (no GPU needed): the entry points are
declared, bound and exported with the ABI unchanged, refuse a NULL context
before any HIP call, exist on the Python and C++ surfaces; the argument checks
and the launch plan (tests/native/ambient_plan_check.cpp: the size and alignment
table, the refusals in their order, the limits, the LDS of every plan); the
kernel table is exactly the ambient_kernel instantiations of the built gfx950
code objects; and the conditions of the case file (tests/ambient_cases.py) that
are asserted before any GPU answer is compared."""
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

import ambient_cases as A
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_UNITS = ("ambient_plan", "query_plan", "render_plan", "stage_scene", "bvh", "rtw_host")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
ENTRIES = ("rtw_ambient_occlusion", "rtw_ambient_occlusion_device")
# the substrings other host tests select kernel families by
TAKEN = ("render_kernel", "hit_rays_kernel", "light_pdf_rays_kernel", "occlusion_kernel", "light_sample_kernel",
         "direct_light_kernel", "camera_rays_kernel", "shade_rays_kernel", "primary_features_kernel", "denoise_",
         "path_begin", "path_advance", "path_fold", "PathBegin", "PathAdvance", "PathFold")


@functools.lru_cache(maxsize=None)
def ambient_plan_check_exe():
    """tests/native/ambient_plan_check.cpp, compiled once per test run."""
    out = tempfile.mkdtemp(prefix="ambient_plan_check_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "ambient_plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "ambient_plan_check.cpp"),
                    *[os.path.join(CSRC, "host", u + ".cpp") for u in HOST_UNITS], "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


@needs_hipcc
def test_sizes_refusals_limits_and_every_plan():
    r = subprocess.run([ambient_plan_check_exe()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("\n0 wrong")


def _symbol(prec, world, robust):
    return f"_ZN3rtw3dev14ambient_kernelI{'f' if prec == 'f32' else 'd'}Li{world}ELb{robust}EEEvNS_7AParamsIT_EE"


@needs_hipcc
def test_kernel_table_is_the_library_ambient_kernels():
    """ambient_kernels.h ambient_kernel_exists -- what the launcher's table holds --
    names exactly the kernels of the built library (the worlds and test forms of
    the any-hit query), and none of them counts as another family's kernel by name."""
    from ray_tracing_weekend_amd import isa
    out = subprocess.run([ambient_plan_check_exe(), "kernels"], capture_output=True, text=True, timeout=60,
                         check=True).stdout
    table = {_symbol(p, int(w), int(r)) for p, w, r in re.findall(r"^ambient (f32|f64) (-?\d+) (\d)$", out, flags=re.M)}
    built = {k for co in isa.gfx950_code_objects() for k in isa.kernel_bytes(co) if "ambient_kernel" in k}
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
    # the header states the law, operation by operation, and the stats value
    flat = re.sub(r"\s*\n\s*\*\s*", " ", header)      # (the comment's line breaks are no part of a phrase)
    for text in ("first_stream + k", "pdf.rs:38-52", "onb.rs:8-35", "utils.rs:146-161",
                 "CosinePdf::new(normal).generate(rng)", "sqrt(1 - r2)", "normalize(cross(w, a))",
                 "d is not renormalised", "t_min..=t_max", "open[k] += !occ", "exactly (0, 0, 0)",
                 "NaN or < t_min", "An empty light list is fine", "is_light_pdf = 9", "9 ambient occlusion"):
        assert text in flat, text
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert re.search(r"\bfn " + name + r"\(", integration), name


def test_refusals_without_a_device():
    """A NULL context is RTW_E_INVALID from both entry points, before any HIP
    call (there is no GPU here)."""
    lib = rtw._lib
    inv = _capi.RTW_E_INVALID
    inf = float("inf")
    pts, open_ = np.zeros((2, 6)), np.zeros(2, np.uint32)
    dirs, occ = np.zeros((4, 3)), np.zeros(4, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.rtw_ambient_occlusion(None, vp(pts), 2, 7, 0, 0, 2, 0.0, inf, 0, vp(open_), vp(dirs), vp(occ)) == inv
    assert lib.rtw_ambient_occlusion(None, None, 0, 7, 0, 0, 1, 0.0, inf, 0, None, None, None) == inv
    assert lib.rtw_ambient_occlusion_device(None, vp(pts), pts.nbytes, 2, 7, 0, 0, 2, 0.0, inf, 0, vp(open_),
                                            open_.nbytes, vp(dirs), dirs.nbytes, vp(occ), occ.nbytes, None) == inv
    assert lib.rtw_ambient_occlusion_device(None, None, 0, 0, 7, 0, 0, 1, 0.0, inf, 0, None, 0, None, 0, None, 0,
                                            None) == inv


def test_python_and_cpp_mirrors_have_the_surface():
    for name in ("ambient_occlusion", "render_ao"):
        assert callable(getattr(rtw.Renderer, name))
    assert callable(rtw.HittableList.ambient_occlusion)
    hpp = open(os.path.join(CSRC, "host", "rtw_host.hpp")).read()
    cpp = open(os.path.join(CSRC, "host", "ray_queries.cpp")).read()
    assert re.search(r"\bambient_occlusion\(const HittableList& world, const HittableList& lights", hpp)
    assert re.search(r"\brtw_ambient_occlusion\(ctx,", cpp)


# name: (points, open pairs, occluded pairs) of the restatement at the cases' t_min = 1e-3, and of
# the two cases kept at the reference's own t_min = f64::EPSILON too
COUNTS = {"simple": (206, 145, 267), "cornell_box": (163, 319, 333), "simple_light": (44, 95, 81),
          "lights64": (128, 440, 72)}
EPS_COUNTS = {"simple": (206, 79, 333), "simple_light": (44, 55, 121)}


@pytest.mark.parametrize("name", list(A.CASES))
def test_case_file_conditions(name):
    """What tests/ambient_cases.py asserts about a case before a GPU answer is
    compared (at least 10 % open and 10 % occluded pairs on the restatement alone,
    no sphere's gate changing an answer), and what the restated law implies for
    its records."""
    soa, pts, S, t_max, exp = A.case(name)
    n = len(pts)
    assert pts.shape == (n, 6) and exp.directions.shape == (n * S, 3) and exp.occluded.shape == (n * S,)
    assert (n, exp.n_open, exp.n_occluded) == COUNTS[name] and exp.t_min == A.T_MIN == 1e-3
    if name in A.EPS_CASES:      # the same points at the reference's t_min: its own surface blocks more
        e = A.eps_case(name)[4]
        assert (n, e.n_open, e.n_occluded) == EPS_COUNTS[name] and e.t_min == A.EPS
        assert np.array_equal(e.directions, exp.directions) and (e.occluded >= exp.occluded).all()
    assert n <= 250 and S <= 4 and exp.pairs == n * S and exp.gate_changes == 0
    assert 10 * exp.n_open >= exp.pairs and 10 * exp.n_occluded >= exp.pairs
    assert (t_max == A.INF) == (name == "simple")          # the sky, and three finite reaches
    assert exp.open.dtype == np.uint32 and int(exp.open.sum()) == exp.n_open and (exp.open <= S).all()
    # every direction lies in the normal's hemisphere and is a unit vector within rounding
    nrm = np.repeat(pts[:, 3:6], S, 0)
    assert ((exp.directions * nrm).sum(-1) >= -1e-12).all()
    assert np.allclose(np.linalg.norm(exp.directions, axis=-1), 1.0, rtol=0, atol=1e-12)


def test_zero_normals_windows_and_empty_ranges_on_the_cpu():
    """The restated law's special rows: a zero normal is skipped (its count kept
    when continued), sample windows compose, an empty or NaN range leaves every
    pair open."""
    soa, pts, S, t_max, exp = A.case("simple_light")
    T = A.T_MIN
    p = pts[:9].copy()
    p[4, 3:6] = 0.0
    start = np.arange(9, dtype=np.uint32) + 5
    e = A.Expected(soa, p, A.SEED, S, t_max, T, open=start)
    assert e.open[4] == 5 + 4 and not e.directions[4 * S:5 * S].any() and not e.live[4 * S:5 * S].any()
    keep = np.r_[0:4 * S, 5 * S:9 * S]
    assert np.array_equal(e.directions[keep], exp.directions[keep]) and np.array_equal(e.occluded[keep], exp.occluded[keep])
    a = A.Expected(soa, pts[:9], A.SEED, 2, t_max, T)
    b = A.Expected(soa, pts[:9], A.SEED, 2, t_max, T, first_sample=2, open=a.open)
    assert np.array_equal(b.open, exp.open[:9])
    for empty in (float("nan"), T / 2):
        assert (A.Expected(soa, pts[:9], A.SEED, S, empty, T).open == S).all()


def test_closed_form_on_the_cpu():
    """One sphere of r = 1 at distance D = 4 along the normal blocks r^2 / D^2 =
    1/16 of the cosine-weighted hemisphere: the restated open share is 15/16
    within six standard errors; with t_max = 2.5 < D - r every sample is open."""
    assert A.CLOSED_BLOCKED == 1 / 16 and abs(A.CLOSED_BOUND - 0.0227) < 5e-5 and A.CLOSED_S == 4096
    _, t_max, exp = A.closed_form(False)
    assert t_max == A.INF
    assert abs(int(exp.open[0]) / A.CLOSED_S - 15 / 16) <= A.CLOSED_BOUND
    _, t_max, exp = A.closed_form(True)
    assert t_max == 2.5 < A.CLOSED_D - A.CLOSED_R
    assert int(exp.open[0]) == A.CLOSED_S and not exp.occluded.any()
