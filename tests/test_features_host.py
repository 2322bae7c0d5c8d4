"""The feature pass (rtw_render_features) on the CPU (no GPU needed): the entry
points are declared, bound and exported; the refusals the C-ABI makes before it
touches a device; the launcher's kernel table against the library's symbols;
the pass's plan against the render's (tests/native/features_plan_check.cpp);
feature_means on a hand-made array; and the oracle expectations the GPU tests
compare with (tests/feature_cases.py) are not vacuous and are safe to compare
bit for bit."""
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

import feature_cases as F
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_UNITS = ("query_plan", "render_plan", "stage_scene", "bvh", "rtw_host")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
ENTRIES = ("rtw_render_features", "rtw_render_features_device")


@functools.lru_cache(maxsize=None)
def features_plan_check_exe():
    """tests/native/features_plan_check.cpp, compiled once per test run."""
    out = tempfile.mkdtemp(prefix="features_plan_check_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "features_plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "features_plan_check.cpp"),
                    *[os.path.join(CSRC, "host", u + ".cpp") for u in HOST_UNITS], "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


def test_feature_entry_points_are_declared_bound_and_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtw.h")).read()
    bound = {p[0] for p in _capi.PROTOTYPES}
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in bound, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert re.search(r"#define RTW_ABI_VERSION 10\b", header)
    assert callable(rtw.Renderer.render_features) and callable(rtw.Camera.render_features)
    assert callable(rtw.feature_means)


def test_feature_refusals_without_a_device():
    """A NULL context is RTW_E_INVALID from both entry points whatever else is
    wrong with the call, before any HIP call (the test needs no GPU)."""
    lib = rtw._lib
    inv = _capi.RTW_E_INVALID
    cam, _ = F.cameras("simple", 8, 8)
    wide = _capi.rtw_camera.from_buffer_copy(cam.raw)
    wide.image_width = 1 << 16
    feat, ids, counts = np.zeros((8, 8, 8)), np.zeros((8, 8, 2), np.int32), np.ones((8, 8), np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    calls = [
        (C.byref(cam.raw), 0, 4, vp(counts), vp(feat), vp(ids)),           # nothing else wrong
        (None, 0, 4, None, vp(feat), None),                                # NULL camera
        (C.byref(cam.raw), 0, 4, None, None, None),                        # NULL features
        (C.byref(cam.raw), 0xFFFFFFFF, 1, None, vp(feat), None),           # first + n overflows
        (C.byref(wide), 0, 4, None, vp(feat), None),                       # W >= 2^16
        (C.byref(cam.raw), 0, 0, None, vp(feat), None),                    # n = 0
    ]
    for cam_p, first, n, cp, fp, ip in calls:
        assert lib.rtw_render_features(None, cam_p, C.c_uint64(1), first, n, cp, fp, ip) == inv
        assert lib.rtw_render_features_device(None, cam_p, C.c_uint64(1), first, n, cp, counts.nbytes, fp,
                                              feat.nbytes, ip, ids.nbytes, None) == inv
    # a buffer that is too small
    assert lib.rtw_render_features_device(None, C.byref(cam.raw), C.c_uint64(1), 0, 4, None, 0, vp(feat),
                                          feat.nbytes - 8, None, 0, None) == inv


def _symbol(prec, world, robust):
    return f"_ZN3rtw3dev23primary_features_kernelI{'f' if prec == 'f32' else 'd'}Li{world}ELb{robust}EEEvNS_7FParamsIT_EE"


@needs_hipcc
def test_feature_kernel_table_is_the_library_feature_kernels():
    """What the launcher's table holds (hit_kernel_exists, features_launch.hpp)
    names exactly the primary_features_kernel symbols of the built library, and
    none of them counts as a render or query kernel by name."""
    from ray_tracing_weekend_amd import isa
    out = subprocess.run([features_plan_check_exe(), "kernels"], capture_output=True, text=True, timeout=60,
                         check=True).stdout
    table = {_symbol(p, int(w), int(r)) for p, w, r in re.findall(r"^features (f32|f64) (-?\d+) (\d)$", out, flags=re.M)}
    built = {k for co in isa.gfx950_code_objects() for k in isa.kernel_bytes(co) if "primary_features_kernel" in k}
    assert len(table) == 18
    assert table == built, (sorted(table - built), sorted(built - table))
    for k in built:
        assert not any(s in k for s in ("render_kernel", "hit_rays_kernel", "light_pdf_rays_kernel")), k


@needs_hipcc
def test_feature_plan_is_the_render_plan_of_the_camera():
    r = subprocess.run([features_plan_check_exe()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("\n0 wrong")


def test_feature_means_on_a_hand_made_array():
    f = np.zeros((2, 2, 8))
    # 4 samples, 2 hits: albedo sum (2, 1, 0), normals (0, 0, 1) + (0, 1, 0), distances 3 + 5
    f[0, 0] = (2.0, 1.0, 0.0, 0.0, 1.0, 1.0, 8.0, 2.0)
    # 4 samples, all misses on a (0.5, 0.5, 1) background
    f[0, 1] = (2.0, 2.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    # 4 hits whose normals cancel: (1, 0, 0) twice, (-1, 0, 0) twice
    f[1, 0] = (4.0, 4.0, 4.0, 0.0, 0.0, 0.0, 4.0, 4.0)
    # f[1, 1]: a pixel that took no sample
    albedo, normal, distance, coverage = rtw.feature_means(f, 4)
    assert np.array_equal(albedo[0, 0], (0.5, 0.25, 0.0)) and np.array_equal(albedo[0, 1], (0.5, 0.5, 1.0))
    assert np.allclose(normal[0, 0], (0.0, 2 ** -0.5, 2 ** -0.5), rtol=0, atol=1e-15)
    assert not normal[0, 1].any() and not normal[1, 0].any() and not normal[1, 1].any()
    assert distance[0, 0] == 4.0 and distance[1, 0] == 1.0 and np.isinf(distance[0, 1]) and np.isinf(distance[1, 1])
    assert np.array_equal(coverage, [[0.5, 0.0], [1.0, 0.0]])
    # per-pixel counts: the pixel without samples divides by nothing
    counts = np.array([[4, 2], [4, 0]], np.uint32)
    albedo, normal, distance, coverage = rtw.feature_means(f, counts)
    assert np.array_equal(albedo[0, 1], (1.0, 1.0, 2.0)) and not albedo[1, 1].any() and coverage[1, 1] == 0.0
    assert np.isfinite(albedo).all() and np.isfinite(normal).all() and np.isfinite(coverage).all()
    assert albedo.shape == (2, 2, 3) and normal.shape == (2, 2, 3) and distance.shape == (2, 2) == coverage.shape
    with pytest.raises(rtw.RenderError):
        rtw.feature_means(np.zeros((2, 2, 3)), 4)


# ---- the reference inputs of tests/test_gpu_features.py, on the oracle alone
def test_expectations_agree_with_world_hit_and_fold_in_order():
    e = F.samples("simple")
    assert e.world_hit_agrees                       # world_hit answers every primary ray as trace_path met it
    one = e.fold(0, 1)
    assert F.same(e.fold(1, 3, onto=one), e.fold(0, 4))
    hit = e.mtype >= 0
    assert F.same(e.fold(0, 4)[..., 7], hit.sum(-1))
    # unit normals (the ground sphere of radius 1000 loses digits in its discriminant:
    # |p - c| / r is 1 to about r^2 * EPSILON * 10), distances ahead of the camera
    n = e.f[..., 3:6][hit]
    assert np.allclose((n * n).sum(-1), 1.0, rtol=0, atol=1e-8) and (e.f[..., 6][hit] > 0).all()


def test_simple_meets_hits_misses_and_three_material_kinds():
    e = F.samples("simple")
    hit = e.mtype >= 0
    assert hit.sum() >= 100 and (~hit).sum() >= 100, (int(hit.sum()), int((~hit).sum()))
    assert len(set(e.mtype[hit].tolist())) >= 3, set(e.mtype[hit].tolist())


def test_cornell_box_meets_the_light_a_cuboid_and_a_quad():
    e = F.samples("cornell_box")
    assert e.world_hit_agrees
    assert (e.mtype == rtw.RTW_DIFFUSE_LIGHT).sum() >= 1
    assert (e.kind == _capi.RTW_PRIM_CUBOID).sum() >= 1 and (e.kind == _capi.RTW_PRIM_QUAD).sum() >= 1
    # the light's albedo is its emitted colour: beyond 1
    assert (e.f[..., :3][e.mtype == rtw.RTW_DIFFUSE_LIGHT] > 1.0).all()


def test_checkered_spheres_samples_stay_clear_of_the_checker_edges():
    """The device's atan2 / acos differ from libm by a few ulp (tests/test_gpu_query.py
    b), so a sample whose u or v * inv_scale sat on an integer could flip colour
    legally; none is within 2^-30 of one, and none is excluded."""
    e = F.samples("checkered_spheres")
    read = np.isfinite(e.checker_margin)
    assert read.sum() >= 100 and read.sum() == (e.mtype >= 0).sum()
    assert e.checker_margin.min() >= 2.0 ** -30, e.checker_margin.min()
    cols = {tuple(c) for c in e.f[..., :3][read].tolist()}
    assert len(cols) >= 2                           # both colours of the checker are met


def test_some_camera_has_defocus_and_some_has_none():
    assert F.samples("simple_defocus").cam.defocus_angle > 0.0
    assert F.samples("simple").cam.defocus_angle == 0.0
    a, b = F.samples("simple_defocus").f, F.samples("simple").f
    assert not F.same(a, b)
