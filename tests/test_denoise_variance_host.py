"""The variance-guided denoiser (rtw_denoise_variance) and the luminance moments
on the CPU (no GPU needed): the entry points are declared, bound and exported
and the ABI version stays 10; the new struct has one layout in rtw.h (through
gcc), the ctypes mirror and INTEGRATION.md's Rust blocks; the plan
(tests/native/denoise_variance_plan_check.cpp); the launcher's kernel table
against the library's symbols; and the restatement the GPU tests compare with
(tests/denoise_variance_cases.py) behaves as the contract says -- on made-up
frames, and on the committed oracle frame of scenes::simple it closes the
defect it was written for: the old filter makes a 256-spp image worse, this one
makes it better."""
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

import denoise_cases as D
import denoise_variance_cases as V
import ray_tracing_weekend_amd as rtw
import test_integration_layout as L
from ray_tracing_weekend_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
ENTRIES = ("rtw_render_window_moments", "rtw_render_window_moments_device", "rtw_adaptive_moments",
           "rtw_adaptive_moments_device", "rtw_denoise_variance_params_default", "rtw_denoise_variance",
           "rtw_denoise_variance_device")
STRUCT = "rtw_denoise_variance_params"
SVGF_SYMBOLS = {
    "svgf_prepare_kernel<float>": "_ZN3rtw3dev19svgf_prepare_kernelIfEEvNS_11SvgfPrepareE",
    "svgf_prepare_kernel<double>": "_ZN3rtw3dev19svgf_prepare_kernelIdEEvNS_11SvgfPrepareE",
    "svgf_atrous_kernel<false>": "_ZN3rtw3dev18svgf_atrous_kernelILb0EEEvNS_10SvgfAtrousE",
    "svgf_atrous_kernel<true>": "_ZN3rtw3dev18svgf_atrous_kernelILb1EEEvNS_10SvgfAtrousE",
}
MOMENTS_SYMBOLS = {
    "_ZN3rtw3dev19fold_moments_kernelIfEEvNS_11MomentsFoldE",
    "_ZN3rtw3dev19fold_moments_kernelIdEEvNS_11MomentsFoldE",
    "_ZN3rtw3dev21unpack_moments_kernelEPKdjjjPd",
}


@functools.lru_cache(maxsize=None)
def plan_check_exe():
    """tests/native/denoise_variance_plan_check.cpp with the plan unit alone, compiled once per test run."""
    out = tempfile.mkdtemp(prefix="denoise_variance_plan_check_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "denoise_variance_plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "denoise_variance_plan_check.cpp"),
                    os.path.join(CSRC, "host", "denoise_variance_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


# ---- declarations
def test_entry_points_are_declared_bound_and_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtw.h")).read()
    bound = {p[0] for p in _capi.PROTOTYPES}
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in bound, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert re.search(r"#define RTW_ABI_VERSION 10\b", header)
    assert _capi.ABI_VERSION == 10 and lib.rtw_abi_version() == 10
    for method in ("render_window_moments", "render_window_moments_device", "adaptive_moments",
                   "adaptive_moments_device", "denoise_variance"):
        assert callable(getattr(rtw.Renderer, method)), method
    assert rtw.DenoiseVarianceParams().as_dict() == V.SHIPPED
    assert rtw.DenoiseVarianceParams(iterations=3, sigma_var=0).as_dict() == dict(V.SHIPPED, iterations=3,
                                                                                  sigma_var=0.0)
    with pytest.raises(rtw.RenderError):
        rtw.DenoiseVarianceParams(sigma_colour=1.0)
    # the old parameters are as they were
    assert rtw.DenoiseParams().as_dict() == D.SHIPPED
    assert [f for f, _ in _capi.rtw_denoise_params._fields_] == list(D.SHIPPED)


def test_refusals_without_a_device():
    """A NULL context is RTW_E_INVALID from every new entry point, before any HIP call."""
    lib = rtw._lib
    s, f, m, o = np.zeros((4, 4, 3)), np.zeros((4, 4, 8)), np.zeros((4, 4, 2)), np.zeros((4, 4, 3))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    dp = lambda a: a.ctypes.data_as(_capi._f64p)   # noqa: E731
    cam = rtw.CameraBuilder().with_image_width(4).with_image_height(4).build()
    inv = _capi.RTW_E_INVALID
    assert lib.rtw_denoise_variance(None, vp(s), vp(f), vp(m), None, 4, 4, 4, None, vp(o)) == inv
    assert lib.rtw_denoise_variance_device(None, vp(s), _capi.RTW_F64, s.nbytes, vp(f), f.nbytes, vp(m), m.nbytes,
                                           None, 0, 4, 4, 4, None, vp(o), o.nbytes, None) == inv
    assert lib.rtw_render_window_moments(None, C.byref(cam.raw), 1, 0, 1, dp(s), dp(m), None) == inv
    assert lib.rtw_render_window_moments_device(None, C.byref(cam.raw), 1, 0, 1, vp(s), s.nbytes, vp(m), m.nbytes,
                                                None) == inv
    assert lib.rtw_adaptive_moments(None, dp(m)) == inv
    assert lib.rtw_adaptive_moments_device(None, vp(m), m.nbytes, None) == inv
    assert not s.any() and not m.any() and not o.any()
    p = _capi.rtw_denoise_variance_params()
    lib.rtw_denoise_variance_params_default(None)   # a NULL struct is left alone
    lib.rtw_denoise_variance_params_default(C.byref(p))
    assert {k: getattr(p, k) for k, _ in p._fields_} == V.SHIPPED


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """offsetof / sizeof of the new struct's fields, from gcc on rtw.h."""
    d = tmp_path_factory.mktemp("denoise_variance_layout")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "rtw.h"', "int main(void) {",
             f'printf("sizeof %zu\\n", sizeof({STRUCT}));']
    for field, _ in getattr(_capi, STRUCT)._fields_:
        lines.append(f'printf("{field} %zu %zu\\n", offsetof({STRUCT}, {field}), sizeof((({STRUCT} *)0)->{field}));')
    lines.append("return 0; }")
    src, exe = d / "probe.c", d / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        parts = line.split()
        out[parts[0]] = int(parts[1]) if parts[0] == "sizeof" else (int(parts[1]), int(parts[2]))
    return out


def test_struct_layouts_agree(c_layout):
    ct = getattr(_capi, STRUCT)
    fields, size = L._rust_layout(STRUCT)
    assert [f for f, _, _ in fields] == [f for f, _ in ct._fields_] == list(V.SHIPPED)
    for field, off, sz in fields:
        assert c_layout[field] == (off, sz), field
    for field, ftype in ct._fields_:
        assert c_layout[field] == (getattr(ct, field).offset, C.sizeof(ftype)), field
    assert c_layout["sizeof"] == size == C.sizeof(ct)


@needs_hipcc
def test_plan():
    r = subprocess.run([plan_check_exe()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("0 wrong")


@needs_hipcc
def test_kernel_tables_are_the_library_kernels():
    """The four svgf kernels of the launcher's table and the three moments
    kernels are in the library, and nothing else carries their names."""
    from ray_tracing_weekend_amd import isa
    out = subprocess.run([plan_check_exe(), "kernels"], capture_output=True, text=True, timeout=60,
                         check=True).stdout
    table = {SVGF_SYMBOLS[name] for name in re.findall(r"^svgf (.+)$", out, flags=re.M)}
    kernels = {k for co in isa.gfx950_code_objects() for k in isa.kernel_bytes(co)}
    assert len(table) == 4
    assert table == {k for k in kernels if "svgf_" in k}
    assert MOMENTS_SYMBOLS == {k for k in kernels if "moments_kernel" in k}


# ---- the restatement the GPU tests compare with
def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


def same(a, b):
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("size", [(37, 19), (5, 3), (1, 1)])
def test_with_every_count_one_it_is_the_old_filter_without_a_colour_stop(size):
    sums, features, counts = D.synthetic(*size)
    moments = V.synthetic_moments(*size)
    ones = np.where(counts > 0, 1, 0).astype(np.uint32)
    for params in (V.SHIPPED, dict(V.SHIPPED, iterations=7, demodulate=0), dict(V.SHIPPED, fill_nonfinite=0)):
        new = V.restate_variance(sums, features, moments, ones, details=True, **params)
        old_params = {k: v for k, v in params.items() if k != "sigma_var"}
        old = D.restate(sums, features, ones, sigma_colour=0.0, **old_params)
        assert not new[3].any()
        assert same(new[0], old[0]) and new[1:3] == old[1:3]


@pytest.mark.parametrize("params", [V.SHIPPED, dict(V.SHIPPED, demodulate=0), dict(V.SHIPPED, sigma_var=0.0),
                                    dict(V.SHIPPED, iterations=7, normal_power_log2=0)])
def test_a_constant_image_over_constant_guides_comes_back(params):
    sums, features = D.constant(23, 17, spp=8)
    moments = V.constant_moments(23, 17, spp=8)
    out, filled, left, has_var, ve = V.restate_variance(sums, features, moments, 8, details=True, **params)
    assert ulps(out, sums / 8).max() <= 4 and filled == 0 and left == 0
    # every pixel has a variance, and filtering equal variances makes them smaller
    assert has_var.all() and (ve > 0).all()
    first = V.restate_variance(sums, features, moments, 8, details=True, **dict(params, iterations=1))[4]
    assert (ve <= first).all() and (ve[4:-4, 4:-4] < first[4:-4, 4:-4]).all()


def test_nonfinite_moments_and_single_samples_have_no_variance():
    size = (37, 19)
    sums, features, _ = D.synthetic(*size)
    moments, counts = V.synthetic_moments(*size), V.counts_with_ones(*size)
    out, filled, left, has_var, ve = V.restate_variance(sums, features, moments, counts, details=True, **V.SHIPPED)
    bad = ~np.isfinite(moments).all(-1)
    assert bad.sum() >= 10 and (counts == 1).sum() >= 10
    assert not has_var[bad].any() and not has_var[counts <= 1].any()
    assert (ve[~has_var] == 0).all() and np.isfinite(ve).all() and (ve >= 0).all()
    assert has_var.sum() >= 300
    # with the fill on, a non-finite moment costs no pixel: what is left is what the old filter leaves
    _, _, left_old = D.restate(sums, features, counts, **D.SHIPPED)
    assert left == left_old and filled >= 1
    with np.errstate(all="ignore"):
        valid = np.isfinite(sums / counts[..., None].astype(np.float64)).all(-1) & (counts > 0) & \
            np.isfinite(features).all(-1)
    assert np.isfinite(out[bad & valid]).all() and (bad & valid).sum() >= 5


def test_the_synthetic_moments_are_not_vacuous():
    for size in ((37, 19), (70, 45)):
        sums, features, _ = D.synthetic(*size)
        moments, counts = V.synthetic_moments(*size), V.counts_with_ones(*size)
        assert np.isnan(moments).any() and (moments == np.inf).any() and (moments == -np.inf).any()
        nd = np.maximum(counts, 1).astype(np.float64)
        with np.errstate(all="ignore"):
            var = moments[..., 1] / nd - (moments[..., 0] / nd) ** 2
        assert (var == 0).sum() + (var < 0).sum() >= 10 and (var < 0).sum() >= 2 and (var > 0).sum() >= 300
        has_var, ve = V.restate_variance(sums, features, moments, counts, details=True, **V.SHIPPED)[3:]
        assert 0.5 < has_var.mean() < 0.98
        # the colour stop does something: sigma_var changes the picture
        a = V.restate_variance(sums, features, moments, counts, **V.SHIPPED)[0]
        b = V.restate_variance(sums, features, moments, counts, **dict(V.SHIPPED, sigma_var=0.0))[0]
        assert not same(a, b)


# ---- quality, on the committed oracle frame
@pytest.fixture(scope="module")
def quality():
    """spp -> (noisy, old filter, new filter) display RMS against the 4096-spp
    reference over the pixels finite in noisy and reference, and the new output."""
    g = V.golden_frame()
    ref = g["ref"]
    rows = {}
    for n in (16, 64, 256):
        s, f, m = g[f"sums_{n}"], g[f"features_{n}"], g[f"moments_{n}"]
        with np.errstate(all="ignore"):
            noisy = s / n
        mask = np.isfinite(noisy).all(-1) & np.isfinite(ref).all(-1)
        old = D.restate(s, f, n, **D.SHIPPED)[0]
        new = V.restate_variance(s, f, m, n, **V.SHIPPED)[0]
        rows[n] = (D.display_rms(noisy, ref, mask), D.display_rms(old, ref, mask), D.display_rms(new, ref, mask), new)
        print(f"{n} spp: noisy {rows[n][0]:.5f}, rtw_denoise {rows[n][1]:.5f}, rtw_denoise_variance {rows[n][2]:.5f}")
    return rows


def test_the_fixture_is_the_frame_the_issue_describes():
    g = V.golden_frame()
    assert os.path.getsize(V.GOLDEN) < 1_000_000
    assert sorted(g) == sorted(["ref"] + [f"{k}_{n}" for k in ("sums", "features", "moments") for n in (16, 64, 256)])
    for n in (16, 64, 256):
        assert g[f"sums_{n}"].shape == (40, 64, 3) and g[f"features_{n}"].shape == (40, 64, 8)
        assert g[f"moments_{n}"].shape == (40, 64, 2) and g[f"moments_{n}"].dtype == np.float64
        assert (g[f"features_{n}"][..., 7] <= n).all()
    assert g["ref"].shape == (40, 64, 3)


def test_quality_at_256_and_64_spp_the_new_filter_helps(quality):
    for n in (256, 64):
        noisy, _, new, _ = quality[n]
        assert new < noisy, (n, noisy, new)


def test_quality_at_256_spp_the_old_filter_hurts(quality):
    """The defect rtw_denoise_variance closes: the shipped rtw_denoise makes a 256-spp image worse."""
    noisy, old, _, _ = quality[256]
    assert old > noisy, (noisy, old)


def test_quality_at_16_spp_the_new_filter_keeps_up_with_the_old(quality):
    noisy, old, new, _ = quality[16]
    assert new < noisy and new <= 1.05 * old, (noisy, old, new)


def test_quality_every_output_pixel_is_finite(quality):
    for n in (16, 64, 256):
        assert np.isfinite(quality[n][3]).all(), n
