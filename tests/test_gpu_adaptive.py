"""Adaptive sampling on the GPU: rtw_render_adaptive / rtw_render_adaptive_device.

The rule is restated in numpy (tests/adaptive_rule.py; checked against the
library's own predicate by tests/test_adaptive_plan_host.py).  The invariant
everything hangs on: each pixel's returned sum is the sequential f64 fold of
its first `counts` samples -- bit for bit what Renderer.render_window(cam,
seed, 0, counts) gives at one sample per item, and in f64 the oracle's render
at that spp.  "Identical" is tests/test_gpu_windows.py's: equal NaN masks,
equal values elsewhere."""
import collections
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_rule as A
import ray_tracing_weekend_amd as rtw
from oracle import oracle as O
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, E_NO_SCENE, E_NO_LIGHTS = (_capi.RTW_E_INVALID, _capi.RTW_E_UNSUPPORTED,
                                                      _capi.RTW_E_NO_SCENE, _capi.RTW_E_NO_LIGHTS)
MIN, WIN, MAX, TOL = 4, 4, 32, 0.125


def _identical(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _renderer(soa, prec, **kw):
    r = rtw.Renderer(device=0, precision=prec, **kw)
    r.set_scene(soa)
    return r


def _hist(counts):
    return sorted(collections.Counter(A.tile_counts(counts)).items())


def _raw_adaptive(r, cam, seed, mn, mx, win, tol):
    """(code, sums, counts, stats): a render the reference would panic on still has its image."""
    H, W = cam.raw.image_height, cam.raw.image_width
    sums, counts, st = np.zeros((H, W, 3)), np.zeros((H, W), np.uint32), _capi.rtw_stats()
    rc = rtw._lib.rtw_render_adaptive(r.ctx, C.byref(cam.raw), C.c_uint64(seed), mn, mx, win, float(tol),
                                      sums.ctypes.data_as(_capi._f64p), counts.ctypes.data_as(_capi._u32p),
                                      C.byref(st))
    return rc, sums, counts, st


def _raw_window(r, cam, seed, first, n):
    H, W = cam.raw.image_height, cam.raw.image_width
    sums = np.zeros((H, W, 3))
    rc = rtw._lib.rtw_render_window(r.ctx, C.byref(cam.raw), C.c_uint64(seed), first, n,
                                    sums.ctypes.data_as(_capi._f64p), None)
    return rc, sums


def _check_invariant(r, cam, seed, sums, counts, expect=0):
    """For each distinct count n: the pixels with that count are the window render [0, n)."""
    for n in np.unique(counts):
        rc, ref = _raw_window(r, cam, seed, 0, int(n))
        assert rc == expect
        at = counts == n
        assert _identical(sums[at], ref[at]), int(n)


@functools.lru_cache(maxsize=None)
def _gpu_samples(prec):
    """[H, W, 32, 3]: the GPU's own per-sample values of the shared case, from
    32 one-sample windows onto zeros."""
    soa, cam = A.simple_scene()
    out = np.zeros((A.H, A.W, A.SAMPLES, 3))
    with _renderer(soa, prec) as r:
        for s in range(A.SAMPLES):
            out[:, :, s] = r.render_window(cam, A.SEED, s, 1, np.zeros((A.H, A.W, 3)))
    out.setflags(write=False)
    return out


def test_f64_counts_are_the_restated_rule_and_sums_the_window_renders():
    soa, cam = A.simple_scene()
    want_sums, want_counts = A.adaptive(A.oracle_samples(), MIN, MAX, WIN, TOL)
    with _renderer(soa, rtw.RTW_F64) as r:
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
        st = r.stats
        samples, chunk = st.samples, st.chunk
        print("f64 tile counts:", _hist(counts), "expected", _hist(want_counts))
        assert np.array_equal(counts, want_counts)
        assert len(np.unique(counts)) >= 3
        assert samples == int(counts.astype(np.uint64).sum()) and chunk == 1
        _check_invariant(r, cam, A.SEED, sums, counts)
    assert _identical(sums, want_sums)
    ocam = A.oracle_camera(cam)
    for n in np.unique(counts):
        ocam.samples_per_pixel = int(n)
        ref, _ = O.render(ocam, O.Scene(**soa.__dict__), A.SEED, chunk=1, accel=O.ACCEL_BVH_CACHED)
        at = counts == n
        assert _identical(sums[at], ref[at]), int(n)


@pytest.mark.parametrize("prec", [rtw.RTW_F64, rtw.RTW_F32])
def test_rule_on_the_gpus_own_samples(prec):
    """Tolerance 0.125 in both precisions.  Measured on an MI355X: f64 5 tiles
    at 4, 4 at 12, 5 at 16, 1 at 32 (the oracle's histogram); f32 5 at 4, 4 at
    12, 5 at 16, 1 at 20 -- four distinct counts, so 0.125 serves f32 too.  The
    assertion asks for at least two."""
    soa, cam = A.simple_scene()
    samples = _gpu_samples(prec)
    want_sums, want_counts = A.adaptive(samples, MIN, MAX, WIN, TOL)
    with _renderer(soa, prec) as r:
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
        assert r.stats.samples == int(counts.astype(np.uint64).sum())
    print("precision", prec, "tile counts:", _hist(counts), "expected", _hist(want_counts))
    assert np.array_equal(counts, want_counts)
    assert len(np.unique(counts)) >= 2
    assert _identical(sums, want_sums)


def test_tolerance_zero_runs_every_varying_tile_to_max():
    soa, cam = A.simple_scene()
    samples = A.oracle_samples()
    with _renderer(soa, rtw.RTW_F64) as r:
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, 0.0)
    assert np.array_equal(counts, A.adaptive(samples, MIN, MAX, WIN, 0.0)[1])
    assert set(np.unique(counts)) == {MIN, MAX}
    y = A.luma(samples)
    varying = ~(np.isnan(y).any(-1) | (y == y[..., :1]).all(-1))       # per pixel, over all 32 samples
    for ty in range(0, A.H, 8):
        for tx in range(0, A.W, 8):
            if varying[ty:ty + 8, tx:tx + 8].any():
                assert counts[ty, tx] == MAX, (ty, tx)


def test_huge_tolerance_stops_at_min_samples():
    soa, cam = A.simple_scene()
    with _renderer(soa, rtw.RTW_F64) as r:
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, 1e30)
        assert r.stats.samples == A.W * A.H * MIN
        ref = r.render_window(cam, A.SEED, 0, MIN)
    assert (counts == MIN).all()
    assert _identical(sums, ref)


def test_depth_zero_renders_nothing_and_stops_at_min_samples():
    """max_depth 0: every sample is 0 and no render kernel runs; zero variance
    is settled even at tolerance 0."""
    soa, b = rtw.scenes.simple_soa(A.SEED_SCENE, A.GRID)
    cam = b.with_image_width(20).with_image_height(12).with_samples_per_pixel(1).with_max_depth(0).build()
    with _renderer(soa, rtw.RTW_F64) as r:
        sums, counts = r.render_adaptive(cam, 1, 2, 6, 2, 0.0)
        assert r.stats.samples == 20 * 12 * 2 and r.stats.segments == 0
    assert (sums == 0).all() and (counts == 2).all()


@pytest.mark.parametrize("prec", [rtw.RTW_F64, rtw.RTW_F32])
def test_min_equals_max_is_the_fixed_render(prec):
    soa, cam = A.simple_scene()
    b = rtw.scenes.simple_soa(A.SEED_SCENE, A.GRID)[1]
    cam7 = b.with_image_width(A.W).with_image_height(A.H).with_samples_per_pixel(7).with_max_depth(A.DEPTH).build()
    with _renderer(soa, prec) as r:
        sums, counts = r.render_adaptive(cam, A.SEED, 7, 7, 3, 0.0)      # cam.samples_per_pixel (32) is not read
        assert r.stats.samples == A.W * A.H * 7
        ref = r.render(cam7, A.SEED)
        assert r.stats.chunk == 1
    assert (counts == 7).all()
    got = sums if prec == rtw.RTW_F64 else sums.astype(np.float32).astype(np.float64)
    assert _identical(got, ref)


@pytest.mark.parametrize("prec", [rtw.RTW_F64, rtw.RTW_F32])
@pytest.mark.parametrize("scene", ["cornell_box", "perlin_spheres"])
def test_other_kernel_families(scene, prec):
    """Quads, cuboids and emission (cornell_box) and textures (perlin_spheres:
    no lights, so the render reports the reference's panic, RTW_E_NO_LIGHTS,
    and still has its sums and counts), 16 x 16, depth 6, 4 / 4 / 16."""
    soa, b = rtw.scenes.named_soa(scene)
    cam = b.with_image_width(16).with_image_height(16).with_samples_per_pixel(1).with_max_depth(6).build()
    expect = E_NO_LIGHTS if scene == "perlin_spheres" else 0
    with _renderer(soa, prec) as r:
        rc, sums, counts, st = _raw_adaptive(r, cam, 41, 4, 16, 4, TOL)
        assert rc == expect
        opts = r.last_kernel()[1]
        print(scene, prec, "tile counts:", _hist(counts))
        assert set(np.unique(counts)) <= {4, 8, 12, 16}
        assert st.samples == int(counts.astype(np.uint64).sum()) and st.chunk == 1
        assert np.isfinite(sums).any()
        _check_invariant(r, cam, 41, sums, counts, expect)
    assert bool(opts & 8) and bool(opts & 4) == (scene == "perlin_spheres")   # kOptPrims, kOptTex


def test_no_side_effects_and_the_device_form():
    import torch
    soa, cam = A.simple_scene()                       # 32 spp: the fixed render counts its tile costs
    with _renderer(soa, rtw.RTW_F64) as r:
        a = r.render(cam, A.SEED)
        kernel = r.last_kernel()
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
        assert r.last_kernel() == kernel
        costs = r.tile_costs(cam)                     # still answers: counted by the first render
        assert costs.shape == (15,) and (costs > 0).sum() >= 10   # (an all-sky tile may cost 0)
        b = r.render(cam, A.SEED)
        assert r.last_kernel() == kernel
        assert np.array_equal(r.tile_costs(cam), costs)
        # the device form into the caller's buffers
        d_sums = torch.full((A.H, A.W, 3), -5.0, dtype=torch.float64, device="cuda:0")
        d_counts = torch.full((A.H, A.W), 77, dtype=torch.int32, device="cuda:0")
        r.render_adaptive_device(cam, A.SEED, MIN, MAX, WIN, TOL, d_sums.data_ptr(), d_sums.numel() * 8,
                                 d_counts.data_ptr(), d_counts.numel() * 4)
        torch.cuda.synchronize()
        assert r.get_stats().samples == int(counts.astype(np.uint64).sum())
        c = r.render(cam, A.SEED)
    assert _identical(a, b) and _identical(a, c)
    assert _identical(d_sums.cpu().numpy(), sums)
    assert np.array_equal(d_counts.cpu().numpy().astype(np.uint32), counts)


def test_cpp_host_mirror_render_adaptive(tmp_path):
    """Camera::render_adaptive (host/rtw_host.hpp) from a C++ program linked
    against the library: the same case as the f64 test above, from the C++
    scene generator's object lists -- the restated counts, the folded sums."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    lib_dir = os.path.join(root, "ray_tracing_weekend_amd", "lib")
    exe, out = str(tmp_path / "adaptive_mirror_check"), str(tmp_path / "out.bin")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(root, "ray_tracing_weekend_amd", "csrc"),
                    "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "native", "adaptive_mirror_check.cpp"), "-o", exe,
                    "-L", lib_dir, "-lrtw", "-Wl,-rpath," + lib_dir], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, np.float64).reshape(A.H, A.W, 4)
    want_sums, want_counts = A.adaptive(A.oracle_samples(), MIN, MAX, WIN, TOL)
    assert np.array_equal(got[..., 3], want_counts.astype(np.float64))
    assert _identical(got[..., :3], want_sums)


def test_partial_max_cuts_passes_into_sub_passes():
    """partial_max at its 1 MiB floor holds two samples of a 128 x 128 f64
    image (256 tiles, 393216 bytes a sample): pass 0 (5 samples) runs as 2 + 2 +
    1, the later passes shrink with the active list; the result is the same."""
    soa, b = rtw.scenes.simple_soa(A.SEED_SCENE, A.GRID)
    cam = b.with_image_width(128).with_image_height(128).with_samples_per_pixel(1).with_max_depth(4).build()
    with _renderer(soa, rtw.RTW_F64) as r:
        ref_sums, ref_counts = r.render_adaptive(cam, 3, 5, 13, 3, TOL)
        samples = r.stats.samples
    with _renderer(soa, rtw.RTW_F64) as r:
        r.set_tuning("partial_max", 1 << 20)
        sums, counts = r.render_adaptive(cam, 3, 5, 13, 3, TOL)
        assert r.stats.samples == samples
    print("128 x 128 tile counts:", _hist(counts))
    assert np.array_equal(counts, ref_counts) and _identical(sums, ref_sums)
    assert len(np.unique(counts)) >= 2


def test_errors_launch_nothing():
    import torch
    soa, cam = A.simple_scene()
    lib = rtw._lib
    n = A.W * A.H
    sums, counts = np.full((A.H, A.W, 3), 2.5), np.full((A.H, A.W), 9, np.uint32)
    sp, cp = sums.ctypes.data_as(_capi._f64p), counts.ctypes.data_as(_capi._u32p)
    d_sums = torch.full((n * 3,), 2.5, dtype=torch.float64, device="cuda:0")
    d_counts = torch.full((n,), 9, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()

    def host(r, mn=MIN, mx=MAX, win=WIN, tol=TOL, s=sp, c=cp):
        return lib.rtw_render_adaptive(r.ctx, C.byref(cam.raw), C.c_uint64(1), mn, mx, win, tol, s, c, None)

    def dev(r, mn=MIN, mx=MAX, win=WIN, tol=TOL, s=d_sums.data_ptr(), sb=n * 24, c=d_counts.data_ptr(), cb=n * 4):
        return lib.rtw_render_adaptive_device(r.ctx, C.byref(cam.raw), C.c_uint64(1), mn, mx, win, tol,
                                              C.c_void_p(s) if s else None, sb, C.c_void_p(c) if c else None, cb,
                                              None)
    with _renderer(soa, rtw.RTW_F64) as r:
        for f in (host, dev):
            assert f(r, mn=1) == E_INVALID and f(r, mn=0) == E_INVALID
            assert f(r, mn=8, mx=7) == E_INVALID
            assert f(r, win=0) == E_INVALID
            assert f(r, tol=-0.125) == E_INVALID
            assert f(r, tol=float("nan")) == E_INVALID and f(r, tol=float("inf")) == E_INVALID
            assert f(r, s=None) == E_INVALID and f(r, c=None) == E_INVALID
        assert dev(r, sb=n * 24 - 8) == E_INVALID and dev(r, cb=n * 4 - 4) == E_INVALID
        assert lib.rtw_render_adaptive(r.ctx, None, C.c_uint64(1), MIN, MAX, WIN, TOL, sp, cp, None) == E_INVALID
        # an image too wide for the kernels is refused before any allocation; one without pixels renders nothing
        wide, empty, st = _capi.rtw_camera(), _capi.rtw_camera(), _capi.rtw_stats()
        C.pointer(wide)[0] = cam.raw
        C.pointer(empty)[0] = cam.raw
        wide.image_width, empty.image_height, st.samples = 70000, 0, 5
        assert lib.rtw_render_adaptive(r.ctx, C.byref(wide), C.c_uint64(1), MIN, MAX, WIN, TOL, sp, cp, None) \
            == E_UNSUPPORTED
        assert lib.rtw_render_adaptive_device(r.ctx, C.byref(wide), C.c_uint64(1), MIN, MAX, WIN, TOL,
                                              C.c_void_p(d_sums.data_ptr()), n * 24,
                                              C.c_void_p(d_counts.data_ptr()), n * 4, None) == E_UNSUPPORTED
        assert lib.rtw_render_adaptive(r.ctx, C.byref(empty), C.c_uint64(1), MIN, MAX, WIN, TOL, sp, cp,
                                       C.byref(st)) == 0
        assert st.samples == 0 and st.chunk == 1
        r.set_chunk(2)
        assert host(r) == E_INVALID and dev(r) == E_INVALID           # an explicit chunk above 1
        with pytest.raises(rtw.RenderError):
            r.get_stats()                                             # nothing was ever launched
        r.set_chunk(1)
        a = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)        # chunk 1 is what it renders at anyway
        r.set_chunk(0)
        b = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)        # and the context still renders
        assert np.array_equal(a[1], b[1]) and _identical(a[0], b[0]) and len(np.unique(b[1])) >= 3
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        assert host(r) == E_NO_SCENE and dev(r) == E_NO_SCENE
    with _renderer(soa, rtw.RTW_F64, virtual_ranks=2) as r:
        assert host(r) == E_UNSUPPORTED and dev(r) == E_UNSUPPORTED
        r.render(cam, A.SEED)                                         # it renders its own way afterwards
    torch.cuda.synchronize()
    assert (sums == 2.5).all() and (counts == 9).all()
    assert bool((d_sums == 2.5).all()) and bool((d_counts == 9).all())
