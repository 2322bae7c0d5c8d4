"""Sample windows: rtw_render_window / rtw_render_window_device and the tuning
key "window".  A render taken a window of samples at a time and folded onto
an f64 accumulator is the one-shot render at the same chunk bit for bit, in
both precisions -- "bit for bit" here: identical NaN masks and equal values
elsewhere -- and, in f64, the oracle's."""
import ctypes as C
import functools

import numpy as np
import pytest

import ray_tracing_weekend_amd as rtw
from oracle import oracle as O
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

SEED_SCENE = 0x5EED0001
E_INVALID, E_UNSUPPORTED, E_NO_LIGHTS = _capi.RTW_E_INVALID, _capi.RTW_E_UNSUPPORTED, -3


def _identical(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _as_rendered(sums, prec):
    """The running sums of a window render are f64 in both precisions; an f32
    render is those sums rounded to f32 once (the one-shot fold's rounding)."""
    return sums if prec == rtw.RTW_F64 else sums.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _simple(n=11):
    return rtw.scenes.simple_soa(SEED_SCENE, n)


def _cam(w, h, spp, depth, n=11):
    soa, b = _simple(n)
    return soa, b.copy().with_image_width(w).with_image_height(h).with_samples_per_pixel(spp) \
        .with_max_depth(depth).build()


def _oracle(soa, cam, seed, chunk):          # tests/test_gpu_parity.py's way of calling it
    ocam = O.Camera()
    for name, _ in O.Camera._fields_:
        setattr(ocam, name, getattr(cam.raw, name))
    img, _ = O.render(ocam, O.Scene(**soa.__dict__), seed, chunk=chunk, accel=O.ACCEL_BVH_CACHED)
    return img


def _renderer(soa, prec, chunk=0, tuning=None, **kw):
    r = rtw.Renderer(device=0, precision=prec, **kw)
    if chunk:
        r.set_chunk(chunk)
    for k, v in (tuning or {}).items():
        r.set_tuning(k, v)
    r.set_scene(soa)
    return r


def _one_shot(soa, cam, seed, prec, chunk=0, tuning=None):
    """(image, stats copy) of Renderer.render."""
    with _renderer(soa, prec, chunk, tuning) as r:
        img = r.render(cam, seed)
        st = r.stats
        return img, (st.samples, st.segments, st.lambertian, st.chunk)


def _windows(r, cam, seed, sizes):
    sums, first = None, 0
    for n in sizes:
        sums = r.render_window(cam, seed, first, n, sums)
        first += n
    return sums


def test_f64_ragged_windows_equal_one_shot_and_oracle():
    soa, cam = _cam(37, 21, 7, 50)
    ref, (_, segs, lambs, chunk) = _one_shot(soa, cam, 11, rtw.RTW_F64, chunk=1)
    assert chunk == 1
    with _renderer(soa, rtw.RTW_F64, chunk=1) as r:
        got = _windows(r, cam, 11, (3, 3, 1))
        assert r.stats.samples == 37 * 21 * 1            # stats of a window are that window's
    assert _identical(got, ref)
    assert _identical(got, _oracle(soa, cam, 11, 1))


@pytest.mark.parametrize("prec", [rtw.RTW_F64, rtw.RTW_F32])
def test_fold_window_boundaries(prec):
    """29 + 11 of 40 chunks: 29 = 2 * 12 + 5 (the f64 fold stages 12 chunks
    per pass) = 16 + 13 (f32: 16) -- full passes, a partial one, and a second
    window that starts from the accumulator.  f32: the f64 carry keeps the
    one-shot fold's single rounding: the f64 sums rounded to f32 are the
    one-shot f32 image."""
    soa, cam = _cam(16, 8, 40, 4)
    ref, _ = _one_shot(soa, cam, 5, prec, chunk=1)
    with _renderer(soa, prec, chunk=1) as r:
        got = _windows(r, cam, 5, (29, 11))
    assert _identical(_as_rendered(got, prec), ref)


def test_chunk_two():
    soa, cam = _cam(37, 21, 10, 50)
    ref, (_, _, _, chunk) = _one_shot(soa, cam, 13, rtw.RTW_F64, chunk=2)
    assert chunk == 2
    with _renderer(soa, rtw.RTW_F64, chunk=2) as r:
        got = _windows(r, cam, 13, (4, 6))
        before = got.copy()
        with pytest.raises(rtw.RenderError) as e:
            r.render_window(cam, 13, 3, 2, got)          # not on an item boundary
        assert e.value.code == E_INVALID and _identical(got, before)
    assert _identical(got, ref)
    assert _identical(got, _oracle(soa, cam, 13, 2))


def test_short_last_window_keeps_the_chunk():
    """Chunk 4, windows 4 + 3: the last window is shorter than an item, which
    still starts on the render's own item boundary (sample 4)."""
    soa, cam = _cam(16, 8, 7, 50)
    ref, _ = _one_shot(soa, cam, 15, rtw.RTW_F64, chunk=4)
    with _renderer(soa, rtw.RTW_F64, chunk=4) as r:
        got = _windows(r, cam, 15, (4, 3))
    assert _identical(got, ref)
    with _renderer(soa, rtw.RTW_F64, chunk=4, tuning={"window": 4}) as r:
        assert _identical(r.render(cam, 15), ref)


def test_rank_split_device_form():
    import torch
    soa, cam = _cam(40, 24, 6, 50)
    n = rtw.tiles_for_rank(40, 24, 1, 3) * 64 * 3
    with _renderer(soa, rtw.RTW_F64) as r:
        ref = torch.full((n,), -5.0, dtype=torch.float64, device="cuda:0")
        r.render_device(cam, 9, ref.data_ptr(), n * 8, rank=1, nranks=3)
        acc = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")   # ignored at first == 0
        r.render_window_device(cam, 9, 0, 4, acc.data_ptr(), n * 8, rank=1, nranks=3)
        r.render_window_device(cam, 9, 4, 2, acc.data_ptr(), n * 8, rank=1, nranks=3)
        torch.cuda.synchronize()
        assert r.get_stats().samples == 5 * 64 * 2       # rank 1 of 3: 5 of the 15 (full) tiles, the last window
    assert _identical(acc.cpu().numpy(), ref.cpu().numpy())


@pytest.mark.parametrize("prec", [rtw.RTW_F64, rtw.RTW_F32])
def test_tuning_window_on_every_path(prec):
    soa, cam = _cam(40, 24, 10, 50)
    ref, (samples, segs, lambs, _) = _one_shot(soa, cam, 21, prec)
    for kw in ({}, {"virtual_ranks": 3}):
        with _renderer(soa, prec, tuning={"window": 4}, **kw) as r:
            img = r.render(cam, 21)
            assert (r.stats.samples, r.stats.segments, r.stats.lambertian) == (samples, segs, lambs), kw
            assert r.stats.kernel_ms > 0
        assert _identical(img, ref), kw


def test_tuning_window_auto_keeps_chunk_one():
    """64 x 64 x 40 spp in f64 needs 3.9 MB of chunk-1 sums; partial_max at its
    1 MiB floor holds 10 chunks: without windows the auto chunk grows (another
    fold association), with window = -1 it stays 1 -- the reference's fold."""
    soa, cam = _cam(64, 64, 40, 6)
    _, (_, _, _, chunk) = _one_shot(soa, cam, 31, rtw.RTW_F64, tuning={"partial_max": 1 << 20, "window": 0})
    assert chunk > 1                                     # the case really exceeds the budget
    got, (samples, _, _, chunk) = _one_shot(soa, cam, 31, rtw.RTW_F64, tuning={"partial_max": 1 << 20, "window": -1})
    assert chunk == 1 and samples == 64 * 64 * 40
    assert _identical(got, _oracle(soa, cam, 31, 1))


def _raw_render(r, cam, seed):
    """rtw_render's code and image (a scene that 'panics' still has one)."""
    out = np.zeros((cam.raw.image_height, cam.raw.image_width, 3), np.float64)
    rc = rtw._lib.rtw_render(r.ctx, C.byref(cam.raw), None, C.c_uint64(seed), out.ctypes.data_as(_capi._f64p), None)
    return rc, out


def _raw_windows(r, cam, seed, sizes):
    H, W = cam.raw.image_height, cam.raw.image_width
    sums, first, codes = np.zeros((H, W, 3), np.float64), 0, []
    for n in sizes:
        codes.append(rtw._lib.rtw_render_window(r.ctx, C.byref(cam.raw), C.c_uint64(seed), first, n,
                                                sums.ctypes.data_as(_capi._f64p), None))
        first += n
    return codes, sums


@pytest.mark.parametrize("prec", [rtw.RTW_F64, rtw.RTW_F32])
@pytest.mark.parametrize("scene", ["cornell_box", "perlin_spheres", "light_grid"])
def test_other_kernel_families(scene, prec):
    """Quads, cuboids and emissive materials (cornell_box), textures
    (perlin_spheres: no lights, so every render of it reports the reference's
    panic, RTW_E_NO_LIGHTS, and still has its sums) and the light-grid kernels
    (the 10k-sphere field of tests/test_gpu_c3_c5.py, 488 lights)."""
    if scene == "light_grid":
        soa, b = _simple(50)
        b = b.copy()
    else:
        soa, b = rtw.scenes.named_soa(scene)
    cam = b.with_image_width(24).with_image_height(24).with_samples_per_pixel(6).with_max_depth(8).build()
    expect = E_NO_LIGHTS if scene == "perlin_spheres" else 0
    with _renderer(soa, prec, chunk=1) as r:
        rc, ref = _raw_render(r, cam, 41)
        assert rc == expect
        opts = r.last_kernel()[1]
        codes, got = _raw_windows(r, cam, 41, (4, 2))
        assert codes == [expect, expect] and r.last_kernel()[1] == opts
    assert bool(opts & 2) == (scene == "light_grid")      # kOptLightBvh: the light grid's kernels
    assert bool(opts & 4) == (scene == "perlin_spheres")  # kOptTex
    assert np.isfinite(ref).any() and _identical(_as_rendered(got, prec), ref)


@pytest.mark.parametrize("window", [4, 5])
def test_lpt_windows(window):
    """Longest tiles first with windows: the first window counts the tile
    costs, the later ones (and the second render) take the ordered task list,
    rebuilt for a short last window (5 + 5 + 2); the image does not depend on it."""
    soa, cam = _cam(32, 32, 12, 50)
    ref, (_, segs, _, _) = _one_shot(soa, cam, 51, rtw.RTW_F64, tuning={"lpt": 0})
    with _renderer(soa, rtw.RTW_F64, tuning={"lpt_min_spp": 1, "lpt": 2, "window": window}) as r:
        a = r.render(cam, 51)
        costs = r.tile_costs(cam)                        # counted under the render's own camera key
        assert costs.shape == (16,) and (costs > 0).all()
        b = r.render(cam, 51)
        assert r.stats.segments == segs
        assert np.array_equal(r.tile_costs(cam), costs)  # not counted again: the ordered list ran
    assert _identical(a, ref) and _identical(b, ref)


def test_resume_in_a_new_context():
    world, lights, b = rtw.scenes.simple(SEED_SCENE)
    soa = rtw.flatten(world, lights)
    world_cam = b.with_image_width(24).with_image_height(16).with_samples_per_pixel(9).with_max_depth(50).build()
    ref, _ = _one_shot(soa, world_cam, 61, rtw.RTW_F64)
    with _renderer(soa, rtw.RTW_F64) as r:
        saved = r.render_window(world_cam, 61, 0, 5).copy()
    with _renderer(soa, rtw.RTW_F64) as r:                # a new context: nothing but the sums carries over
        got = r.render_window(world_cam, 61, 5, 4, saved.copy())
    assert _identical(got, ref)
    # render_progressive: the same render 5 + 4, from the world and light lists
    stages = [(done, sums.copy()) for done, sums in
              world_cam.render_progressive(world, lights, 5, seed=61, precision=rtw.RTW_F64)]
    assert [d for d, _ in stages] == [5, 9]
    assert _identical(stages[0][1], saved) and _identical(stages[1][1], ref)


def test_errors_launch_nothing():
    import torch
    soa, cam = _cam(16, 16, 4, 5)
    n = rtw.tiles_for_rank(16, 16, 0, 1) * 64 * 3
    lib = rtw._lib

    def call(r, first, cnt, ptr, nbytes):
        return lib.rtw_render_window_device(r.ctx, C.byref(cam.raw), C.c_uint64(1), 0, 1, first, cnt,
                                            C.c_void_p(ptr) if ptr else None, nbytes, None)
    with _renderer(soa, rtw.RTW_F64) as r:
        acc = torch.full((n,), 2.5, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        assert call(r, 0xFFFFFFFF, 1, acc.data_ptr(), n * 8) == E_INVALID       # first + n overflows u32
        assert call(r, 0, 2, acc.data_ptr(), n * 8 - 8) == E_INVALID            # short accumulator
        assert call(r, 0, 2, None, n * 8) == E_INVALID                          # NULL accumulator
        assert call(r, 4, 0, acc.data_ptr(), n * 8) == 0                        # no samples: nothing to do
        with pytest.raises(rtw.RenderError):
            r.get_stats()                                                       # nothing was ever launched
        assert bool((acc == 2.5).all())
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        assert call(r, 0, 2, acc.data_ptr(), n * 8) == _capi.RTW_E_NO_SCENE
    with _renderer(soa, rtw.RTW_F64, virtual_ranks=2) as r:
        assert call(r, 0, 2, acc.data_ptr(), n * 8) == E_UNSUPPORTED            # windows there: tuning "window"
        sums = np.zeros((16, 16, 3))
        assert lib.rtw_render_window(r.ctx, C.byref(cam.raw), C.c_uint64(1), 0, 2,
                                     sums.ctypes.data_as(_capi._f64p), None) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((acc == 2.5).all())
