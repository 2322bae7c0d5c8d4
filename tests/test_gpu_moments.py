"""The per-pixel luminance moments on the GPU: rtw_render_window_moments and
rtw_adaptive_moments with their device forms.

moments [H, W, 2] = {S1, S2}: the sequential f64 sums of Y and Y * Y of each
pixel's samples, Y = ((0.2126 r) + (0.7152 g)) + (0.0722 b), restated here with
adaptive_rule.luma and np.cumsum (left to right).  The shared case is
adaptive_rule's: scenes::simple at 36 x 20 (5 x 3 tiles, partial on both axes),
32 samples, whose per-sample values come from the oracle once.  "Identical" is
tests/test_gpu_windows.py's: equal NaN masks, equal values elsewhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import adaptive_rule as A
import ray_tracing_weekend_amd as rtw
import test_gpu_tile_cull as TC
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

INV, UNSUPPORTED = _capi.RTW_E_INVALID, _capi.RTW_E_UNSUPPORTED


def _identical(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _renderer(soa, prec=rtw.RTW_F64, **kw):
    r = rtw.Renderer(device=0, precision=prec, **kw)
    r.set_scene(soa)
    return r


def moments_of(samples):
    """[H, W, S, 2]: the running {S1, S2} of per-sample values [H, W, S, 3]."""
    y = A.luma(samples)
    with np.errstate(all="ignore"):
        return np.stack([np.cumsum(y, axis=2), np.cumsum(y * y, axis=2)], -1)


@functools.lru_cache(maxsize=None)
def oracle_moments():
    m = moments_of(A.oracle_samples())
    m.setflags(write=False)
    return m


# ------------------------------------------------------------------ windows
def test_f64_window_moments_are_the_oracles():
    soa, cam = A.simple_scene()
    with _renderer(soa) as r:
        sums, moments = r.render_window_moments(cam, A.SEED, 0, A.SAMPLES)
        samples, chunk = r.stats.samples, r.stats.chunk
    assert sums.shape == (A.H, A.W, 3) and moments.shape == (A.H, A.W, 2) and moments.dtype == np.float64
    assert _identical(sums, A.fold(A.oracle_samples())[:, :, -1, :])
    assert _identical(moments, oracle_moments()[:, :, -1, :])
    assert (samples, chunk) == (A.W * A.H * A.SAMPLES, 1)
    assert (moments[np.isfinite(moments).all(-1)] > 0).all()


@pytest.mark.parametrize("prec", [rtw.RTW_F64, rtw.RTW_F32], ids=("f64", "f32"))
def test_windows_compose_bit_for_bit(prec):
    soa, cam = A.simple_scene()
    with _renderer(soa, prec) as r:
        whole = r.render_window_moments(cam, A.SEED, 0, A.SAMPLES)
        sums, moments, first = None, None, 0
        for n in (5, 11, 16):
            sums, moments = r.render_window_moments(cam, A.SEED, first, n, sums, moments)
            first += n
            assert r.stats.samples == A.W * A.H * n
        # the running arrays are continued in place, and a window of no samples changes nothing
        again = r.render_window_moments(cam, A.SEED, first, 0, sums, moments)
        assert again[0] is sums and again[1] is moments
    assert first == A.SAMPLES
    assert _identical(sums, whole[0]) and _identical(moments, whole[1])
    if prec == rtw.RTW_F64:
        assert _identical(moments[:, :, :], oracle_moments()[:, :, -1, :])


def test_f32_moments_are_the_gpus_own_samples_restated():
    soa, cam = A.simple_scene()
    n = 8
    per_sample = np.zeros((A.H, A.W, n, 3))
    with _renderer(soa, rtw.RTW_F32) as r:
        for s in range(n):
            per_sample[:, :, s] = r.render_window(cam, A.SEED, s, 1, np.zeros((A.H, A.W, 3)))
        window = r.render_window(cam, A.SEED, 0, n)
        sums, moments = r.render_window_moments(cam, A.SEED, 0, n)
    # (an f32 context's per-sample values are f32 values, widened exactly)
    assert np.array_equal(per_sample[np.isfinite(per_sample)],
                          per_sample[np.isfinite(per_sample)].astype(np.float32).astype(np.float64))
    assert _identical(moments, moments_of(per_sample)[:, :, -1, :])
    assert _identical(sums, A.fold(per_sample)[:, :, -1, :]) and _identical(sums, window)


def test_sub_windows_do_not_show():
    """partial_max at its 1 MiB floor holds two samples of a 128 x 128 f64
    image's chunk sums: a window of 5 samples runs as 2 + 2 + 1."""
    soa, b = rtw.scenes.simple_soa(A.SEED_SCENE, A.GRID)
    cam = b.copy().with_image_width(128).with_image_height(128).with_max_depth(8).build()
    got = {}
    for budget in (None, 1 << 20):
        with _renderer(soa) as r:
            if budget:
                r.set_tuning("partial_max", budget)
            got[budget] = r.render_window_moments(cam, A.SEED, 0, 5)
            assert r.stats.samples == 128 * 128 * 5
            if not budget:
                # (under the small budget a plain window would take a larger chunk: another fold)
                window = r.render_window(cam, A.SEED, 0, 5)
                assert r.stats.chunk == 1 and _identical(got[budget][0], window)
    assert _identical(got[None][0], got[1 << 20][0]) and _identical(got[None][1], got[1 << 20][1])


def test_tile_cull_does_not_show():
    """test_gpu_tile_cull's flagship camera: tiles of it are provably empty."""
    cam, soa = TC._cam(), TC._scene()[0]
    got = {}
    for cull in (1, 0):
        with TC._renderer(cull) as r:
            r.render(cam, TC.SEED)
            if cull:
                assert r.culled_tiles() >= 1
            got[cull] = r.render_window_moments(cam, TC.SEED, 0, 3)
            got[cull] += (r.render_window(cam, TC.SEED, 0, 3),)
    assert _identical(got[1][0], got[0][0]) and _identical(got[1][1], got[0][1])
    assert _identical(got[1][0], got[1][2]) and _identical(got[0][0], got[0][2])
    # a provably empty tile is the background's, sample after sample
    y = float(A.luma(np.array([float(x) for x in cam.background])))
    sky = (got[1][1][..., 0] == (y + y) + y) & (got[1][1][..., 1] == (y * y + y * y) + y * y)
    assert soa is TC._scene()[0] and sky.sum() >= 64


# ----------------------------------------------------------------- adaptive
ADAPTIVE = (8, 32, 8, 1.0 / 64)


def _moments_at(counts):
    idx = (counts.astype(np.int64) - 1)[..., None, None]
    return np.take_along_axis(oracle_moments(), np.broadcast_to(idx, (A.H, A.W, 1, 2)), axis=2)[:, :, 0, :]


def test_adaptive_moments_are_the_sums_over_each_pixels_counts():
    soa, cam = A.simple_scene()
    with _renderer(soa) as r:
        sums, counts = r.render_adaptive(cam, A.SEED, *ADAPTIVE)
        moments = r.adaptive_moments()
        # a moments window in between leaves the adaptive state alone
        r.render_window_moments(cam, A.SEED, 0, 3)
        again = r.adaptive_moments()
    assert len(np.unique(counts)) >= 2
    want_sums, want_counts = A.adaptive(A.oracle_samples(), *ADAPTIVE)
    assert np.array_equal(counts, want_counts) and _identical(sums, want_sums)
    assert moments.shape == (A.H, A.W, 2) and _identical(moments, _moments_at(counts))
    assert _identical(again, moments)


def test_adaptive_moments_device_entry_on_a_side_stream():
    import torch
    soa, cam = A.simple_scene()
    with _renderer(soa) as r:
        _, counts = r.render_adaptive(cam, A.SEED, *ADAPTIVE)
        host = r.adaptive_moments()
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            d = torch.full((A.H * A.W * 2 + 2,), -77.0, dtype=torch.float64, device="cuda:0")
            r.adaptive_moments_device(d.data_ptr(), A.H * A.W * 16)
        side.synchronize()
        got = d.cpu().numpy()
    assert _identical(got[:-2].reshape(A.H, A.W, 2), host) and (got[-2:] == -77.0).all()
    assert _identical(host, _moments_at(counts))


def test_window_moments_device_entry_on_a_side_stream():
    import torch
    soa, cam = A.simple_scene()
    px = A.H * A.W
    with _renderer(soa) as r:
        host = r.render_window_moments(cam, A.SEED, 0, 12)
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            d_sums = torch.full((px * 3 + 2,), -77.0, dtype=torch.float64, device="cuda:0")
            d_mom = torch.full((px * 2 + 2,), -77.0, dtype=torch.float64, device="cuda:0")
            r.render_window_moments_device(cam, A.SEED, 0, 5, d_sums.data_ptr(), px * 24, d_mom.data_ptr(), px * 16)
            r.render_window_moments_device(cam, A.SEED, 5, 7, d_sums.data_ptr(), px * 24, d_mom.data_ptr(), px * 16)
        side.synchronize()
        s, m = d_sums.cpu().numpy(), d_mom.cpu().numpy()
    assert _identical(s[:-2].reshape(A.H, A.W, 3), host[0]) and _identical(m[:-2].reshape(A.H, A.W, 2), host[1])
    assert (s[-2:] == -77.0).all() and (m[-2:] == -77.0).all()


# ---------------------------------------------------------------- refusals
def test_refusals_write_nothing():
    import torch
    soa, cam = A.simple_scene()
    lib = rtw._lib
    px = A.H * A.W
    sums, moments = np.full((A.H, A.W, 3), -77.0), np.full((A.H, A.W, 2), -77.0)
    dp = lambda a: None if a is None else a.ctypes.data_as(_capi._f64p)   # noqa: E731

    def window(r, s=sums, m=moments, first=0, n=2):
        return lib.rtw_render_window_moments(r.ctx, C.byref(cam.raw), C.c_uint64(A.SEED), first, n, dp(s), dp(m), None)

    with _renderer(soa) as r:
        # before any adaptive render
        assert lib.rtw_adaptive_moments(r.ctx, dp(moments)) == INV
        with pytest.raises(rtw.RenderError):
            r.adaptive_moments()
        assert window(r, s=None) == INV and window(r, m=None) == INV
        assert window(r, first=0xFFFFFFFF, n=2) == INV
        d_sums = torch.full((px * 3,), -77.0, dtype=torch.float64, device="cuda:0")
        d_mom = torch.full((px * 2,), -77.0, dtype=torch.float64, device="cuda:0")

        def device(s=d_sums.data_ptr(), sb=px * 24, m=d_mom.data_ptr(), mb=px * 16):
            return lib.rtw_render_window_moments_device(r.ctx, C.byref(cam.raw), C.c_uint64(A.SEED), 0, 2,
                                                        C.c_void_p(s) if s else None, sb,
                                                        C.c_void_p(m) if m else None, mb, None)
        assert device(s=None) == INV and device(m=None) == INV
        assert device(sb=px * 24 - 8) == INV and device(mb=px * 16 - 8) == INV
        r.set_chunk(2)
        assert window(r) == INV and device() == INV
        r.set_chunk(1)
        torch.cuda.synchronize()
        assert bool((d_sums == -77.0).all()) and bool((d_mom == -77.0).all())
        assert (sums == -77.0).all() and (moments == -77.0).all()
        assert window(r) == 0 and (sums != -77.0).all() and (moments != -77.0).all()
        # after an adaptive render: short or NULL device buffers; after rtw_set_scene: none again
        r.render_adaptive(cam, A.SEED, *ADAPTIVE)
        assert lib.rtw_adaptive_moments(r.ctx, None) == INV
        assert lib.rtw_adaptive_moments_device(r.ctx, None, px * 16, None) == INV
        assert lib.rtw_adaptive_moments_device(r.ctx, C.c_void_p(d_mom.data_ptr()), px * 16 - 8, None) == INV
        torch.cuda.synchronize()
        assert bool((d_mom == -77.0).all())
        assert lib.rtw_adaptive_moments_device(r.ctx, C.c_void_p(d_mom.data_ptr()), px * 16, None) == 0
        r.set_scene(soa)
        moments[:] = -77.0
        assert lib.rtw_adaptive_moments(r.ctx, dp(moments)) == INV and (moments == -77.0).all()
    with _renderer(soa, virtual_ranks=2) as r:
        sums[:], moments[:] = -77.0, -77.0
        assert window(r) == UNSUPPORTED
        assert lib.rtw_adaptive_moments(r.ctx, dp(moments)) == UNSUPPORTED
        assert (sums == -77.0).all() and (moments == -77.0).all()
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        assert window(r) == _capi.RTW_E_NO_SCENE
