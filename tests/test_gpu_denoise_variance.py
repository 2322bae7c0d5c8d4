"""The variance-guided denoiser (rtw_denoise_variance) on the GPU against the
numpy restatement of tests/denoise_variance_cases.py: made-up frames of every
kind of pixel and moment at sizes around the tile, the staged against the
direct form, the device entry on a side stream, the pipeline moments window ->
feature pass -> denoise, isolation from renders, queries, feature passes and
the old filter, the refusals, the stats and the CLI.  Every comparison is bit
for bit up to the sign of zero with equal NaN masks (feature_cases.same)."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import denoise_cases as D
import denoise_variance_cases as V
import feature_cases as F
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

same = F.same
INV = _capi.RTW_E_INVALID
SIZES = ((1, 1), (5, 3), (37, 19), (70, 45))
SPP = 16


def where_differs(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    return np.argwhere(bad)[:6].tolist()


def param_sets():
    """The shipped defaults; iterations 1 and 7 (step 64 is beyond every image
    here); sigma_var 0; demodulate off; fill off; and two mixes of them with
    normal_power_log2 0."""
    return [dict(V.SHIPPED),
            dict(V.SHIPPED, iterations=1),
            dict(V.SHIPPED, iterations=7),
            dict(V.SHIPPED, sigma_var=0.0),
            dict(V.SHIPPED, demodulate=0),
            dict(V.SHIPPED, fill_nonfinite=0),
            dict(V.SHIPPED, iterations=3, normal_power_log2=0, sigma_var=0.0, demodulate=0, fill_nonfinite=0),
            dict(V.SHIPPED, iterations=7, normal_power_log2=0, sigma_var=3.0, demodulate=0)]


def frame(width, height):
    sums, features, _ = D.synthetic(width, height)
    return sums, features, V.synthetic_moments(width, height), V.counts_with_ones(width, height)


def key_of(params):
    return tuple(sorted(params.items()))


@functools.lru_cache(maxsize=None)
def expected(width, height, per_pixel, key):
    sums, features, moments, counts = frame(width, height)
    return V.restate_variance(sums, features, moments, counts if per_pixel else SPP, **dict(key))


# ------------------------------------------------------- 1. synthetic parity
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("per_pixel", (False, True), ids=("spp", "counts"))
def test_host_entry_is_the_restatement(size, per_pixel):
    width, height = size
    sums, features, moments, counts = frame(width, height)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        for params in param_sets():
            want, filled, left = expected(width, height, per_pixel, key_of(params))
            got = r.denoise_variance(sums, features, moments, counts if per_pixel else SPP, **params)
            assert got.shape == (height, width, 3) and got.dtype == np.float64
            assert same(got, want), (params, where_differs(got, want))
            st = r.denoise_stats()
            assert (st.filled, st.left_nonfinite, st.iterations) == (filled, left, params["iterations"]), params
            assert st.kernel_ms > 0


def test_the_synthetic_cases_are_not_vacuous():
    """The filter changes the image, fills pixels when asked to and leaves some
    non-finite; every parameter set gives another picture; pixels with and
    without a variance, of one sample and with non-finite moments all occur."""
    sums, features, moments, counts = frame(70, 45)
    outs = []
    for params in param_sets():
        want, filled, left = expected(70, 45, True, key_of(params))
        assert (filled > 0) == bool(params["fill_nonfinite"]) and left > 0
        outs.append(want)
    assert sum(same(a, b) for a, b in itertools.combinations(outs, 2)) == 0
    with np.errstate(all="ignore"):
        plain = np.where(counts[..., None] > 0, sums / counts[..., None].astype(np.float64), 0.0)
    assert not same(outs[0], plain)
    has_var = V.restate_variance(sums, features, moments, counts, details=True, **V.SHIPPED)[3]
    assert has_var.sum() >= 1000 and (~has_var).sum() >= 100
    assert (counts == 1).sum() >= 20 and (~np.isfinite(moments).all(-1)).sum() >= 20
    # without the moments the result is another: the old filter without a colour stop
    old = D.restate(sums, features, counts, **{**D.SHIPPED, "sigma_colour": 0.0})[0]
    assert not same(outs[0], old)


def test_every_count_one_is_the_old_filter_without_a_colour_stop():
    sums, features, moments, counts = frame(37, 19)
    ones = np.where(counts > 0, 1, 0).astype(np.uint32)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        new = r.denoise_variance(sums, features, moments, ones)
        old = r.denoise(sums, features, ones, sigma_colour=0.0)
    assert same(new, old) and same(old, D.restate(sums, features, ones, **{**D.SHIPPED, "sigma_colour": 0.0})[0])


# ------------------------------------------------------ 2. LDS against direct
def test_staged_and_direct_forms_are_identical():
    sums, features, moments, counts = frame(70, 45)
    # tile + halo fit the LDS up to step 4 (80 bytes a pixel): the first three iterations
    for iterations, staged in ((1, 1), (2, 2), (3, 3), (4, 3), (7, 3)):
        params = dict(V.SHIPPED, iterations=iterations)
        got = {}
        for lds in (0, 2):
            with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
                r.set_tuning("denoise_lds", lds)
                got[lds] = r.denoise_variance(sums, features, moments, counts, **params)
                st = r.denoise_stats()
            assert (st.iterations, st.lds_iterations) == (iterations, staged if lds else 0)
        want = V.restate_variance(sums, features, moments, counts, **params)[0]
        assert same(got[0], got[2]), where_differs(got[0], got[2])
        assert same(got[0], want), where_differs(got[0], want)
    # the default plan stages steps 1 and 2 and is the same filter
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        assert same(r.denoise_variance(sums, features, moments, counts, **params), want)
        assert r.denoise_stats().lds_iterations == 2


# ------------------------------------------------------------ 3. device entry
def test_device_entry_on_a_side_stream_is_the_host_entry():
    import torch
    width, height = 37, 19
    sums, features, moments, counts = frame(width, height)
    with np.errstate(all="ignore"):
        sums32 = sums.astype(np.float32)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            d_feat = torch.from_numpy(np.array(features)).to("cuda:0")
            d_mom = torch.from_numpy(np.array(moments)).to("cuda:0")
            d_counts = torch.from_numpy(counts.astype(np.int32)).to("cuda:0")
            d64 = r.denoise_variance(torch.from_numpy(np.array(sums)).to("cuda:0"), d_feat, d_mom, d_counts)
            d32 = r.denoise_variance(torch.from_numpy(sums32).to("cuda:0"), d_feat, d_mom, SPP)
            assert d64.is_cuda and d64.dtype == torch.float64 and tuple(d64.shape) == (height, width, 3)
        side.synchronize()
        h64 = r.denoise_variance(sums, features, moments, counts)
        h32 = r.denoise_variance(sums32.astype(np.float64), features, moments, SPP)
    assert same(d64.cpu().numpy(), h64) and same(d32.cpu().numpy(), h32)
    assert same(h64, V.restate_variance(sums, features, moments, counts, **V.SHIPPED)[0])
    assert same(h32, V.restate_variance(sums32, features, moments, SPP, **V.SHIPPED)[0])
    assert not same(h32, h64)


def test_device_entry_refuses_bad_arrays_and_writes_nothing():
    import torch
    width, height = 10, 6
    px = width * height
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        d_sums = torch.ones(px * 3 + 2, dtype=torch.float64, device="cuda:0")
        d_feat = torch.ones(px * 8 + 2, dtype=torch.float64, device="cuda:0")
        d_mom = torch.ones(px * 2 + 2, dtype=torch.float64, device="cuda:0")
        d_out = torch.full((px * 3 + 2,), -77.0, dtype=torch.float64, device="cuda:0")

        def call(sums=d_sums.data_ptr(), sums_bytes=px * 24, feat=d_feat.data_ptr(), feat_bytes=px * 64,
                 mom=d_mom.data_ptr(), mom_bytes=px * 16, out=d_out.data_ptr(), out_bytes=px * 24,
                 prec=_capi.RTW_F64):
            return rtw._lib.rtw_denoise_variance_device(
                r.ctx, C.c_void_p(sums), prec, sums_bytes, C.c_void_p(feat), feat_bytes,
                C.c_void_p(mom) if mom else None, mom_bytes, None, 0, 4, width, height, None, C.c_void_p(out),
                out_bytes, None)
        assert call(sums_bytes=px * 24 - 8) == INV and call(feat_bytes=px * 64 - 8) == INV
        assert call(mom_bytes=px * 16 - 8) == INV and call(mom=None) == INV
        assert call(out_bytes=px * 24 - 8) == INV
        assert call(sums_bytes=px * 12) == INV and call(sums_bytes=px * 12, prec=7) == INV
        assert call(feat=d_feat.data_ptr() + 8) == INV and call(out=d_out.data_ptr() + 8) == INV
        assert call(sums=d_sums.data_ptr() + 8) == INV and call(mom=d_mom.data_ptr() + 8) == INV
        assert call(out=d_sums.data_ptr()) == INV and call(out=d_mom.data_ptr()) == INV     # out is an input
        assert call(out=d_feat.data_ptr() + px * 64 - 16) == INV                   # ... or overlaps one's end
        torch.cuda.synchronize()
        assert bool((d_out == -77.0).all()) and bool((d_sums == 1.0).all()) and bool((d_feat == 1.0).all())
        assert bool((d_mom == 1.0).all())
        with pytest.raises(rtw.RenderError):
            r.denoise_stats()                                                      # nothing ran
        assert call() == 0
        torch.cuda.synchronize()
        assert bool((d_out[:px * 3] != -77.0).all()) and bool((d_out[px * 3:] == -77.0).all())


# ---------------------------------------------------------------- 4. pipeline
def _simple_camera(spp=SPP):
    soa, b = F.scene("simple")
    cam = b.copy().with_image_width(40).with_image_height(24).with_samples_per_pixel(spp).with_max_depth(50).build()
    return soa, cam


def test_moments_features_denoise_is_the_restatement_of_the_gpus_own_buffers():
    soa, cam = _simple_camera()
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        sums, moments = r.render_window_moments(cam, F.SEED, 0, SPP)
        features, _ = r.render_features(cam, F.SEED)
        got = r.denoise_variance(sums, features, moments, SPP)
        a_sums, a_counts = r.render_adaptive(cam, F.SEED, 4, SPP, 4, 0.02)
        a_moments = r.adaptive_moments()
        a_features, _ = r.render_features(cam, F.SEED, 0, SPP, counts=a_counts)
        a_got = r.denoise_variance(a_sums, a_features, a_moments, a_counts)
    want, _, _, has_var, _ = V.restate_variance(sums, features, moments, SPP, details=True, **V.SHIPPED)
    assert same(got, want), where_differs(got, want)
    assert has_var.mean() > 0.9 and not same(got, sums / SPP)
    assert len(np.unique(a_counts)) >= 2            # the adaptive counts differ between tiles
    a_want = V.restate_variance(a_sums, a_features, a_moments, a_counts, **V.SHIPPED)[0]
    assert same(a_got, a_want), where_differs(a_got, a_want)


def test_render_denoised_variance_is_the_three_calls():
    world, lights, b = rtw.scenes.simple(0x5EED0001)
    cam = b.with_image_width(40).with_image_height(24).with_samples_per_pixel(SPP).with_max_depth(50).build()
    params = dict(V.SHIPPED, iterations=3)
    got = cam.render_denoised(world, lights, seed=F.SEED, variance=True, **params)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(rtw.flatten(world, lights))
        sums, moments = r.render_window_moments(cam, F.SEED, 0, SPP)
        features, _ = r.render_features(cam, F.SEED)
        want = r.denoise_variance(sums, features, moments, SPP, **params)
    assert got.shape == (24, 40, 3) and same(got, want)
    assert same(want, V.restate_variance(sums, features, moments, SPP, **params)[0])
    # the default is today's three calls
    old = cam.render_denoised(world, lights, seed=F.SEED)
    assert not same(old, got)


# --------------------------------------------------------------- 5. isolation
def test_a_variance_denoise_leaves_everything_else_alone():
    soa, cam = _simple_camera(4)
    rays = np.random.default_rng(5).normal(size=(64, 6))
    rays[:, :3] = (13.0, 2.0, 3.0)
    sums_s, features_s, moments_s, counts_s = frame(37, 19)
    big = frame(70, 45)
    old_want = D.restate(*D.synthetic(70, 45), **D.SHIPPED)[0]
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        img0, (h0, i0), (f0, _) = r.render(cam, F.SEED), r.hit_rays(rays), r.render_features(cam, F.SEED)
        old0 = r.denoise(*D.synthetic(70, 45))
        first = r.denoise_variance(sums_s, features_s, moments_s, counts_s)
        img1, (h1, i1), (f1, _) = r.render(cam, F.SEED), r.hit_rays(rays), r.render_features(cam, F.SEED)
        old1 = r.denoise(*D.synthetic(70, 45))
        # a second variance denoise of another (smaller, then larger) size reuses the state
        small = r.denoise_variance(*frame(5, 3))
        large = r.denoise_variance(*big)
        old2 = r.denoise(*D.synthetic(70, 45))
        again = r.denoise_variance(sums_s, features_s, moments_s, counts_s)
    assert same(img0, img1) and same(h0, h1) and np.array_equal(i0, i1) and same(f0, f1)
    # the old filter is what it was: the restatement of tests/denoise_cases.py
    assert same(old0, old_want) and same(old1, old_want) and same(old2, old_want)
    assert same(first, expected(37, 19, True, key_of(V.SHIPPED))[0]) and same(again, first)
    assert same(small, expected(5, 3, True, key_of(V.SHIPPED))[0])
    assert same(large, expected(70, 45, True, key_of(V.SHIPPED))[0])


# --------------------------------------------------------------- 6. refusals
def test_refusals_on_a_context():
    lib = rtw._lib
    s, f, m, o = np.ones((4, 4, 3)), np.ones((4, 4, 8)), np.ones((4, 4, 2)), np.full((4, 4, 3), -77.0)
    cnt = np.ones((4, 4), np.uint32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    nan, inf = float("nan"), float("inf")
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        def call(sums=s, feat=f, mom=m, counts=None, spp=4, w=4, h=4, out=o, **fields):
            p = rtw.DenoiseVarianceParams(**fields).raw
            return lib.rtw_denoise_variance(r.ctx, vp(sums), vp(feat), vp(mom), vp(counts), spp, w, h, C.byref(p),
                                            vp(out))
        assert call(sums=None) == INV and call(feat=None) == INV and call(mom=None) == INV and call(out=None) == INV
        assert call(spp=0) == INV and call(spp=0, counts=cnt) == 0
        assert call(w=1 << 16, h=1) == INV and call(w=1, h=1 << 16) == INV
        for bad in (dict(iterations=0), dict(iterations=17), dict(normal_power_log2=11), dict(sigma_var=-1.0),
                    dict(sigma_var=nan), dict(sigma_var=inf), dict(sigma_depth=0.0), dict(sigma_depth=-1.0),
                    dict(sigma_depth=nan), dict(sigma_depth=inf), dict(demodulate=2), dict(fill_nonfinite=2)):
            o[:] = -77.0
            assert call(**bad) == INV, bad
            assert (o == -77.0).all() and lib.rtw_last_error(r.ctx)
        assert call(iterations=16, normal_power_log2=10, sigma_var=0.0) == 0
        assert (o != -77.0).all()
        # NULL parameters are the defaults
        st = _capi.rtw_denoise_stats()
        assert lib.rtw_denoise_variance(r.ctx, vp(s), vp(f), vp(m), None, 4, 4, 4, None, vp(o)) == 0
        assert lib.rtw_get_denoise_stats(r.ctx, C.byref(st)) == 0 and st.iterations == 5


# ------------------------------------------------------------------ the CLI
def test_cli_writes_the_variance_denoised_image(tmp_path):
    """rtw simple --denoise PATH --denoise-variance (the C++ mirror's
    render_window_moments and denoise_variance, the default parameters): the PPM
    is the Python mirror's means through the same writer."""
    width, height, spp, seed = 40, 24, 16, 0x5EED0001
    cfg = tmp_path / "Config.toml"
    cfg.write_text(f"[image]\nimage_width = {width}\nimage_height = {height}\nsamples_per_pixel = {spp}\n"
                   "max_depth = 50\n")
    exe = os.path.join(os.path.dirname(_capi.LIB_PATH), "rtw")
    run = subprocess.run([exe, "simple", "--seed", str(seed), "--config", str(cfg), "--out", str(tmp_path / "image.ppm"),
                          "--denoise", str(tmp_path / "clean.ppm"), "--denoise-variance"], capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    soa, b = rtw.scenes.simple_soa(seed)
    cam = b.with_vfov(40.0).with_aspect_ratio(width / height).with_max_depth(50).with_image_width(width) \
           .with_image_height(height).with_samples_per_pixel(spp).build()
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        sums, moments = r.render_window_moments(cam, seed, 0, spp)
        features, _ = r.render_features(cam, seed)
        mean = r.denoise_variance(sums, features, moments, spp)
        st = r.denoise_stats()
    assert np.isfinite(mean).all() and st.left_nonfinite == 0
    rtw.write_ppm(str(tmp_path / "want.ppm"), mean, 1)
    got = (tmp_path / "clean.ppm").read_bytes()
    assert got == (tmp_path / "want.ppm").read_bytes() and len(got) > width * height * 6
    assert f"{st.filled} pixels filled, 0 left non-finite" in run.stderr
    # the flag alone is refused
    run = subprocess.run([exe, "simple", "--config", str(cfg), "--denoise-variance"], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 2
