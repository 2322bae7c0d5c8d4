"""The denoiser (rtw_denoise) on the GPU against the numpy restatement of
tests/denoise_cases.py: made-up frames of every kind of pixel at sizes around
the tile, the staged against the direct form, the device entry on a side
stream, the pipeline render -> feature pass -> denoise in both precisions and
with adaptive counts, isolation from renders, queries and feature passes, a
virtual-rank context, the refusals and the stats.  Every comparison is bit for
bit up to the sign of zero with equal NaN masks (feature_cases.same)."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import denoise_cases as D
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
    """Every combination of normal_power_log2 {0, 5}, sigma_colour {0, 1},
    demodulate {0, 1} and fill_nonfinite {0, 1}, the iterations 1, 3, 5, 7 dealt
    over them so that each count meets both values of every other parameter."""
    out = []
    for c, (m, sc, dm, fill) in enumerate(itertools.product((0, 5), (0.0, 1.0), (0, 1), (0, 1))):
        out.append(dict(iterations=(1, 3, 5, 7)[(c + c // 4) % 4], normal_power_log2=m, sigma_colour=sc,
                        sigma_depth=0.125, demodulate=dm, fill_nonfinite=fill))
    return out


@functools.lru_cache(maxsize=None)
def expected(width, height, per_pixel, key):
    sums, features, counts = D.synthetic(width, height)
    return D.restate(sums, features, counts if per_pixel else SPP, **dict(key))


def key_of(params):
    return tuple(sorted(params.items()))


# ------------------------------------------------------- 1. synthetic parity
def test_param_sets_cover_what_they_claim():
    sets = param_sets()
    assert len(sets) == 16
    for it in (1, 3, 5, 7):
        mine = [p for p in sets if p["iterations"] == it]
        for k in ("normal_power_log2", "sigma_colour", "demodulate", "fill_nonfinite"):
            assert len({p[k] for p in mine}) == 2, (it, k)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("per_pixel", (False, True), ids=("spp", "counts"))
def test_host_entry_is_the_restatement(size, per_pixel):
    width, height = size
    sums, features, counts = D.synthetic(width, height)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        for params in param_sets():
            want, filled, left = expected(width, height, per_pixel, key_of(params))
            got = r.denoise(sums, features, counts if per_pixel else SPP, **params)
            assert got.shape == (height, width, 3) and got.dtype == np.float64
            assert same(got, want), (params, where_differs(got, want))
            st = r.denoise_stats()
            assert (st.filled, st.left_nonfinite, st.iterations) == (filled, left, params["iterations"]), params
            assert st.kernel_ms > 0


def test_the_synthetic_cases_are_not_vacuous():
    """The filter changes the image, fills pixels when asked to and leaves some
    non-finite; the parameters matter."""
    sums, features, counts = D.synthetic(70, 45)
    outs = []
    for params in param_sets():
        want, filled, left = expected(70, 45, True, key_of(params))
        assert (filled > 0) == bool(params["fill_nonfinite"]) and left > 0
        outs.append(want)
    assert sum(same(a, b) for a, b in itertools.combinations(outs, 2)) == 0
    with np.errstate(all="ignore"):
        plain = np.where(counts[..., None] > 0, sums / counts[..., None].astype(np.float64), 0.0)
    assert not same(outs[-1], plain)


# ------------------------------------------------------ 2. LDS against direct
def test_staged_and_direct_forms_are_identical():
    sums, features, counts = D.synthetic(70, 45)
    for iterations in (1, 2, 3, 4):
        params = dict(D.START, iterations=iterations)
        got = {}
        for lds in (0, 2):
            with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
                r.set_tuning("denoise_lds", lds)
                got[lds] = r.denoise(sums, features, counts, **params)
                st = r.denoise_stats()
            # tile + halo fit the LDS up to step 8: every one of these iterations is staged
            assert (st.iterations, st.lds_iterations) == (iterations, iterations if lds else 0)
        want, _, _ = D.restate(sums, features, counts, **params)
        assert same(got[0], got[2]), where_differs(got[0], got[2])
        assert same(got[0], want), where_differs(got[0], want)
    # steps beyond 8 do not fit and fall back
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_tuning("denoise_lds", 2)
        got7 = r.denoise(sums, features, counts, **dict(D.START, iterations=7))
        assert r.denoise_stats().lds_iterations == 4
    want7 = D.restate(sums, features, counts, **dict(D.START, iterations=7))[0]
    assert same(got7, want7)
    # the default plan, whatever it stages, is the same filter
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        assert same(r.denoise(sums, features, counts, **dict(D.START, iterations=7)), want7)
        assert r.denoise_stats().lds_iterations <= 4


# ------------------------------------------------------------ 3. device entry
def test_device_entry_on_a_side_stream_is_the_host_entry():
    import torch
    width, height = 37, 19
    sums, features, counts = D.synthetic(width, height)
    with np.errstate(all="ignore"):
        sums32 = sums.astype(np.float32)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            d_feat = torch.from_numpy(np.array(features)).to("cuda:0")
            d_counts = torch.from_numpy(counts.astype(np.int32)).to("cuda:0")
            d64 = r.denoise(torch.from_numpy(np.array(sums)).to("cuda:0"), d_feat, d_counts, **D.START)
            d32 = r.denoise(torch.from_numpy(sums32).to("cuda:0"), d_feat, SPP, **D.START)
            assert d64.is_cuda and d64.dtype == torch.float64 and tuple(d64.shape) == (height, width, 3)
        side.synchronize()
        h64 = r.denoise(sums, features, counts, **D.START)
        h32 = r.denoise(sums32.astype(np.float64), features, SPP, **D.START)
    assert same(d64.cpu().numpy(), h64) and same(d32.cpu().numpy(), h32)
    assert same(h64, D.restate(sums, features, counts, **D.START)[0])
    assert same(h32, D.restate(sums32, features, SPP, **D.START)[0])
    assert not same(h32, h64)


def test_device_entry_refuses_bad_arrays_and_writes_nothing():
    import torch
    width, height = 10, 6
    px = width * height
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        d_sums = torch.ones(px * 3 + 2, dtype=torch.float64, device="cuda:0")
        d_feat = torch.ones(px * 8 + 2, dtype=torch.float64, device="cuda:0")
        d_out = torch.full((px * 3 + 2,), -77.0, dtype=torch.float64, device="cuda:0")

        def call(sums=d_sums.data_ptr(), sums_bytes=px * 24, feat=d_feat.data_ptr(), feat_bytes=px * 64,
                 out=d_out.data_ptr(), out_bytes=px * 24, prec=_capi.RTW_F64):
            return rtw._lib.rtw_denoise_device(r.ctx, C.c_void_p(sums), prec, sums_bytes, C.c_void_p(feat), feat_bytes,
                                               None, 0, 4, width, height, None, C.c_void_p(out), out_bytes, None)
        assert call(sums_bytes=px * 24 - 8) == INV and call(feat_bytes=px * 64 - 8) == INV
        assert call(out_bytes=px * 24 - 8) == INV
        assert call(sums_bytes=px * 12) == INV and call(sums_bytes=px * 12, prec=7) == INV
        assert call(feat=d_feat.data_ptr() + 8) == INV and call(out=d_out.data_ptr() + 8) == INV
        assert call(sums=d_sums.data_ptr() + 8) == INV
        assert call(out=d_sums.data_ptr()) == INV                                  # out is an input
        assert call(out=d_feat.data_ptr() + px * 64 - 16) == INV                   # ... or overlaps one's end
        torch.cuda.synchronize()
        assert bool((d_out == -77.0).all()) and bool((d_sums == 1.0).all()) and bool((d_feat == 1.0).all())
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


def test_render_features_denoise_is_the_restatement_of_the_gpus_own_buffers():
    soa, cam = _simple_camera()
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        sums = r.render(cam, F.SEED)
        features, _ = r.render_features(cam, F.SEED)
        got = r.denoise(sums, features, SPP, **D.START)
        a_sums, a_counts = r.render_adaptive(cam, F.SEED, 4, SPP, 4, 0.02)
        a_features, _ = r.render_features(cam, F.SEED, 0, SPP, counts=a_counts)
        a_got = r.denoise(a_sums, a_features, a_counts, **D.START)
    want, _, _ = D.restate(sums, features, SPP, **D.START)
    assert same(got, want), where_differs(got, want)
    assert not same(got, sums / SPP)
    assert len(np.unique(a_counts)) >= 2            # the adaptive counts differ between tiles
    a_want, _, _ = D.restate(a_sums, a_features, a_counts, **D.START)
    assert same(a_got, a_want), where_differs(a_got, a_want)


def test_render_denoised_is_the_three_calls():
    world, lights, b = rtw.scenes.simple(0x5EED0001)
    cam = b.with_image_width(40).with_image_height(24).with_samples_per_pixel(SPP).with_max_depth(50).build()
    params = dict(D.START, iterations=3)
    got = cam.render_denoised(world, lights, seed=F.SEED, **params)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(rtw.flatten(world, lights))
        sums = r.render(cam, F.SEED)
        features, _ = r.render_features(cam, F.SEED)
        want = r.denoise(sums, features, SPP, **params)
    assert got.shape == (24, 40, 3) and same(got, want)
    assert same(want, D.restate(sums, features, SPP, **params)[0])


def test_an_f32_contexts_device_image_through_the_device_entry():
    import torch
    soa, cam = _simple_camera()
    with rtw.Renderer(device=0, precision=rtw.RTW_F32) as r:
        r.set_scene(soa)
        img = torch.zeros((24, 40, 3), dtype=torch.float32, device="cuda:0")
        r.render_image_device(cam, F.SEED, img.data_ptr(), img.numel() * 4)
        features = torch.zeros((24, 40, 8), dtype=torch.float64, device="cuda:0")
        r.render_features(cam, F.SEED, features=features, want_ids=False)
        got = r.denoise(img, features, SPP, **D.START)
        torch.cuda.synchronize()
    sums32, feat = img.cpu().numpy(), features.cpu().numpy()
    assert sums32.dtype == np.float32 and np.isfinite(sums32).any() and feat[..., 7].sum() > 0
    want, _, _ = D.restate(sums32, feat, SPP, **D.START)
    assert same(got.cpu().numpy(), want), where_differs(got.cpu().numpy(), want)


# --------------------------------------------------------------- 5. isolation
def test_a_denoise_leaves_renders_queries_and_feature_passes_alone():
    soa, cam = _simple_camera(4)
    rays = np.random.default_rng(5).normal(size=(64, 6))
    rays[:, :3] = (13.0, 2.0, 3.0)
    sums_s, features_s, counts_s = D.synthetic(37, 19)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        img0, (h0, i0), (f0, _) = r.render(cam, F.SEED), r.hit_rays(rays), r.render_features(cam, F.SEED)
        first = r.denoise(sums_s, features_s, counts_s, **D.START)
        img1, (h1, i1), (f1, _) = r.render(cam, F.SEED), r.hit_rays(rays), r.render_features(cam, F.SEED)
        # a second denoise of another (smaller, then larger) size reuses the state
        small = r.denoise(*D.synthetic(5, 3)[:2], D.synthetic(5, 3)[2], **D.START)
        large = r.denoise(*D.synthetic(70, 45)[:2], D.synthetic(70, 45)[2], **D.START)
        again = r.denoise(sums_s, features_s, counts_s, **D.START)
    assert same(img0, img1) and same(h0, h1) and np.array_equal(i0, i1) and same(f0, f1)
    assert same(first, expected(37, 19, True, key_of(D.START))[0]) and same(again, first)
    assert same(small, expected(5, 3, True, key_of(D.START))[0])
    assert same(large, expected(70, 45, True, key_of(D.START))[0])


# -------------------------------------------------------------- 6. multi-rank
def test_a_virtual_rank_context_denoises_its_gathered_image():
    soa, cam = _simple_camera()
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        sums = r.render(cam, F.SEED)
        features, _ = r.render_features(cam, F.SEED)
        want = r.denoise(sums, features, SPP, **D.START)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        r.set_scene(soa)
        gathered = r.render(cam, F.SEED)
        got = r.denoise(gathered, features, SPP, **D.START)
        assert r.denoise_stats().iterations == D.START["iterations"]
    assert same(gathered, sums) and same(got, want)


# --------------------------------------------------------------- 7. refusals
def test_refusals_on_a_context():
    lib = rtw._lib
    s, f, o = np.ones((4, 4, 3)), np.ones((4, 4, 8)), np.full((4, 4, 3), -77.0)
    cnt = np.ones((4, 4), np.uint32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    nan, inf = float("nan"), float("inf")
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        st = _capi.rtw_denoise_stats()
        assert lib.rtw_get_denoise_stats(r.ctx, C.byref(st)) == INV           # before the first denoise

        def call(sums=s, feat=f, counts=None, spp=4, w=4, h=4, out=o, **fields):
            p = rtw.DenoiseParams(**fields).raw
            return lib.rtw_denoise(r.ctx, vp(sums), vp(feat), vp(counts), spp, w, h, C.byref(p), vp(out))
        assert call(sums=None) == INV and call(feat=None) == INV and call(out=None) == INV
        assert call(spp=0) == INV and call(spp=0, counts=cnt) == 0
        assert call(w=1 << 16, h=1) == INV and call(w=1, h=1 << 16) == INV
        for bad in (dict(iterations=0), dict(iterations=17), dict(normal_power_log2=11), dict(sigma_colour=-1.0),
                    dict(sigma_colour=nan), dict(sigma_colour=inf), dict(sigma_depth=0.0), dict(sigma_depth=-1.0),
                    dict(sigma_depth=nan), dict(sigma_depth=inf), dict(demodulate=2), dict(fill_nonfinite=2)):
            o[:] = -77.0
            assert call(**bad) == INV, bad
            assert (o == -77.0).all() and lib.rtw_last_error(r.ctx)
        assert call(iterations=16, normal_power_log2=10, sigma_colour=0.0) == 0
        assert (o != -77.0).all()
        # NULL parameters are the defaults
        assert lib.rtw_denoise(r.ctx, vp(s), vp(f), None, 4, 4, 4, None, vp(o)) == 0
        assert lib.rtw_get_denoise_stats(r.ctx, C.byref(st)) == 0 and st.iterations == 5
        assert lib.rtw_get_denoise_stats(r.ctx, None) == INV


# ------------------------------------------------------------------ the CLI
def test_cli_writes_the_denoised_image(tmp_path):
    """rtw simple --denoise PATH (rtw::denoise of the C++ mirror, the default
    parameters): the PPM is the Python mirror's means through the same writer,
    and no pixel of it is a black NaN pixel."""
    import os
    import subprocess
    width, height, spp, seed = 40, 24, 16, 0x5EED0001
    cfg = tmp_path / "Config.toml"
    cfg.write_text(f"[image]\nimage_width = {width}\nimage_height = {height}\nsamples_per_pixel = {spp}\n"
                   "max_depth = 50\n")
    exe = os.path.join(os.path.dirname(_capi.LIB_PATH), "rtw")
    run = subprocess.run([exe, "simple", "--seed", str(seed), "--config", str(cfg), "--out", str(tmp_path / "image.ppm"),
                          "--denoise", str(tmp_path / "clean.ppm")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    soa, b = rtw.scenes.simple_soa(seed)
    cam = b.with_vfov(40.0).with_aspect_ratio(width / height).with_max_depth(50).with_image_width(width) \
           .with_image_height(height).with_samples_per_pixel(spp).build()
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        sums = r.render(cam, seed)
        features, _ = r.render_features(cam, seed)
        mean = r.denoise(sums, features, spp)
        st = r.denoise_stats()
    assert np.isfinite(mean).all() and st.left_nonfinite == 0
    rtw.write_ppm(str(tmp_path / "want.ppm"), mean, 1)
    rtw.write_ppm(str(tmp_path / "noisy.ppm"), sums, spp)
    got = (tmp_path / "clean.ppm").read_bytes()
    assert got == (tmp_path / "want.ppm").read_bytes() and len(got) > width * height * 6
    assert (tmp_path / "image.ppm").read_bytes() == (tmp_path / "noisy.ppm").read_bytes()
    assert f"{st.filled} pixels filled, 0 left non-finite" in run.stderr
