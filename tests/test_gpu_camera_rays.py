"""Camera rays (rtw_camera_rays) on the GPU in f64, bit for bit against the
independent restatement (tests/path_cases.py get_ray: the head of
restate.trace_sample): the rays and the xoshiro256++ words after get_ray's
draws, with and without defocus, for consecutive pixels, a shuffled list with
repeats and the batch tails; the numpy and torch entries; the refusals; f32."""
import numpy as np
import pytest

import feature_cases as F
import path_cases as P
import ray_tracing_weekend_amd as rtw
from oracle import oracle as O
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu


def same(a, b):
    """bit for bit (the sign of zero included; the rays here hold no NaN)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and not np.isnan(a).any() and \
        bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


W, H, SEED = 40, 24, 7
BLOCK = 256                                    # kQueryBlock
CAMERA_RAYS = 4                                # rtw_query_stats.is_light_pdf


def cams(name):
    cam, ocam = F.cameras(name, W, H)
    return cam, O.camera_dict(ocam)


@pytest.fixture(scope="module")
def r64():
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        yield r                                # (no scene is staged: camera rays need none)


@pytest.mark.parametrize("name", ["simple", "simple_defocus"])
@pytest.mark.parametrize("sample", [0, 3])
def test_rays_and_streams_are_the_restatements(r64, name, sample):
    cam, camd = cams(name)
    assert (camd["defocus_angle"] > 0) == (name == "simple_defocus")
    # every pixel in order (first_pixel 0, n = W * H)
    want_rays, want_rng = P.camera_rays(camd, SEED, range(W * H), sample)
    rays, rng = r64.camera_rays(cam, SEED, sample)
    assert rays.shape == (W * H, 6) and rng.shape == (W * H, 4) and rng.dtype == np.uint64
    assert same(rays, want_rays) and np.array_equal(rng, want_rng)
    st = r64.get_query_stats()
    assert (st.is_light_pdf, st.rays) == (CAMERA_RAYS, W * H)
    # consecutive pixels from the middle of the image: the batch tails
    for n in (0, 1, 63, 64, 65, BLOCK + 1):
        rays, rng = r64.camera_rays(cam, SEED, sample, first_pixel=300, n=n)
        assert rays.shape == (n, 6) and rng.shape == (n, 4)
        assert same(rays, want_rays[300:300 + n]) and np.array_equal(rng, want_rng[300:300 + n])
    # a shuffled list with repeats
    pix = np.random.default_rng(5).integers(0, W * H, BLOCK + 1)
    pix[7] = pix[3] = W * H - 1
    rays, rng = r64.camera_rays(cam, SEED, sample, pixels=pix)
    assert same(rays, want_rays[pix]) and np.array_equal(rng, want_rng[pix])
    for n in (0, 1, 65):
        rays, rng = r64.camera_rays(cam, SEED, sample, pixels=pix[:n])
        assert same(rays, want_rays[pix[:n]]) and np.array_equal(rng, want_rng[pix[:n]])


def test_defocus_draws_more_words(r64):
    """Without defocus the state is two draws from the stream's start; with it, further."""
    cam, camd = cams("simple")
    _, rng = r64.camera_rays(cam, SEED, 0, first_pixel=0, n=4)
    for k in range(4):
        g = P.R.Rng(SEED, k, 0)
        g.next_u64(), g.next_u64()
        assert tuple(int(x) for x in rng[k]) == tuple(g.s)
    dcam, _ = cams("simple_defocus")
    _, drng = r64.camera_rays(dcam, SEED, 0, first_pixel=0, n=4)
    assert not (drng == rng).all(1).any()


def test_numpy_and_torch_entries_are_identical(r64):
    import torch
    cam, _ = cams("simple_defocus")
    rays, rng = r64.camera_rays(cam, SEED, 3)
    t_rays, t_rng = r64.camera_rays(cam, SEED, 3, as_torch=True)
    assert t_rays.is_cuda and t_rng.dtype == torch.int64
    assert same(t_rays.cpu().numpy(), rays) and np.array_equal(t_rng.cpu().numpy().view(np.uint64), rng)
    pix = np.random.default_rng(9).integers(0, W * H, 321).astype(np.int32)
    t_rays, t_rng = r64.camera_rays(cam, SEED, 3, pixels=torch.as_tensor(pix, device="cuda:0"))
    assert same(t_rays.cpu().numpy(), rays[pix]) and np.array_equal(t_rng.cpu().numpy().view(np.uint64), rng[pix])
    # the device form clamps an index beyond the image to the last pixel (the caller's error)
    bad = torch.as_tensor(np.array([5, W * H, 2 ** 31 - 1], np.int32), device="cuda:0")
    t_rays, _ = r64.camera_rays(cam, SEED, 3, pixels=bad)
    assert same(t_rays.cpu().numpy(), rays[[5, W * H - 1, W * H - 1]])


def test_refusals(r64):
    cam, _ = cams("simple")
    for kw in (dict(pixels=[0, W * H]), dict(first_pixel=W * H, n=1), dict(first_pixel=W * H - 1, n=2)):
        with pytest.raises(rtw.RenderError) as e:
            r64.camera_rays(cam, SEED, 0, **kw)
        assert e.value.code == _capi.RTW_E_INVALID
    for bad in ([0, -1], [0, 1 << 32]):       # not a uint32: refused before the upload, on both entries
        for as_torch in (False, True):
            with pytest.raises(rtw.RenderError) as e:
                r64.camera_rays(cam, SEED, 0, pixels=bad, as_torch=as_torch)
            assert e.value.code == _capi.RTW_E_INVALID
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        with pytest.raises(rtw.RenderError) as e:
            r.camera_rays(cam, SEED, 0)
        assert e.value.code == _capi.RTW_E_UNSUPPORTED


def test_f32_rays_follow_the_f64_ones_and_draw_the_same_words():
    """(The absolute bound below is the coarse one; tests/test_gpu_f32_records.py
    test_camera_rays holds the f32 rays, with and without defocus, to the law of the f32
    form within 4 x the rounding of a correctly rounded f32 evaluation.)"""
    cam, camd = cams("simple")
    want_rays, want_rng = P.camera_rays(camd, SEED, range(W * H), 1)
    with rtw.Renderer(device=0, precision=rtw.RTW_F32) as r:
        rays, rng = r.camera_rays(cam, SEED, 1)
        again, _ = r.camera_rays(cam, SEED, 1)
    assert rays.dtype == np.float32 and same(rays, again)
    assert np.array_equal(rng, want_rng)       # no defocus: two words in both precisions
    assert np.abs(rays - want_rays).max() < 1e-4
