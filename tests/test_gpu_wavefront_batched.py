"""rtw_render_wavefront -- the wavefront loop with its rounds on the device, a
batch of samples at a time -- against Camera::render and the host loop it
replaces (Renderer.render_wavefront): in f64 the three images are equal bit for
bit (NaN masks and the sign of zero included) on every named scene with
lights, for the planner's batch, one sample a batch and a batch that does not
divide the samples; the driver's stats are the render's segments and
Lambertian scatters; f32 equals the host loop's f32; shallow depths end with
survivors; windows compose across batch boundaries; the Python hook loop over
path_advance equals the driver; the torch form returns the same bits; scenes
without lights are refused; a render afterwards is unchanged.
The setup is tests/test_gpu_wavefront.py's: 40 x 24, 4 spp, seed 7, chunk 1."""
import functools

import numpy as np
import pytest
import torch

import path_cases as P
import query_cases as Q
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 40, 24, 4, 7
LIT = [n for n in rtw.scenes.NAMES if n not in P.NO_LIGHTS]


def bits(a):
    """the values' bit patterns, every NaN as the one pattern of all ones (payloads aside)"""
    a = np.ascontiguousarray(a, np.float64)
    u = a.view(np.uint64).copy()
    u[np.isnan(a)] = ~np.uint64(0)
    return u


def same(a, b):
    """bit for bit, the sign of zero included; NaN masks equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def camera(name, depth=50, spp=SPP):
    _, b = Q.scene(name)
    return b.copy().with_image_width(W).with_image_height(H).with_samples_per_pixel(spp).with_max_depth(depth).build()


@functools.lru_cache(maxsize=None)
def references(name, precision=rtw.RTW_F64, depth=50):
    """(render's sums, the host loop's sums, render's segments, render's lambertian): computed once, shared"""
    soa, _ = Q.scene(name)
    cam = camera(name, depth)
    with rtw.Renderer(device=0, precision=precision) as r:
        r.set_chunk(1)
        r.set_scene(soa)
        ref = r.render(cam, SEED)
        st = (r.stats.segments, r.stats.lambertian)
        loop = r.render_wavefront(cam, SEED)
    ref.flags.writeable = loop.flags.writeable = False
    return ref, loop, st[0], st[1]


@pytest.mark.parametrize("name", LIT)
def test_batched_is_render_and_the_host_loop_bit_for_bit(name):
    ref, loop, segments, lambertian = references(name)
    soa, _ = Q.scene(name)
    cam = camera(name)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_chunk(1)
        r.set_scene(soa)
        for batch in (0, 1, 3):
            got = r.render_wavefront_batched(cam, SEED, batch=batch)
            assert got.shape == (H, W, 3) and got.dtype == np.float64
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            assert np.array_equal(bits(got), bits(ref)), (batch, int((bits(got) != bits(ref)).sum()))
            assert same(got, loop)
            st = r.get_query_stats()
            assert st.is_light_pdf == 7 and st.rays == segments and st.hits == lambertian, batch
            assert st.kernel_ms > 0
        assert same(r.render(cam, SEED), ref)             # a render after the driver is unchanged


@pytest.mark.parametrize("name", ["simple", "cornell_box"])
def test_f32_is_the_host_loops_f32(name):
    _, loop, _, _ = references(name, rtw.RTW_F32)
    soa, _ = Q.scene(name)
    with rtw.Renderer(device=0, precision=rtw.RTW_F32) as r:
        r.set_chunk(1)
        r.set_scene(soa)
        for batch in (0, 3):
            assert same(r.render_wavefront_batched(camera(name), SEED, batch=batch), loop), batch


class Rounds:
    """an on_bounce hook that counts: the rays of every round, the SCATTER events, the
    paths that go on out of each depth"""

    def __init__(self):
        self.rays, self.scatter, self.on = 0, 0, {}

    def __call__(self, depth, paths, rays, hits, ids, event, weight, emitted):
        assert len(paths) == len(rays) == len(hits) == len(ids) == len(event) == len(weight) == len(emitted)
        assert paths.dtype == torch.int64 and rays.is_cuda
        assert int(paths.max()) < SPP * W * H and len(torch.unique(paths)) == len(paths)
        self.rays += len(rays)
        self.scatter += int((event == _capi.RTW_EVENT_SCATTER).sum())
        self.on[depth] = self.on.get(depth, 0) + int((event >= _capi.RTW_EVENT_REFLECT).sum())


@pytest.mark.parametrize("depth", [1, 3])
def test_shallow_depths_end_with_survivors(depth):
    ref, loop, segments, lambertian = references("simple", depth=depth)
    soa, _ = Q.scene("simple")
    cam = camera("simple", depth)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_chunk(1)
        r.set_scene(soa)
        for batch in (0, 3):
            assert same(r.render_wavefront_batched(cam, SEED, batch=batch), ref), batch
            st = r.get_query_stats()
            assert (st.is_light_pdf, st.rays, st.hits) == (7, segments, lambertian)
        hook = Rounds()
        assert same(r.render_wavefront_batched(cam, SEED, batch=3, on_bounce=hook), ref)
        assert hook.on[depth - 1] > 100                    # the `last` round had paths to end with 0 + res'
        assert hook.rays == segments and hook.scatter == lambertian


def test_max_depth_0_adds_zero_per_sample():
    soa, _ = Q.scene("simple")
    cam = camera("simple", 1)
    cam.raw.max_depth = 0
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        loop = r.render_wavefront(cam, SEED)
        hook = Rounds()
        for kw in ({}, {"batch": 3}, {"on_bounce": hook}):
            got = r.render_wavefront_batched(cam, SEED, **kw)
            assert same(got, loop) and same(got, np.zeros((H, W, 3)))
        assert not hook.on and hook.rays == 0
        onto = r.render_wavefront_batched(cam, SEED, sums=np.full((H, W, 3), -0.0))
        assert same(onto, np.zeros((H, W, 3)))             # -0 + 0 = +0: the 0 was added
        r.render_wavefront_batched(cam, SEED, batch=1)
        st = r.get_query_stats()
        assert (st.is_light_pdf, st.rays, st.hits) == (7, 0, 0)


def test_windows_compose_across_batch_boundaries():
    ref, _, _, _ = references("cornell_box")
    soa, _ = Q.scene("cornell_box")
    cam = camera("cornell_box")
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_chunk(1)
        r.set_scene(soa)
        a = r.render_wavefront_batched(cam, SEED, 0, 2, batch=0)          # one batch of 2
        c = r.render_wavefront_batched(cam, SEED, 2, 2, batch=1, sums=a)  # then 1 + 1 onto it
        assert same(c, ref) and not same(a, ref)
        whole = r.render_wavefront_batched(cam, SEED, 0, 4, batch=3)      # 3 + 1: other boundaries
        assert same(whole, c)
        one = r.render_wavefront_batched(cam, SEED, 1, 3, batch=2, sums=r.render_wavefront_batched(cam, SEED, 0, 1))
        assert same(one, ref)
        st = r.get_query_stats()
        assert st.is_light_pdf == 7 and 0 < st.rays < references("cornell_box")[2]   # the last call's three samples
        nothing = r.render_wavefront_batched(cam, SEED, 2, 0, sums=a)     # no samples: the sums as they were
        assert same(nothing, a)


@pytest.mark.parametrize("name,precision", [("simple", rtw.RTW_F64), ("cornell_box", rtw.RTW_F64),
                                            ("simple", rtw.RTW_F32)])
def test_the_hook_loop_is_the_driver(name, precision):
    ref, loop, segments, lambertian = references(name, precision)
    soa, _ = Q.scene(name)
    cam = camera(name)
    with rtw.Renderer(device=0, precision=precision) as r:
        r.set_chunk(1)
        r.set_scene(soa)
        driver = r.render_wavefront_batched(cam, SEED, batch=3)
        hook = Rounds()
        got = r.render_wavefront_batched(cam, SEED, batch=3, on_bounce=hook)
        assert same(got, driver) and same(got, loop)
        if precision == rtw.RTW_F64:                       # (the f32 render is the hit64 kernel's: other paths)
            assert hook.rays == segments and hook.scatter == lambertian
        st = r.get_query_stats()                           # the hook loop's last query is an advance
        assert st.is_light_pdf == 6
        # the torch form: device sums in and out, the same bits
        t = r.render_wavefront_batched(cam, SEED, as_torch=True)
        assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (H, W, 3)
        assert same(t.cpu().numpy(), driver)
        half = r.render_wavefront_batched(cam, SEED, 0, 2, as_torch=True)
        before = half.clone()
        full = r.render_wavefront_batched(cam, SEED, 2, 2, sums=half, as_torch=True)
        assert same(full.cpu().numpy(), driver) and same(half.cpu().numpy(), before.cpu().numpy())   # sums is not written to
        th = r.render_wavefront_batched(cam, SEED, batch=0, on_bounce=Rounds(), as_torch=True)
        assert th.is_cuda and same(th.cpu().numpy(), driver)


@pytest.mark.parametrize("name", sorted(P.NO_LIGHTS))
def test_scenes_without_lights_are_refused(name):
    soa, _ = Q.scene(name)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        sums = np.full((H, W, 3), 5.0)
        for kw in ({}, {"as_torch": True}):
            with pytest.raises(rtw.RenderError) as e:
                r.render_wavefront_batched(camera(name), SEED, sums=sums, **kw)
            assert e.value.code == _capi.RTW_E_NO_LIGHTS
        assert (sums == 5.0).all()


def test_refusals_and_the_camera_form():
    soa, _ = Q.scene("simple")
    cam = camera("simple")
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        with pytest.raises(rtw.RenderError) as e:          # before rtw_set_scene
            r.render_wavefront_batched(cam, SEED)
        assert e.value.code == _capi.RTW_E_NO_SCENE
        r.set_scene(soa)
        small = torch.zeros((H * W * 3 - 1,), dtype=torch.float64, device="cuda")
        rc = rtw._lib.rtw_render_wavefront_device(r.ctx, cam.raw, SEED, 0, 1, 0, small.data_ptr(), small.numel() * 8, None)
        assert rc == _capi.RTW_E_INVALID and not small.any()
    with rtw.Renderer(precision=rtw.RTW_F64, virtual_ranks=2) as v:
        v.set_scene(soa)
        with pytest.raises(rtw.RenderError) as e:
            v.render_wavefront_batched(cam, SEED)
        assert e.value.code == _capi.RTW_E_UNSUPPORTED
    world, lights, _ = rtw.scenes.simple(0x5EED0001)
    got = cam.render_wavefront_batched(world, lights, seed=SEED, batch=3)
    assert same(got, cam.render_wavefront(world, lights, seed=SEED)) and np.isfinite(got).any()
