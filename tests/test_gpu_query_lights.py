"""The batched light pdf query (rtw_light_pdf_rays) against the independent
restatement's World.lights_pdf on the Lambertian bounces of oracle paths, in
f64 bit for bit through every light path; the f32 query against the f64 one;
and the plumbing of both queries (torch tensors and streams, refusals, the
render's caches left alone)."""
import ctypes as C

import numpy as np
import pytest

import query_cases as Q
import ray_tracing_weekend_amd as rtw
from indep import restate as R
from ray_tracing_weekend_amd import _capi
from test_gpu_query import query, same

pytestmark = pytest.mark.gpu

LINEAR, LIGHT_BVH, GRID, MIXED = 0, 1, 2, 3


def light_pdf(soa, rays, precision=rtw.RTW_F64, accel=rtw.RTW_ACCEL_AUTO, **tuning):
    with rtw.Renderer(device=0, precision=precision) as r:
        for k, v in tuning.items():
            r.set_tuning(k, v)
        r.set_accel(accel)
        r.set_scene(soa)
        pdf = r.light_pdf(rays)
        return pdf, r.get_query_stats()


def restate_pdf(soa, rays):
    w = R.World(soa)
    return np.array([w.lights_pdf(tuple(r[:3]), tuple(r[3:])) for r in rays])


def test_simple_linear_list():
    seg = Q.segments("simple")
    rays = Q.lambertian_bounces(seg)
    assert len(rays) >= 100 and len(seg.soa.lights) == 19
    want = restate_pdf(seg.soa, rays)
    assert (want > 0).sum() >= 5
    pdf, st = light_pdf(seg.soa, rays)
    assert (st.kernel, st.is_light_pdf, st.rays) == (LINEAR, 1, len(rays))
    assert st.light_tests == len(rays) * 19
    assert same(pdf, want)


def test_64_lights_grid_light_bvh_and_linear_list_give_identical_bits():
    soa, _ = Q.scene("lights64")
    # bounces of the oracle's paths, camera rays, and rays aimed at the lights (the
    # scene's first 64 spheres)
    rays = np.ascontiguousarray(np.concatenate([Q.lambertian_bounces(Q.segments("simple")),
                                                Q.camera_rays("simple63", 40, 24), Q.rays_at_lights(soa)]))
    want = restate_pdf(soa, rays)
    assert (want > 0).sum() >= 50 and (want == 0).sum() >= 50
    got = {}
    for what, tuning, path in (("grid", {}, GRID), ("light BVH", {"light_grid": 0}, LIGHT_BVH),
                               ("linear", {"light_bvh_min": 1 << 20}, LINEAR)):
        pdf, st = light_pdf(soa, rays, **tuning)
        assert st.kernel == path, (what, st.kernel)
        assert st.light_tests > 0
        got[what] = pdf
        assert same(pdf, want), (what, int((pdf != want).sum()))
    assert same(got["grid"], got["linear"]) and same(got["light BVH"], got["linear"])


def test_cornell_box_mixed_list():
    seg = Q.segments("cornell_box")
    rays = Q.lambertian_bounces(seg)
    assert len(rays) >= 100
    want = restate_pdf(seg.soa, rays)
    assert (want > 0).sum() >= 20
    pdf, st = light_pdf(seg.soa, rays)
    assert st.kernel == MIXED
    assert same(pdf, want)


def test_bvh_leaf_list_empty_list_and_origins_inside_a_light():
    soa, _ = Q.scene("simple")
    seg = Q.segments("simple")
    rays = Q.lambertian_bounces(seg)
    # RTW_LIGHTS_BVH_LEAF: (sum / n * n) / n over a list of 5
    # (on these rays the extra * n / n rounds back to the list's own value, so this pins
    # the flag's path, not a difference in value)
    leaf = Q.with_lights(soa, soa.lights[:5], flags=rtw.RTW_LIGHTS_BVH_LEAF)
    leaf_rays = np.ascontiguousarray(np.concatenate([rays, Q.rays_at_lights(leaf)]))
    want = restate_pdf(leaf, leaf_rays)
    assert (want > 0).sum() >= 10
    pdf, _ = light_pdf(leaf, leaf_rays)
    assert same(pdf, want)
    # an empty list: 0 / 0
    empty = Q.with_lights(soa, np.zeros((0, 4)))
    pdf, st = light_pdf(empty, rays[:70])
    assert np.isnan(pdf).all() and np.isnan(restate_pdf(empty, rays[:3])).all() and st.light_tests == 0
    # origins inside a light sphere: sqrt of a negative (sphere.rs:105)
    rng = np.random.default_rng(3)
    L = soa.lights
    inside = []
    for k in range(len(L)):
        for _ in range(4):
            off = rng.uniform(-1, 1, 3)
            off *= 0.6 * L[k, 3] / np.linalg.norm(off)
            inside.append(list(L[k, :3] + off) + list(rng.uniform(-1, 1, 3)))
    mixed = np.ascontiguousarray(np.concatenate([np.array(inside), rays[:60]]))
    want = restate_pdf(soa, mixed)
    assert np.isnan(want[:len(inside)]).all() and np.isfinite(want[len(inside):]).sum() >= 50
    pdf, _ = light_pdf(soa, mixed)
    assert np.array_equal(np.isnan(pdf), np.isnan(want)) and same(pdf, want)


# ------------------------------------------------------------------- g. f32
def test_f32_query_against_f64_on_camera_rays():
    """DESIGN 2b puts the f32 discriminant's cancellation band at ~1e-4 of a
    radius for this camera: about one ray in 10^4 may pick another object; the
    cap of 1 % leaves two orders of margin."""
    soa, _ = Q.scene("simple")
    rays = Q.camera_rays("simple", 120, 80)
    _, i64, _ = query(soa, rays)
    h32, i32, st = query(soa, rays.astype(np.float32), precision=rtw.RTW_F32)
    assert st.kernel == 5 and h32.dtype == np.float32
    assert (i64[:, 0] >= 0).sum() > 1000
    share = float((i32[:, 0] != i64[:, 0]).mean())
    print(f"f32 vs f64 object ids on {len(rays)} camera rays: {int((i32[:, 0] != i64[:, 0]).sum())} differ "
          f"({100 * share:.4f} %)")
    assert share <= 0.01
    # numpy input of another dtype is converted: the f64 rays through the f32 context
    h, i, _ = query(soa, rays, precision=rtw.RTW_F32)
    assert np.array_equal(i, i32) and same(h, h32)
    # the light pdf in f32 runs; its values are held row by row to the law of the f32 form in
    # tests/test_gpu_f32_records.py (test_light_pdf)
    b = Q.lambertian_bounces(Q.segments("simple"))
    p32, st = light_pdf(soa, b, precision=rtw.RTW_F32)
    assert p32.dtype == np.float32 and p32.shape == (len(b),) and st.kernel == LINEAR
    assert (p32 > 0).any()


# -------------------------------------------------------------- h. plumbing
def test_torch_tensors_on_a_side_stream_equal_the_numpy_path():
    import torch
    seg = Q.segments("simple")
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(seg.soa)
        want_h, want_i = r.hit_rays(seg.rays)
        bounces = Q.lambertian_bounces(seg)
        want_p = r.light_pdf(bounces)
        s = torch.cuda.Stream(device=0)
        with torch.cuda.stream(s):
            t = torch.from_numpy(seg.rays).to("cuda:0", non_blocking=True)
            hits, ids = r.hit_rays(t)
            pdf = r.light_pdf(torch.from_numpy(bounces).to("cuda:0", non_blocking=True))
            assert isinstance(hits, torch.Tensor) and hits.is_cuda and ids.dtype == torch.int32
            doubled = hits * 2          # torch work ordered after the query on the same stream
        s.synchronize()
        assert same(hits.cpu().numpy(), want_h) and np.array_equal(ids.cpu().numpy(), want_i)
        assert same(doubled.cpu().numpy(), 2 * want_h) and same(pdf.cpu().numpy(), want_p)
        with pytest.raises(rtw.RenderError):                 # a tensor of the other precision
            r.hit_rays(t.float())
        with pytest.raises(rtw.RenderError):
            r.light_pdf(torch.from_numpy(seg.rays))          # a CPU tensor


def test_refusals():
    import torch
    lib = rtw._lib
    soa, _ = Q.scene("simple")
    rays = torch.zeros((8, 6), dtype=torch.float64, device="cuda:0")
    rays[:, 5] = -1.0
    hits = torch.zeros((8, 9), dtype=torch.float64, device="cuda:0")
    ids = torch.zeros((8, 4), dtype=torch.int32, device="cuda:0")
    pdf = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        hit = lambda n, t_min, hb, ib: lib.rtw_hit_rays_device(r.ctx, vp(rays), n, t_min, vp(hits), hb, vp(ids), ib, None)  # noqa: E731
        assert hit(8, 0.0, 8 * 72, 8 * 16) == _capi.RTW_E_NO_SCENE
        assert lib.rtw_light_pdf_rays_device(r.ctx, vp(rays), 8, vp(pdf), 64, None) == _capi.RTW_E_NO_SCENE
        st = _capi.rtw_query_stats()
        assert lib.rtw_get_query_stats(r.ctx, C.byref(st)) == _capi.RTW_E_INVALID      # no query yet
        r.set_scene(soa)
        assert hit(8, 0.0, 8 * 72, 8 * 16) == _capi.RTW_OK
        assert hit(8, 0.0, 8 * 72 - 1, 8 * 16) == _capi.RTW_E_INVALID                  # short buffers
        assert hit(8, 0.0, 8 * 72, 8 * 16 - 1) == _capi.RTW_E_INVALID
        assert lib.rtw_light_pdf_rays_device(r.ctx, vp(rays), 8, vp(pdf), 63, None) == _capi.RTW_E_INVALID
        assert lib.rtw_light_pdf_rays_device(r.ctx, vp(rays), 8, vp(pdf), 64, None) == _capi.RTW_OK
        for bad in (-1.0, float("nan"), float("inf"), -0.5e-300):
            assert hit(8, bad, 8 * 72, 8 * 16) == _capi.RTW_E_INVALID, bad
        assert lib.rtw_hit_rays_device(r.ctx, None, 8, 0.0, vp(hits), 8 * 72, vp(ids), 8 * 16, None) == _capi.RTW_E_INVALID
        assert lib.rtw_hit_rays_device(r.ctx, vp(rays), 8, 0.0, None, 8 * 72, vp(ids), 8 * 16, None) == _capi.RTW_E_INVALID
        assert lib.rtw_hit_rays_device(r.ctx, None, 0, 0.0, None, 0, None, 0, None) == _capi.RTW_OK   # n = 0
        assert lib.rtw_light_pdf_rays(r.ctx, None, 0, None) == _capi.RTW_OK
        torch.cuda.synchronize()
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        r.set_scene(soa)
        assert lib.rtw_hit_rays_device(r.ctx, vp(rays), 8, 0.0, vp(hits), 8 * 72, vp(ids), 8 * 16, None) \
            == _capi.RTW_E_UNSUPPORTED
        with pytest.raises(rtw.RenderError) as e:
            r.light_pdf(np.zeros((4, 6)))
        assert e.value.code == _capi.RTW_E_UNSUPPORTED


def test_a_query_between_two_renders_leaves_them_identical():
    soa, b = Q.scene("simple")
    cam = b.copy().with_image_width(48).with_image_height(32).with_samples_per_pixel(40).with_max_depth(12).build()
    seg = Q.segments("simple")
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        first = r.render(cam, 5)
        stats = (r.stats.segments, r.stats.kernel)
        kernel = r.last_kernel()
        _, ids = r.hit_rays(seg.rays)
        r.light_pdf(Q.lambertian_bounces(seg))
        assert np.array_equal(ids[:, 0], seg.ids)
        assert r.last_kernel() == kernel and r.get_stats().segments == stats[0]
        second = r.render(cam, 5)
        assert (r.stats.segments, r.stats.kernel) == stats
    assert same(first, second)


def test_hittable_list_conveniences():
    world, lights, _ = rtw.scenes.simple(0x5EED0001)
    seg = Q.segments("simple")
    hits, ids = world.hit(seg.rays[:300], lights=lights)
    assert np.array_equal(ids[:, 0], seg.ids[:300]) and same(hits[:, 0], seg.hits[:300, 0])
    b = Q.lambertian_bounces(seg)[:100]
    assert same(lights.pdf_value(b, world=world), restate_pdf(seg.soa, b))
