"""Light sampling (rtw_light_sample) on the GPU in f64, bit for bit against the
independent restatement (tests/nee_cases.py light_samples: World.lights_random
on the stream Rng(seed, first_stream + k, sample), World.lights_pdf of the
direction drawn): directions, list indices and the fused pdf through every
light path, the identities (fused pdf == light_pdf, composition over
first_stream, pdf off), the refusals and the plumbing."""
import ctypes as C

import numpy as np
import pytest

import nee_cases as N
import query_cases as Q
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

LINEAR, LIGHT_BVH, GRID, MIXED = 0, 1, 2, 3
LIGHT_SAMPLE = 3                              # rtw_query_stats.is_light_pdf


def same(a, b):
    """bit for bit up to the sign of zero, NaN masks equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def sample(soa, origins, seed, first_stream=0, sample_index=0, pdf=True, precision=rtw.RTW_F64, **tuning):
    """((directions, pdf, light), fused pdf == light_pdf, query stats) on a fresh context"""
    with rtw.Renderer(device=0, precision=precision) as r:
        for k, v in tuning.items():
            r.set_tuning(k, v)
        r.set_scene(soa)
        d, p, light = r.light_sample(origins, seed, first_stream, sample_index, pdf)
        st = r.get_query_stats()
        alone = r.light_pdf(np.concatenate([np.asarray(origins, d.dtype), d], 1)) if pdf else None
        return (d, p, light), alone, st


def check(soa, origins, seed, first_stream, sample_index, path, **tuning):
    want_d, want_i, want_p = N.light_samples(soa, origins, seed, first_stream, sample_index)
    (d, p, light), alone, st = sample(soa, origins, seed, first_stream, sample_index, **tuning)
    assert (st.kernel, st.is_light_pdf, st.rays) == (path, LIGHT_SAMPLE, len(origins))
    assert light.dtype == np.int32 and np.array_equal(light, want_i)
    assert same(d, want_d), np.flatnonzero(~((d == want_d) | (np.isnan(d) & np.isnan(want_d))).all(1))[:8]
    assert same(p, want_p), np.flatnonzero(~((p == want_p) | (np.isnan(p) & np.isnan(want_p))))[:8]
    assert same(p, alone)                      # the fused pdf is rtw_light_pdf_rays of {origin, direction}
    return d, p, light


def test_simple_sphere_lights_at_lambertian_bounces():
    soa, pts = N.bounce_points("simple")
    assert len(pts) >= 100 and len(soa.lights) == 19
    drawn = set()
    for first_stream, s in ((1000, 3), (5, 0)):
        d, p, light = check(soa, pts, 7, first_stream, s, LINEAR)
        assert np.isfinite(d).all() and (p > 0).sum() >= 100
        drawn |= set(light.tolist())
    assert drawn == set(range(19))             # every light is drawn
    # composition: one call equals its two halves; the pdf off gives the same directions
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        d, p, light = r.light_sample(pts, 7, 1000, 3)
        h = 77
        d0, p0, l0 = r.light_sample(pts[:h], 7, 1000, 3)
        d1, p1, l1 = r.light_sample(pts[h:], 7, 1000 + h, 3)
        assert same(np.concatenate([d0, d1]), d) and same(np.concatenate([p0, p1]), p)
        assert np.array_equal(np.concatenate([l0, l1]), light)
        dn, pn, ln = r.light_sample(pts, 7, 1000, 3, pdf=False)
        assert pn is None and same(dn, d) and np.array_equal(ln, light)
        assert r.get_query_stats().light_tests == 0
        # a 64-bit stream index
        want_d, want_i, _ = N.light_samples(soa, pts[:40], 7, (1 << 40) + 3, 1)
        dd, _, ll = r.light_sample(pts[:40], 7, (1 << 40) + 3, 1)
        assert same(dd, want_d) and np.array_equal(ll, want_i)


def test_64_lights_grid_light_bvh_and_linear_list_give_identical_bits():
    soa, _ = Q.scene("lights64")
    pts = np.ascontiguousarray(np.concatenate([N.bounce_points("simple")[1][:120], Q.rays_at_lights(soa, 1)[:, :3]]))
    got = {}
    for what, tuning, path in (("grid", {}, GRID), ("light BVH", {"light_grid": 0}, LIGHT_BVH),
                               ("linear", {"light_bvh_min": 1 << 20}, LINEAR)):
        got[what] = check(soa, pts, 11, 40, 2, path, **tuning)
    for what in ("grid", "light BVH"):
        assert same(got[what][0], got["linear"][0]) and same(got[what][1], got["linear"][1]), what
        assert np.array_equal(got[what][2], got["linear"][2])
    assert len(set(got["linear"][2].tolist())) >= 50


def test_cornell_box_mixed_list_and_the_default_entries():
    soa, pts = N.bounce_points("cornell_box", 200)
    assert len(pts) >= 100 and list(soa.light_kinds) == [1, 0]          # a quad light, a sphere
    d, p, light = check(soa, pts, 3, 9, 1, MIXED)
    assert set(light.tolist()) == {0, 1} and (p > 0).sum() >= 50
    # simple_transform: a RTW_LIGHTS_BVH_LEAF list of default entries -- random() is (1, 0, 0), pdf 0
    soa, _ = Q.scene("simple_transform")
    assert list(soa.light_kinds) == [2, 2, 2] and soa.light_flags == rtw.RTW_LIGHTS_BVH_LEAF
    pts = np.ascontiguousarray(Q.segments("simple_transform").rays[:70, :3])
    d, p, light = check(soa, pts, 3, 0, 0, MIXED)
    assert (d == [1.0, 0.0, 0.0]).all() and not p.any() and set(light.tolist()) == {0, 1, 2}


def test_bvh_leaf_list_and_origins_inside_a_light():
    soa, pts = N.bounce_points("simple")
    leaf = Q.with_lights(soa, soa.lights[:5], flags=rtw.RTW_LIGHTS_BVH_LEAF)
    check(leaf, pts[:150], 21, 7, 0, LINEAR)
    # origins inside a light sphere: the reference's NaN (sphere.rs:114-127), masks equal
    rng = np.random.default_rng(3)
    L = soa.lights
    inside = []
    for k in range(len(L)):
        for _ in range(3):
            off = rng.uniform(-1, 1, 3)
            inside.append(L[k, :3] + off * (0.6 * L[k, 3] / np.linalg.norm(off)))
    mixed = np.ascontiguousarray(np.concatenate([np.array(inside), pts[:60]]))
    d, p, light = check(soa, mixed, 7, 0, 0, LINEAR)
    own = light[:len(inside)] == np.repeat(np.arange(len(L)), 3)
    assert own.sum() >= 1 and np.isnan(d[:len(inside)][own]).any(1).all()      # its own light drawn: NaN
    assert np.isfinite(d[len(inside):]).all()


def test_an_empty_light_list_is_refused():
    soa, pts = N.bounce_points("simple")
    empty = Q.with_lights(soa, np.zeros((0, 4)))
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(empty)
        with pytest.raises(rtw.RenderError) as e:
            r.light_sample(pts[:8], 7)
        assert e.value.code == _capi.RTW_E_INVALID and "empty" in str(e.value)
        assert rtw._lib.rtw_light_sample(r.ctx, None, 0, 7, 0, 0, None, None, None) == _capi.RTW_E_INVALID


def test_counts_torch_stream_and_refusals():
    import torch
    lib = rtw._lib
    soa, pts = N.bounce_points("simple")
    pts = np.ascontiguousarray(np.tile(pts, (3, 1))[:600])
    want_d, want_i, want_p = N.light_samples(soa, pts, 7, 2, 1)
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        t = torch.from_numpy(pts).to("cuda:0")
        dirs = torch.zeros((600, 3), dtype=torch.float64, device="cuda:0")
        assert lib.rtw_light_sample_device(r.ctx, vp(t), 8, 7, 0, 0, vp(dirs), 8 * 24, None, 0, None, 0, None) \
            == _capi.RTW_E_NO_SCENE
        r.set_scene(soa)
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 600):
            d, p, light = r.light_sample(pts[:n], 7, 2, 1)
            assert d.shape == (n, 3) and p.shape == (n,) and light.shape == (n,)
            assert same(d, want_d[:n]) and same(p, want_p[:n]) and np.array_equal(light, want_i[:n]), n
            if n:
                assert r.get_query_stats().rays == n
        # the tail lanes write nothing beyond n
        for n in (1, 65, 257):
            guard = torch.full((n + 8, 3), -7.0, dtype=torch.float64, device="cuda:0")
            gp = torch.full((n + 8,), -7.0, dtype=torch.float64, device="cuda:0")
            gl = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda:0")
            assert lib.rtw_light_sample_device(r.ctx, vp(t), n, 7, 2, 1, vp(guard), 24 * n, vp(gp), 8 * n, vp(gl), 4 * n,
                                               None) == _capi.RTW_OK
            torch.cuda.synchronize()
            assert same(guard[:n].cpu().numpy(), want_d[:n]) and (guard[n:] == -7.0).all()
            assert same(gp[:n].cpu().numpy(), want_p[:n]) and (gp[n:] == -7.0).all() and (gl[n:] == -7).all()
        s = torch.cuda.Stream(device=0)
        with torch.cuda.stream(s):
            ts = torch.from_numpy(pts).to("cuda:0", non_blocking=True)
            d, p, light = r.light_sample(ts, 7, 2, 1)
            assert isinstance(d, torch.Tensor) and d.is_cuda and light.dtype == torch.int32
            doubled = d * 2
        s.synchronize()
        assert same(d.cpu().numpy(), want_d) and same(p.cpu().numpy(), want_p)
        assert np.array_equal(light.cpu().numpy(), want_i) and same(doubled.cpu().numpy(), 2 * want_d)
        with pytest.raises(rtw.RenderError):
            r.light_sample(ts.float(), 7)                        # a tensor of the other precision
        with pytest.raises(rtw.RenderError):
            r.light_sample(torch.from_numpy(pts), 7)             # a CPU tensor
        with pytest.raises(rtw.RenderError):
            r.light_sample(np.zeros((4, 6)), 7)                  # not [n, 3]
        run = lambda n, db, pb, lb: lib.rtw_light_sample_device(r.ctx, vp(t), n, 7, 0, 0, vp(dirs), db, vp(gp), pb,  # noqa: E731
                                                                vp(gl), lb, None)
        assert run(8, 8 * 24, 64, 32) == _capi.RTW_OK
        assert run(8, 8 * 24 - 1, 64, 32) == _capi.RTW_E_INVALID
        assert run(8, 8 * 24, 63, 32) == _capi.RTW_E_INVALID
        assert run(8, 8 * 24, 64, 31) == _capi.RTW_E_INVALID
        assert lib.rtw_light_sample_device(r.ctx, None, 8, 7, 0, 0, vp(dirs), 8 * 24, None, 0, None, 0, None) \
            == _capi.RTW_E_INVALID
        assert lib.rtw_light_sample_device(r.ctx, vp(t), 8, 7, 0, 0, None, 0, None, 0, None, 0, None) == _capi.RTW_E_INVALID
        assert lib.rtw_light_sample_device(r.ctx, None, 0, 7, 0, 0, None, 0, None, 0, None, 0, None) == _capi.RTW_OK
        torch.cuda.synchronize()
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        r.set_scene(soa)
        with pytest.raises(rtw.RenderError) as e:
            r.light_sample(pts[:4], 7)
        assert e.value.code == _capi.RTW_E_UNSUPPORTED


def test_hittable_list_convenience():
    world, lights, _ = rtw.scenes.simple(0x5EED0001)
    soa, pts = N.bounce_points("simple")
    want_d, want_i, want_p = N.light_samples(soa, pts[:80], 7, 1, 0)
    d, p, light = lights.random(pts[:80], 7, 1, 0, world=world)
    assert same(d, want_d) and same(p, want_p) and np.array_equal(light, want_i)
