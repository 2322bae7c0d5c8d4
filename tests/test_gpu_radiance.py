"""Radiance along arbitrary rays as one query (rtw_radiance_rays) on the GPU.

Every comparison is bit for bit with NaN masks equal (wavefront_cases.same), over
every row.  f64: the colours of camera_rays + radiance(rng) are the oracle's
traced sample of every pixel, render_radiance is render_window at chunk 1, and
colours, segments and the written-back states are the loop of the context's own
hit_rays, shade_rays and the advance rule (radiance_cases.compose).  f32: that
loop on the f32 context, bit for bit -- plain f32, as every query.  The seeded
and the rng mode agree, windows and streams compose, every world and light path
gives the same f64 bits, lanes out of phase keep their sample order, and the
edges: depth 0 and 1, survivors, a NaN ray, a zero state, two closed forms."""
import ctypes as C

import numpy as np
import pytest

import path_cases as P
import query_cases as Q
import radiance_cases as RC
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

same = RC.same
SEED, DEPTH, W, H = RC.SEED, RC.DEPTH, RC.W, RC.H
RADIANCE = 10                                 # rtw_query_stats.is_light_pdf
LINEAR, LIGHT_BVH, GRID, MIXED = 0, 1, 2, 3
WORLD_OF_KIND = {0: 2, 1: 3, 2: 4, 3: 5}      # rtw_query_stats.kernel of tuning bvh_kind
WORLDS = [("brute, lds 1", rtw.RTW_ACCEL_BRUTE, {"lds": 1}, 1), ("brute, lds 0", rtw.RTW_ACCEL_BRUTE, {"lds": 0}, 0)] + \
         [(f"bvh_kind {k}", rtw.RTW_ACCEL_BVH, {"bvh_kind": k}, WORLD_OF_KIND[k]) for k in range(4)]
PRECISIONS = [(rtw.RTW_F64, "f64"), (rtw.RTW_F32, "f32")]


def context(soa, precision=rtw.RTW_F64, accel=None, **tuning):
    r = rtw.Renderer(device=0, precision=precision)
    if accel is not None:
        r.set_accel(accel)
    for k, v in tuning.items():
        r.set_tuning(k, v)
    r.set_scene(soa)
    return r


def rows_off(a, b):
    a, b = np.asarray(a), np.asarray(b)
    ok = RC.WF.bits(a) == RC.WF.bits(b)
    return np.flatnonzero(~ok.reshape(len(a), -1).all(1))[:8]


def agrees(r, rays, rng0, depth, bg, what=""):
    """radiance(rng=) on these rays and start states against the loop of the context's own
    queries: colours, segments, the states afterwards, and the fold from zero"""
    rng = rng0.copy()
    rad, col, seg = r.radiance(rays, 0, 1, depth, bg, rng=rng, records=True)
    c, s, g = RC.compose(r, rays, rng0, depth, bg)
    assert same(col, c), (what, "colours", rows_off(col, c))
    assert np.array_equal(seg, s), (what, "segments", np.flatnonzero(seg != s)[:8])
    assert np.array_equal(rng, g), (what, "rng", rows_off(rng, g))
    assert same(rad, RC.fold(np.zeros((len(rays), 3)), col, 1)), (what, "fold")
    return rad, col, seg, rng


# ------------------------------------------------------------------- 1. f64 against the reference
@pytest.mark.parametrize("name", RC.SCENES)
def test_f64_is_the_oracles_sample_of_every_pixel(name):
    soa, _ = RC.scene(name)
    cam = RC.camera(name)
    want = RC.oracle_samples(name)
    with context(soa) as r:
        r.set_chunk(1)
        acc = np.zeros((W * H, 3))
        for a, s in enumerate(RC.SAMPLES):
            rays, rng0 = r.camera_rays(cam, SEED, s)
            assert len(rays) == W * H == 375
            rad, col, seg, _ = agrees(r, rays, rng0, DEPTH, cam.background, (name, s))
            assert same(col, want[a]), (name, s, rows_off(col, want[a]))
            acc = acc + want[a]
        sums = r.render_radiance(cam, SEED)
        ref = r.render_window(cam, SEED, 0, len(RC.SAMPLES))
        assert same(sums, ref) and same(sums.reshape(-1, 3), acc), name
        # a window continued is the whole
        a = r.render_radiance(cam, SEED, 0, 1)
        assert same(r.render_radiance(cam, SEED, 1, 2, sums=a), sums) and not same(a, sums)


# ------------------------------------------------------------------- 2. both precisions against the own queries
@pytest.mark.parametrize("precision,pname", PRECISIONS, ids=[p[1] for p in PRECISIONS])
@pytest.mark.parametrize("name", RC.SCENES)
def test_colours_segments_and_states_are_the_contexts_own_loop(name, precision, pname):
    soa, _ = RC.scene(name)
    cam = RC.camera(name)
    with context(soa, precision) as r:
        rays, _ = r.camera_rays(cam, SEED, 1)
        assert rays.dtype == (np.float32 if precision == rtw.RTW_F32 else np.float64)
        rng0 = RC.start_states(SEED, 0, len(rays), 1)
        rad, col, seg, rng = agrees(r, rays, rng0, DEPTH, cam.background, (name, pname))
        rng = rng0.copy()                      # (compose's queries ran since: the stats of the call alone)
        r.radiance(rays, 0, 1, DEPTH, cam.background, rng=rng)
        st = r.get_query_stats()
        assert st.is_light_pdf == RADIANCE and st.rays == int(seg.sum())
        for n in RC.SIZES:
            agrees(r, np.ascontiguousarray(rays[:n]), rng0[:n], DEPTH, cam.background, (name, pname, n))


@pytest.mark.parametrize("precision,pname", PRECISIONS, ids=[p[1] for p in PRECISIONS])
def test_depth_50(precision, pname):
    soa, _ = RC.scene("cornell_box")
    cam = RC.camera("cornell_box", 50)
    with context(soa, precision) as r:
        rays, rng0 = r.camera_rays(cam, SEED, 0)
        rad, col, seg, _ = agrees(r, rays, rng0, 50, cam.background, pname)
        assert seg.max() > DEPTH
        if precision == rtw.RTW_F64:
            assert same(col, RC.oracle_samples("cornell_box", 50)[0])


# ------------------------------------------------------------------- 3. seeded and rng modes agree
@pytest.mark.parametrize("precision,pname", PRECISIONS, ids=[p[1] for p in PRECISIONS])
def test_seeded_mode_is_the_rng_mode_on_the_streams_start_states(precision, pname):
    soa, _ = RC.scene("simple")
    cam = RC.camera("simple")
    with context(soa, precision) as r:
        rays, _ = r.camera_rays(cam, SEED, 0)
        for s in RC.SAMPLES:
            for first_stream in (0, (1 << 40) + 3):
                rng = RC.start_states(SEED, first_stream, len(rays), s)
                a = r.radiance(rays, 0, 1, DEPTH, cam.background, rng=rng, records=True)
                b = r.radiance(rays, SEED, 1, DEPTH, cam.background, first_stream, s, records=True)
                for x, y in zip(a, b):
                    assert same(x, y), (pname, s, first_stream)


# ------------------------------------------------------------------- 4. windows compose
@pytest.mark.parametrize("precision,pname", PRECISIONS, ids=[p[1] for p in PRECISIONS])
def test_sample_windows_and_streams_compose(precision, pname):
    soa, _ = RC.scene("cornell_box")
    cam = RC.camera("cornell_box")
    with context(soa, precision) as r:
        rays, _ = r.camera_rays(cam, SEED, 0)
        n = len(rays)
        whole, col, seg = r.radiance(rays, SEED, 3, DEPTH, cam.background, records=True)
        assert same(whole, RC.fold(np.zeros((n, 3)), col, 3))
        assert same(r.radiance(rays, SEED, 3, DEPTH, cam.background), whole)      # without records: the same sums
        acc = None
        for s in range(3):
            acc, c1, s1 = r.radiance(rays, SEED, 1, DEPTH, cam.background, 0, s, radiance=acc, records=True)
            assert same(c1, col[s::3]) and np.array_equal(s1, seg[s::3]), (pname, s)
        assert same(acc, whole)
        w0 = r.radiance(rays, SEED, 2, DEPTH, cam.background)
        assert not same(w0, whole)
        assert same(r.radiance(rays, SEED, 1, DEPTH, cam.background, 0, 2, radiance=w0.copy()), whole)
        # calls compose over first_stream
        a, h = 1000, 77
        big = r.radiance(rays, SEED, 3, DEPTH, cam.background, a, records=True)
        d0 = r.radiance(rays[:h], SEED, 3, DEPTH, cam.background, a, records=True)
        d1 = r.radiance(rays[h:], SEED, 3, DEPTH, cam.background, a + h, records=True)
        for x, y0, y1 in zip(big, d0, d1):
            assert same(np.concatenate([y0, y1]), x)
        assert not same(big[0], whole)                                        # (another stream, another answer)


# ------------------------------------------------------------------- 5. worlds and light paths
def base_answer(name):
    soa, _ = RC.scene(name)
    cam = RC.camera(name)
    with context(soa) as r:
        rays, _ = r.camera_rays(cam, SEED, 0)
        return rays, r.radiance(rays, SEED, 2, DEPTH, cam.background, records=True)


@pytest.mark.parametrize("what,accel,tuning,world", WORLDS, ids=[w[0] for w in WORLDS])
def test_every_world_gives_identical_f64_bits_and_its_own_f32_loop(what, accel, tuning, world):
    for name in ("simple", "lights64_emissive", "cornell_box"):
        soa, _ = RC.scene(name)
        cam = RC.camera(name)
        rays, want = base_answer(name)
        with context(soa, accel=accel, **tuning) as r:
            got = r.radiance(rays, SEED, 2, DEPTH, cam.background, records=True)
            st = r.get_query_stats()
            assert name != "simple" or st.kernel == world
            for x, y in zip(got, want):
                assert same(x, y), (name, what)
    soa, _ = RC.scene("simple")
    cam = RC.camera("simple")
    with context(soa, rtw.RTW_F32, accel=accel, **tuning) as r:
        rays32, _ = r.camera_rays(cam, SEED, 0)
        agrees(r, rays32, RC.start_states(SEED, 0, len(rays32), 0), DEPTH, cam.background, what)
        r.radiance(rays32, SEED, 1, DEPTH, cam.background)
        assert r.get_query_stats().kernel == world


LIGHT_PATHS = (("grid", {}, GRID), ("light BVH", {"light_grid": 0}, LIGHT_BVH), ("linear", {"light_bvh_min": 1 << 20}, LINEAR))


@pytest.mark.parametrize("what,tuning,path", LIGHT_PATHS, ids=[p[0] for p in LIGHT_PATHS])
def test_every_light_path_gives_identical_f64_bits_and_its_own_f32_loop(what, tuning, path):
    name = "lights64_emissive"
    soa, _ = RC.scene(name)
    cam = RC.camera(name)
    rays, want = base_answer(name)
    with context(soa, **tuning) as r:
        got = r.radiance(rays, SEED, 2, DEPTH, cam.background, records=True)
        for x, y in zip(got, want):
            assert same(x, y), what
        r.light_sample(rays[:, :3], SEED)
        assert r.get_query_stats().kernel == path, what
    # the light BVH under a BVH world: its stacks behind the closest hit's LDS
    for accel, extra in ((None, {}), (rtw.RTW_ACCEL_BVH, {"bvh_kind": 3})):
        with context(soa, rtw.RTW_F32, accel=accel, **tuning, **extra) as r:
            rays32, _ = r.camera_rays(cam, SEED, 0)
            agrees(r, rays32, RC.start_states(SEED, 0, len(rays32), 0), DEPTH, cam.background, (what, accel))
    with context(soa, accel=rtw.RTW_ACCEL_BVH, bvh_kind=3, **tuning) as r:
        got = r.radiance(rays, SEED, 2, DEPTH, cam.background, records=True)
        for x, y in zip(got, want):
            assert same(x, y), (what, "bvh_kind 3")


# ------------------------------------------------------------------- 6. lanes out of phase
@pytest.mark.parametrize("precision,pname", PRECISIONS, ids=[p[1] for p in PRECISIONS])
@pytest.mark.parametrize("grid,n", [(0, 64), (1, 600)])
def test_lanes_out_of_phase_keep_sample_order_and_streams(grid, n, precision, pname):
    """One wave alternates rays that miss at round 0 with rays inside the closed box at depth
    50, S = 4: a lane regenerates while its neighbours are mid-path."""
    soa, _ = RC.scene("cornell_box")
    S, depth, bg = 4, 50, (0.25, 0.5, 1.0)
    dt = np.float32 if precision == rtw.RTW_F32 else np.float64
    rays = np.ascontiguousarray(RC.cornell_phase_rays(n).astype(dt))
    with context(soa, precision, query_grid=grid) as r:
        rad, col, seg = r.radiance(rays, SEED, S, depth, bg, first_stream=9, records=True)
        st = r.get_query_stats()
        assert st.is_light_pdf == RADIANCE and st.rays == int(seg.sum())
        for j in range(S):
            c, s, _ = RC.compose(r, rays, RC.start_states(SEED, 9, n, j), depth, bg)
            assert same(col[j::S], c), (pname, j, rows_off(col[j::S], c))
            assert np.array_equal(seg[j::S], s), (pname, j)
        assert same(rad, RC.fold(np.zeros((n, 3)), col, S))
        assert (seg.reshape(n, S)[0::2] == 1).all() and seg.reshape(n, S)[1::2].mean() > 3
        assert same(col.reshape(n, S, 3)[0::2], np.broadcast_to(np.asarray(bg, dt), (n // 2, S, 3)))


# ------------------------------------------------------------------- 7. edges
@pytest.mark.parametrize("precision,pname", PRECISIONS, ids=[p[1] for p in PRECISIONS])
def test_depth_0_and_1_survivors_a_nan_ray_and_a_zero_state(precision, pname):
    soa, _ = RC.scene("cornell_box")
    cam = RC.camera("cornell_box")
    bg = (0.25, 0.5, 1.0)
    with context(soa, precision) as r:
        rays, rng0 = r.camera_rays(cam, SEED, 0)
        n = len(rays)
        # depth 0: 0 + 0 for every sample, nothing traced, the states untouched
        rng = rng0.copy()
        rad, col, seg = r.radiance(rays, 0, 1, 0, bg, rng=rng, records=True)
        assert not rad.any() and not col.any() and not seg.any() and np.array_equal(rng, rng0)
        assert not np.signbit(col).any() and not np.signbit(rad).any()
        rad, col, seg = r.radiance(rays, SEED, 3, 0, bg, radiance=np.full((n, 3), 2.5), records=True)
        assert (rad == 2.5).all() and not col.any() and not seg.any()
        assert r.get_query_stats().rays == 0
        # depth 1 and 2: the survivors of the last round get 0 + res
        for depth in (1, 2):
            _, col, seg, _ = agrees(r, rays, rng0, depth, bg, (pname, depth))
            longer = RC.compose(r, rays, rng0, depth + 1, bg)[1]
            alive = longer > depth
            assert alive.any() and (seg[alive] == depth).all()
            if depth == 1:
                assert not col[alive].any()                                  # res is still 0
        # a NaN ray between live rows: it meets nothing, the background
        odd = rays.copy()
        odd[[5, 70, 300], 3] = np.nan
        odd[71, :] = np.nan
        _, col, seg, _ = agrees(r, odd, rng0, DEPTH, bg, (pname, "NaN"))
        assert (seg[[5, 70, 71, 300]] == 1).all() and same(col[[5, 70, 71, 300]], np.tile(np.asarray(bg, col.dtype), (4, 1)))
        # zero-state rows: the stream of (0, 0, 0) from the first hit on; a row that misses keeps its zeros
        z = rng0.copy()
        zero = [0, 64, 65, 187, 374, 375]
        z[zero[:-1]] = 0
        mixed = np.ascontiguousarray(np.concatenate([rays, RC.cornell_phase_rays(2).astype(rays.dtype)[:1]]))
        z = np.concatenate([z, np.zeros((1, 4), np.uint64)])
        _, col, seg, after = agrees(r, mixed, z, DEPTH, bg, (pname, "zero state"))
        met = r.hit_rays(mixed)[1][zero, 0] >= 0
        assert np.array_equal(after[zero].any(1), met) and met[3] and not met[5] and seg[375] == 1


@pytest.mark.parametrize("precision,pname", PRECISIONS, ids=[p[1] for p in PRECISIONS])
def test_closed_forms(precision, pname):
    dt = np.float32 if precision == rtw.RTW_F32 else np.float64
    S = 5
    # inside one DiffuseLight sphere: every sample is (1, 1, 1) * E + 0 = E, the sum S * E exactly
    rays = np.ascontiguousarray(RC.rays_from_inside().astype(dt))
    with context(RC.inside_a_light(), precision) as r:
        rad, col, seg = r.radiance(rays, SEED, S, DEPTH, (9.0, 9.0, 9.0), records=True)
        E = np.asarray(RC.LIGHT_E, dt)
        assert same(col, np.tile(E, (len(rays) * S, 1))) and (seg == 1).all()
        assert same(rad, np.tile(E.astype(np.float64) * S, (len(rays), 1)))
        st = r.get_query_stats()
        assert st.rays == len(rays) * S and st.hits == 0
    # an empty direction: the f64 fold of S backgrounds, rounded to the context's precision first
    soa, _ = RC.scene("cornell_box")
    away = np.ascontiguousarray(RC.cornell_phase_rays(130).astype(dt)[0::2])
    bg = (0.1, 0.7, 1.0 / 3.0)
    with context(soa, precision) as r:
        rad, col, seg = r.radiance(away, SEED, S, DEPTH, bg, records=True)
        b = np.asarray(bg, dt)
        fold = np.zeros(3)
        for _ in range(S):
            fold = fold + b.astype(np.float64)
        assert same(col, np.tile(b, (len(away) * S, 1))) and same(rad, np.tile(fold, (len(away), 1)))


# ------------------------------------------------------------------- 8. interface
def test_refusals_and_empty_calls():
    soa, _ = RC.scene("cornell_box")
    cam = RC.camera("cornell_box")
    inv = _capi.RTW_E_INVALID

    def refused(code, fn):
        with pytest.raises(rtw.RenderError) as e:
            fn()
        assert e.value.code == code

    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        refused(_capi.RTW_E_NO_SCENE, lambda: r.radiance(np.zeros((1, 6)), 1))
    for name in sorted(P.NO_LIGHTS):
        with context(Q.scene(name)[0]) as r:
            refused(_capi.RTW_E_NO_LIGHTS, lambda: r.radiance(np.zeros((1, 6)), 1))
    with context(soa) as r:
        rays, rng = r.camera_rays(cam, SEED, 0)
        refused(inv, lambda: r.radiance(rays, 1, 0))
        refused(inv, lambda: r.radiance(rays, 1, 2, rng=rng))
        refused(inv, lambda: r.radiance(rays, 1, 2, first_sample=0xFFFFFFFF))
        assert r.radiance(rays[:3], 1, 1, first_sample=0xFFFFFFFF).shape == (3, 3)
        refused(inv, lambda: r.radiance(rays, 1, radiance=np.zeros((3, 3))))
        refused(inv, lambda: r.radiance(rays, 1, rng=rng[:5].copy()))
        refused(inv, lambda: r.radiance(np.zeros((4, 5)), 1))
        out = r.radiance(np.zeros((0, 6)), 1, 2, records=True)
        assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[2].shape == (0,)
        # the device form: short and misaligned buffers (host pointers: refused before any is read)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        r8, g8, rad = np.zeros((8, 6)), np.ones((8, 4), np.uint64), np.zeros((8, 3))
        col, seg = np.zeros((8, 3)), np.zeros(8, np.uint32)
        bg = (C.c_double * 3)(0.0, 0.0, 0.0)
        dev = lambda *a: rtw._lib.rtw_radiance_rays_device(r.ctx, *a, None)   # noqa: E731
        ok_args = [vp(r8), r8.nbytes, 8, 1, 0, 0, 1, DEPTH, bg, vp(g8), g8.nbytes, 0, vp(rad), rad.nbytes,
                   vp(col), col.nbytes, vp(seg), seg.nbytes]
        for at, short in ((1, r8.nbytes - 1), (10, g8.nbytes - 1), (13, rad.nbytes - 1), (15, col.nbytes - 1),
                          (17, seg.nbytes - 1)):
            a = list(ok_args)
            a[at] = short
            assert dev(*a) == inv, at
        big = np.zeros(16 * 6 + 2)
        mis = big.ctypes.data + (8 if big.ctypes.data % 16 == 0 else 0)   # 8 B off a 16 B boundary
        assert mis % 16 == 8
        for at, off in ((0, 0), (9, 0), (12, 4), (14, 4), (16, 2)):       # rays, rng: 16 B; radiance, colours: 8 B; segments: 4 B
            a = list(ok_args)
            a[at] = C.c_void_p(mis + off)
            assert dev(*a) == inv, at
        a = list(ok_args)
        a[6] = 2                                                          # rng with n_samples = 2
        assert dev(*a) == inv
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        r.set_scene(soa)
        refused(_capi.RTW_E_UNSUPPORTED, lambda: r.radiance(np.zeros((1, 6)), 1))


def test_stats_torch_entry_and_renders_unchanged():
    import torch
    soa, _ = RC.scene("simple")
    cam = RC.camera("simple")
    for precision, pname in PRECISIONS:
        with context(soa, precision) as r:
            before = r.render(cam, SEED)
            rays, rng0 = r.camera_rays(cam, SEED, 0)
            rad, col, seg = r.radiance(rays, SEED, 2, DEPTH, cam.background, records=True)
            st = r.get_query_stats()
            assert st.is_light_pdf == RADIANCE and st.rays == int(seg.sum()) and st.kernel_ms > 0
            # hits are the SCATTER events: those of the loop's rounds, both samples
            scatter = 0
            for j in range(2):
                cur, g = rays, RC.start_states(SEED, 0, len(rays), j)
                for _ in range(DEPTH):
                    if not len(cur):
                        break
                    hits, ids = r.hit_rays(cur)
                    nxt, _, _, event = r.shade_rays(cur, hits, ids, g)
                    scatter += int((event == _capi.RTW_EVENT_SCATTER).sum())
                    keep = event >= _capi.RTW_EVENT_REFLECT
                    cur, g = np.ascontiguousarray(nxt[keep]), np.ascontiguousarray(g[keep])
            assert st.hits == scatter and st.node_visits > 0 and st.sphere_tests > 0
            # the torch device entry: the same bits, tensors on the GPU
            t_rays = torch.as_tensor(rays, device="cuda:0")
            t = r.radiance(t_rays, SEED, 2, DEPTH, cam.background, records=True)
            assert all(x.is_cuda for x in t)
            assert same(t[0].cpu().numpy(), rad) and same(t[1].cpu().numpy(), col)
            assert np.array_equal(t[2].cpu().numpy().view(np.uint32), seg)
            t_rng = torch.as_tensor(rng0.view(np.int64), device="cuda:0")
            h_rng = rng0.copy()
            a = r.radiance(t_rays, 0, 1, DEPTH, cam.background, rng=t_rng, radiance=t[0].clone())
            b = r.radiance(rays, 0, 1, DEPTH, cam.background, rng=h_rng, radiance=rad.copy())
            assert same(a.cpu().numpy(), b) and np.array_equal(t_rng.cpu().numpy().view(np.uint64), h_rng)
            assert same(r.render(cam, SEED), before), pname                   # a render after the queries is unchanged


def test_hittable_list_convenience():
    """the world's entry stages the scene for one call"""
    world, lights, _ = rtw.scenes.simple(0x5EED0001)
    soa, _ = RC.scene("simple")
    cam = RC.camera("simple")
    with context(soa) as r:
        rays, _ = r.camera_rays(cam, SEED, 0)
        want = r.radiance(rays[:65], SEED, 2, DEPTH, cam.background, records=True)
    got = world.radiance(rays[:65], SEED, 2, DEPTH, cam.background, lights=lights, records=True)
    for x, y in zip(got, want):
        assert same(x, y)
