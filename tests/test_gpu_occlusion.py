"""The any-hit query (rtw_occluded_rays) on the GPU in f64 against the
independent restatement (tests/nee_cases.py): world.hit(&r, t_min..=t_max[i])
.is_some() on the oracle's path segments with every kind of upper end, far
roots, every traversal, ray counts around the wave and workgroup sizes, the
early exit, and the plumbing.  Every comparison is exact; the expected bytes
never come from the GPU, and the conditions the reference meets on the inputs
are asserted on the CPU first (a surprise then points at the input)."""
import ctypes as C
import math

import numpy as np
import pytest

import nee_cases as N
import query_cases as Q
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

EPS, INF = N.EPS, N.INF
ANY_HIT = 2                                   # rtw_query_stats.is_light_pdf
WORLD_OF_KIND = {0: 2, 1: 3, 2: 4, 3: 5}      # rtw_query_stats.kernel of tuning bvh_kind


def occluded(soa, rays, t_max=None, t_min=EPS, precision=rtw.RTW_F64, accel=rtw.RTW_ACCEL_AUTO, **tuning):
    """(bytes, query stats) of one query on a fresh context"""
    with rtw.Renderer(device=0, precision=precision) as r:
        for k, v in tuning.items():
            r.set_tuning(k, v)
        r.set_accel(accel)
        r.set_scene(soa)
        occ = r.occluded(rays, t_max, t_min)
        return occ, (r.get_query_stats() if len(rays) else None)


# ------------------------------------------------------------ a. path segments
def test_the_reference_meets_the_identities_on_simple_and_so_does_the_gpu():
    seg, by_kind = N.simple_identities()
    hit = seg.ids >= 0
    assert (len(seg.rays), int(hit.sum()), int((hit & (seg.t < 1e-9)).sum())) == (239, 143, 40)
    want = {0: hit, 1: hit, 2: np.zeros_like(hit), 3: np.zeros_like(hit), 4: hit}   # inf, t, below t, t / 2, 2 t
    for kind, (on, model, off) in by_kind.items():
        assert np.array_equal(on, want[kind].astype(np.uint8)), N.KINDS[kind]
        assert np.array_equal(on, model) and np.array_equal(on, off), N.KINDS[kind]   # the gates decide nothing
    tt = np.where(hit, seg.t, 1.0)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(seg.soa)
        for kind in by_kind:
            t_max = np.array([N.t_max_of_kind(kind, float(t), 0.5) for t in tt])
            occ = r.occluded(seg.rays, t_max)
            assert occ.dtype == np.uint8 and np.array_equal(occ, by_kind[kind][0]), N.KINDS[kind]
        assert r.get_query_stats().kernel == 5


@pytest.mark.parametrize("name,worlds", [("simple", (5,)), ("simple63", (0, 1)), ("cornell_box", (0, 1)),
                                         ("simple_transform", (0, 1)), ("simple_light", (0, 1)), ("plane", (0, 1))])
def test_oracle_path_segments_with_every_kind_of_upper_end(name, worlds):
    soa, rays, t_max, want = N.mixed_batch(name)
    tunings = [{}] if name != "simple63" else [{"lds": 1}, {"lds": 0}]
    for tuning in tunings:
        occ, st = occluded(soa, rays, t_max, **tuning)
        assert st.kernel in worlds and st.is_light_pdf == ANY_HIT
        if "lds" in tuning:
            assert st.kernel == tuning["lds"]
        assert np.array_equal(occ, want), np.flatnonzero(occ != want)[:8]
        assert (st.rays, st.hits) == (len(rays), int(want.sum()))
    # NULL is every upper end +inf
    inf_want = N.reference(soa, rays, np.full(len(rays), INF))
    occ_null, _ = occluded(soa, rays, None)
    occ_inf, _ = occluded(soa, rays, np.full(len(rays), INF))
    assert np.array_equal(occ_null, inf_want) and np.array_equal(occ_inf, inf_want)


# ---------------------------------------------------------------- b. far roots
def _far_root_cases():
    grey = rtw.Lambertian((0.5, 0.5, 0.5))
    world = rtw.HittableList([rtw.Sphere((0.0, 0.0, 0.0), 1.0, grey), rtw.Sphere((4.0, 0.5, -1.0), 1.5, grey),
                              rtw.Sphere((-3.0, 0.0, 2.0), 0.25, grey)])
    soa = rtw.flatten(world, rtw.HittableList())
    rng = np.random.default_rng(5)
    rays, t_max = [], []
    for c, rad in ((np.zeros(3), 1.0), (np.array([4.0, 0.5, -1.0]), 1.5), (np.array([-3.0, 0.0, 2.0]), 0.25)):
        for _ in range(6):
            off = rng.uniform(-1, 1, 3)
            o = c + off * (0.7 * rad / np.linalg.norm(off))          # inside: the near root is negative
            d = rng.uniform(-1, 1, 3)
            oc = o - c
            a, hb, cc = d @ d, d @ oc, oc @ oc - rad * rad
            far = (-hb + math.sqrt(hb * hb - a * cc)) / a
            for hi in (far, math.nextafter(far, -INF), math.nextafter(far, INF), far * (1 - 1e-12), far * (1 + 1e-12),
                       far / 2, INF):
                rays.append(list(o) + list(d))
                t_max.append(hi)
    return soa, np.ascontiguousarray(rays), np.array(t_max)


def test_far_root_inside_spheres():
    soa, rays, t_max = _far_root_cases()
    want = N.reference(soa, rays, t_max, every_gate=True)
    # the far root is the only root in range: below it nothing is met
    assert want.reshape(-1, 7)[:, 6].all() and not want.reshape(-1, 7)[:, 5].any()
    assert 0 < want.sum() < len(want)
    for accel, world in ((rtw.RTW_ACCEL_BRUTE, 1), (rtw.RTW_ACCEL_BVH, 5)):
        occ, st = occluded(soa, rays, t_max, accel=accel)
        assert st.kernel == world
        assert np.array_equal(occ, want), (world, np.flatnonzero(occ != want)[:8])


def test_negative_radius_and_coincident_spheres():
    grey, red = rtw.Lambertian((0.5, 0.5, 0.5)), rtw.Metal((0.9, 0.1, 0.1), 0.0)
    world = rtw.HittableList([rtw.Sphere((0.0, 0.0, 0.0), -1.0, grey), rtw.Sphere((3.0, 0.0, 0.0), 1.0, grey),
                              rtw.Sphere((3.0, 0.0, 0.0), 1.0, red), rtw.Sphere((0.0, 0.0, -4.0), 1.0, red)])
    soa = rtw.flatten(world, rtw.HittableList())
    base = np.array([[0.0, 0.0, 5.0, 0.0, 0.0, -1.0], [0.0, 0.0, 0.0, 0.0, 0.0, -1.0], [0.0, 0.0, 5.0, 0.01, 0.02, -1.0],
                     [3.0, 0.0, 5.0, 0.0, 0.0, -1.0], [3.0, 0.0, 0.0, 0.3, 0.2, -1.0], [-3.0, 0.5, 0.0, 1.0, -0.1, 0.0]])
    ends = (INF, 0.5, 1.0, 2.0, 3.0, 4.0, 4.5, 6.0, 8.0, 10.0)
    rays = np.ascontiguousarray(np.repeat(base, len(ends), 0))
    t_max = np.tile(ends, len(base))
    # (a sphere of negative radius has an inverted box, which the reference's gate never passes)
    want = N.reference(soa, rays, t_max)
    assert 0 < want.sum() < len(want)
    for accel, world in ((rtw.RTW_ACCEL_BRUTE, 1), (rtw.RTW_ACCEL_BVH, 5)):
        occ, st = occluded(soa, rays, t_max, accel=accel)
        assert st.kernel == world and np.array_equal(occ, want), (world, np.flatnonzero(occ != want)[:8])


def test_t_min_zero_against_epsilon_on_rehit_rays():
    seg = Q.segments("simple")
    rehit = np.flatnonzero((seg.ids >= 0) & (seg.ids == seg.prev))[:120]
    rays = np.ascontiguousarray(seg.rays[rehit])
    assert len(rays) >= 100
    ends = np.where(np.arange(len(rays)) % 2 == 0, INF, seg.t[rehit])
    differ = None
    for t_min in (0.0, EPS):
        want = N.reference(seg.soa, rays, ends, t_min)
        if t_min == EPS:
            assert want.all()            # t itself is in range
        differ = want if differ is None else int((differ != want).sum())
        for accel, world in ((rtw.RTW_ACCEL_BRUTE, 1), (rtw.RTW_ACCEL_BVH, 5)):
            occ, st = occluded(seg.soa, rays, ends, t_min, accel=accel)
            assert st.kernel == world and np.array_equal(occ, want), (t_min, world)
    print(f"{len(rays)} re-hit rays, the answer differs between t_min 0 and EPSILON on {differ}")


# -------------------------------------------------------- c. every traversal
def test_every_traversal_gives_identical_bytes():
    soa, rays, t_max, want = N.mixed_batch("simple")
    configs = [("brute, lds 1", rtw.RTW_ACCEL_BRUTE, {"lds": 1}, 1), ("brute, lds 0", rtw.RTW_ACCEL_BRUTE, {"lds": 0}, 0)]
    for kind in (0, 1, 2, 3):
        for lds in (0, 1):
            configs.append((f"bvh_kind {kind}, lds {lds}", rtw.RTW_ACCEL_BVH, {"bvh_kind": kind, "lds": lds},
                            WORLD_OF_KIND[kind]))
    configs.append(("bvh_kind 3, bvh_lds_max 1", rtw.RTW_ACCEL_BVH, {"bvh_kind": 3, "bvh_lds_max": 1}, 3))
    failures = []
    for what, accel, tuning, world in configs:
        for robust in (0, 1):            # (f64 has one test form: the key must change nothing)
            occ, st = occluded(soa, rays, t_max, accel=accel, robust=robust, **tuning)
            if st.kernel != world:
                failures.append(f"{what}: ran world {st.kernel}, not {world}")
            if not np.array_equal(occ, want):
                failures.append(f"{what} robust {robust}: rays {np.flatnonzero(occ != want)[:6].tolist()} differ")
            if world >= 2 and not (st.node_visits > 0 and st.sphere_tests > 0):
                failures.append(f"{what}: no traversal work counted")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ d. counts
def test_ray_counts_and_guard_bytes():
    import torch
    soa, rays, t_max, want = N.mixed_batch("simple")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # a workgroup is 256 rays; at most 8 workgroups of 4 waves are resident per CU (8 waves per
    # SIMD), so the grid has at most 8 * cus workgroups and this count gives one a second block
    big = 2 * 256 * 8 * cus + 1
    lib = rtw._lib
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        for n in (0, 1, 63, 64, 65, 255, 256, 257, big):
            reps = -(-max(n, 1) // len(rays))
            rr = torch.from_numpy(np.tile(rays, (reps, 1))[:n].copy()).to("cuda:0")
            tm = torch.from_numpy(np.tile(t_max, reps)[:n].copy()).to("cuda:0")
            out = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
            rc = lib.rtw_occluded_rays_device(r.ctx, C.c_void_p(rr.data_ptr()) if n else None, n, EPS,
                                              C.c_void_p(tm.data_ptr()) if n else None, 8 * n,
                                              C.c_void_p(out.data_ptr()), n, None)
            assert rc == _capi.RTW_OK, n
            if n:
                assert r.get_query_stats().rays == n
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got[:n], np.tile(want, reps)[:n]), n
            assert (got[n:] == 0xAB).all(), n                      # the tail lanes write nothing
            h = r.occluded(np.tile(rays, (reps, 1))[:n], np.tile(t_max, reps)[:n]) if n <= 257 else None
            assert h is None or (h.shape == (n,) and np.array_equal(h, got[:n]))


# -------------------------------------------------------------- e. early exit
def test_rays_blocked_by_the_plane_never_enter_the_sphere_traversal():
    soa, _ = Q.scene("simple")
    assert len(soa.planes) == 1 and len(soa.spheres) == 484
    # the plane y = 0 is one-sided (plane.rs:61-76): rays from below, moving along +n, meet it
    rng = np.random.default_rng(9)
    n = 500
    o = np.stack([rng.uniform(-10, 10, n), rng.uniform(-3, -1, n), rng.uniform(-10, 10, n)], 1)
    d = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(0.5, 1.5, n), rng.uniform(-0.5, 0.5, n)], 1)
    rays = np.ascontiguousarray(np.concatenate([o, d], 1))
    t_plane = -o[:, 1] / d[:, 1]
    t_max = np.where(np.arange(n) % 2 == 0, INF, 2 * t_plane)
    want = N.reference(soa, rays[:60], t_max[:60], every_gate=True)
    assert want.all()
    for kind in (0, 1, 2, 3):
        occ, st = occluded(soa, rays, t_max, accel=rtw.RTW_ACCEL_BVH, bvh_kind=kind)
        assert st.kernel == WORLD_OF_KIND[kind] and occ.all()
        assert (st.node_visits, st.sphere_tests, st.hits) == (0, 0, n), kind      # a closest hit in disguise walks
    # the same rays stopped short of the plane do walk
    occ, st = occluded(soa, rays, 0.5 * t_plane)
    assert st.node_visits > 0
    # and an accepted sphere ends the walk: fewer visits than the closest-hit query of the same rays
    # (the while-while tree outside LDS: neither walk steals, so both counts are each lane's own --
    # the two walks are the same until a lane's first accepted sphere, after which only the
    # closest hit goes on)
    cam = Q.camera_rays("simple", 60, 40)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_tuning("bvh_kind", 1)
        r.set_accel(rtw.RTW_ACCEL_BVH)
        r.set_scene(soa)
        _, ids = r.hit_rays(cam)
        closest = r.get_query_stats()
        occ = r.occluded(cam)
        st = r.get_query_stats()
        assert closest.kernel == 3 and st.kernel == 3
        assert np.array_equal(occ, (ids[:, 0] >= 0).astype(np.uint8))
        print(f"{len(cam)} camera rays: node visits any hit {st.node_visits}, closest hit {closest.node_visits}; "
              f"sphere tests {st.sphere_tests}, {closest.sphere_tests}")
        assert st.node_visits < closest.node_visits


# --------------------------------------------------------------- f. plumbing
def test_torch_tensors_on_a_side_stream_equal_the_numpy_path():
    import torch
    soa, rays, t_max, want = N.mixed_batch("simple")
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        s = torch.cuda.Stream(device=0)
        with torch.cuda.stream(s):
            t = torch.from_numpy(rays).to("cuda:0", non_blocking=True)
            tm = torch.from_numpy(t_max).to("cuda:0", non_blocking=True)
            occ = r.occluded(t, tm)
            occ_inf = r.occluded(t)
            assert isinstance(occ, torch.Tensor) and occ.is_cuda and occ.dtype == torch.uint8
            total = occ.sum()           # torch work ordered after the query on the same stream
        s.synchronize()
        assert np.array_equal(occ.cpu().numpy(), want) and int(total) == int(want.sum())
        assert np.array_equal(occ_inf.cpu().numpy(), r.occluded(rays))
        with pytest.raises(rtw.RenderError):                 # a tensor of the other precision
            r.occluded(t.float())
        with pytest.raises(rtw.RenderError):                 # t_max of the other precision
            r.occluded(t, tm.float())
        with pytest.raises(rtw.RenderError):                 # a CPU tensor
            r.occluded(torch.from_numpy(rays))
        # numpy input of another dtype is converted, as hit_rays converts it
        assert np.array_equal(r.occluded(rays.astype(np.float32).astype(np.float64), t_max.astype(np.float32)),
                              r.occluded(rays.astype(np.float32), t_max.astype(np.float32)))
        with pytest.raises(rtw.RenderError):
            r.occluded(rays, t_max[:-1])


def test_refusals_and_stats():
    import torch
    lib = rtw._lib
    soa, _ = Q.scene("simple")
    rays = torch.zeros((8, 6), dtype=torch.float64, device="cuda:0")
    rays[:, 5] = -1.0
    tm = torch.full((8,), 3.0, dtype=torch.float64, device="cuda:0")
    occ = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        run = lambda n, t_min, tb, ob: lib.rtw_occluded_rays_device(r.ctx, vp(rays), n, t_min, vp(tm), tb, vp(occ), ob, None)  # noqa: E731
        assert run(8, 0.0, 64, 8) == _capi.RTW_E_NO_SCENE
        r.set_scene(soa)
        assert run(8, 0.0, 64, 8) == _capi.RTW_OK
        st = r.get_query_stats()
        assert (st.rays, st.is_light_pdf, st.kernel) == (8, ANY_HIT, 5) and st.kernel_ms > 0 and st.hits <= 8
        assert run(8, 0.0, 63, 8) == _capi.RTW_E_INVALID                               # short buffers
        assert run(8, 0.0, 64, 7) == _capi.RTW_E_INVALID
        for bad in (-1.0, float("nan"), float("inf"), -0.5e-300):
            assert run(8, bad, 64, 8) == _capi.RTW_E_INVALID, bad
        assert lib.rtw_occluded_rays_device(r.ctx, None, 8, 0.0, vp(tm), 64, vp(occ), 8, None) == _capi.RTW_E_INVALID
        assert lib.rtw_occluded_rays_device(r.ctx, vp(rays), 8, 0.0, vp(tm), 64, None, 8, None) == _capi.RTW_E_INVALID
        assert lib.rtw_occluded_rays_device(r.ctx, vp(rays), 8, 0.0, None, 0, vp(occ), 8, None) == _capi.RTW_OK
        assert lib.rtw_occluded_rays_device(r.ctx, None, 0, 0.0, None, 0, None, 0, None) == _capi.RTW_OK   # n = 0
        assert lib.rtw_occluded_rays(r.ctx, None, 0, 0.0, None, None) == _capi.RTW_OK
        assert lib.rtw_occluded_rays(r.ctx, None, 4, 0.0, None, None) == _capi.RTW_E_INVALID
        torch.cuda.synchronize()
        # NaN rays and NaN / short upper ends answer 0
        nan = float("nan")
        bad_rays = np.array([[nan, 0, 5, 0, 0, -1], [0, 0, 5, nan, 0, -1], [0, -2, 0, 0, 1, 0], [0, -2, 0, 0, 1, 0],
                             [0, -2, 0, 0, 1, 0]], np.float64)
        assert r.occluded(bad_rays, np.array([INF, INF, nan, EPS / 2, INF])).tolist() == [0, 0, 0, 0, 1]
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        r.set_scene(soa)
        assert lib.rtw_occluded_rays_device(r.ctx, vp(rays), 8, 0.0, None, 0, vp(occ), 8, None) == _capi.RTW_E_UNSUPPORTED
        with pytest.raises(rtw.RenderError) as e:
            r.occluded(np.zeros((4, 6)))
        assert e.value.code == _capi.RTW_E_UNSUPPORTED


def test_a_query_between_two_renders_leaves_them_identical():
    soa, b = Q.scene("simple")
    cam = b.copy().with_image_width(32).with_image_height(24).with_samples_per_pixel(16).with_max_depth(12).build()
    _, rays, t_max, want = N.mixed_batch("simple")
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        first = r.render(cam, 5)
        stats = (r.stats.segments, r.stats.kernel)
        kernel = r.last_kernel()
        assert np.array_equal(r.occluded(rays, t_max), want)
        assert r.last_kernel() == kernel and r.get_stats().segments == stats[0]
        second = r.render(cam, 5)
        assert (r.stats.segments, r.stats.kernel) == stats
    assert np.array_equal(first, second, equal_nan=True)


def test_hittable_list_convenience():
    world, lights, _ = rtw.scenes.simple(0x5EED0001)
    _, rays, t_max, want = N.mixed_batch("simple")
    assert np.array_equal(world.occluded(rays, t_max, lights=lights), want)
