"""The feature pass (rtw_render_features) on the GPU against the oracle
expectations of tests/feature_cases.py: every scene family, sample windows,
per-pixel counts, image sizes around the tile, every traversal, the pairing
with adaptive sampling, isolation from renders and queries, the device form.
All f64 comparisons are bit for bit up to the sign of zero with equal NaN
masks; no expected value comes from the GPU."""
import ctypes as C

import numpy as np
import pytest

import feature_cases as F
import query_cases as Q
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

WORLD_OF_KIND = {0: 2, 1: 3, 2: 4, 3: 5}      # rtw_query_stats.kernel of tuning bvh_kind
same = F.same


def renderer(name, precision=rtw.RTW_F64, accel=rtw.RTW_ACCEL_AUTO, **tuning):
    r = rtw.Renderer(device=0, precision=precision)
    for k, v in tuning.items():
        r.set_tuning(k, v)
    r.set_accel(accel)
    r.set_scene(F.scene(name)[0])
    return r


def where_differs(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    return np.argwhere(bad)[:6].tolist()


def raw_features(r, cam, seed, first, n, counts, features, ids):
    """rtw_render_features on the caller's arrays (ids too, which the Python form allocates)"""
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = rtw._lib.rtw_render_features(r.ctx, C.byref(cam.raw), C.c_uint64(seed), first, n, vp(counts), vp(features),
                                      vp(ids))
    assert rc == 0, rtw._lib.rtw_last_error(r.ctx)


# ------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("name,worlds", [("simple", (5,)), ("simple63", (0, 1)), ("cornell_box", (0, 1)),
                                         ("cornell_box_front", (0, 1)), ("simple_transform", (0, 1)),
                                         ("simple_light", (0, 1)), ("plane", (0, 1)), ("checkered_spheres", (0, 1)),
                                         ("perlin_spheres", (0, 1)), ("simple_defocus", (5,))])
def test_features_and_ids_are_the_oracles(name, worlds):
    e = F.samples(name)
    with renderer(name) as r:
        feat, ids = r.render_features(e.cam, e.seed, 0, F.SAMPLES)
        st = r.get_query_stats()
    want = e.fold(0, F.SAMPLES)
    assert feat.shape == (F.H, F.W, 8) and ids.shape == (F.H, F.W, 2) and ids.dtype == np.int32
    assert st.kernel in worlds and st.is_light_pdf == 0
    assert np.array_equal(ids, e.ids()), np.argwhere(ids != e.ids())[:6].tolist()
    assert same(feat[..., 7], want[..., 7]), where_differs(feat[..., 7], want[..., 7])          # hits
    assert same(feat[..., 6], want[..., 6]), where_differs(feat[..., 6], want[..., 6])          # distance
    assert same(feat[..., 3:6], want[..., 3:6]), where_differs(feat[..., 3:6], want[..., 3:6])  # normal
    assert same(feat[..., 0:3], want[..., 0:3]), where_differs(feat[..., 0:3], want[..., 0:3])  # albedo
    assert (st.rays, st.hits) == (F.H * F.W * F.SAMPLES, int(want[..., 7].sum()))
    if 5 in worlds:
        assert st.node_visits > 0 and st.sphere_tests > 0
    else:
        assert st.node_visits == 0 and st.sphere_tests == st.rays * len(e.soa.spheres)


# ----------------------------------------------------------------- 2. windows
def test_windows_continue_bit_for_bit_and_leave_ids_alone():
    e = F.samples("simple")
    with renderer("simple") as r:
        feat, ids = r.render_features(e.cam, e.seed, 0, 1)
        assert same(feat, e.fold(0, 1)) and np.array_equal(ids, e.ids())
        again, none = r.render_features(e.cam, e.seed, 1, 3, features=feat)
        assert again is feat and none is None
        assert same(feat, e.fold(0, 4)), where_differs(feat, e.fold(0, 4))
        # sample 3 alone onto zeros; the caller's ids are not touched by a call that starts later
        alone = np.zeros((F.H, F.W, 8))
        marks = np.full((F.H, F.W, 2), -77, np.int32)
        raw_features(r, e.cam, e.seed, 3, 1, None, alone, marks)
        assert same(alone, e.fold(3, 1)), where_differs(alone, e.fold(3, 1))
        assert (marks == -77).all()
        raw_features(r, e.cam, e.seed, 1, 3, None, feat.copy(), marks)
        assert (marks == -77).all()
        assert r.get_query_stats().rays == F.H * F.W * 3
        # n = 0 does nothing
        before = alone.copy()
        raw_features(r, e.cam, e.seed, 2, 0, None, alone, marks)
        assert same(alone, before) and (marks == -77).all()


# ------------------------------------------------------------------ 3. counts
def _counts_inside_tiles():
    """0..4, varying inside every 8 x 8 tile: the lanes of a wave stop at different trips"""
    jj, ii = np.mgrid[0:F.H, 0:F.W]
    return ((3 * ii + 5 * jj + (ii * jj) % 3) % 5).astype(np.uint32)


def _counts_per_tile():
    """constant per 8 x 8 tile, as adaptive sampling gives them; one tile takes none"""
    jj, ii = np.mgrid[0:F.H, 0:F.W]
    return (((ii // 8) * 2 + (jj // 8) * 3) % 5).astype(np.uint32)


@pytest.mark.parametrize("counts_of", [_counts_inside_tiles, _counts_per_tile], ids=["inside_tiles", "per_tile"])
def test_counts_clip_each_pixel(counts_of):
    e = F.samples("simple")
    counts = counts_of()
    assert set(np.unique(counts)) == {0, 1, 2, 3, 4}
    if counts_of is _counts_inside_tiles:
        assert len(np.unique(counts[:8, :8])) == 5
    want = e.fold(0, F.SAMPLES, counts=counts)
    marks = np.full((F.H, F.W, 2), -77, np.int32)
    with renderer("simple") as r:
        feat, ids = r.render_features(e.cam, e.seed, 0, F.SAMPLES, counts=counts)
        st = r.get_query_stats()
        assert same(feat, want), where_differs(feat, want)
        assert np.array_equal(ids, e.ids(counts=counts))
        assert not feat[counts == 0].any() and (counts == 0).sum() > 0
        assert st.rays == int(np.minimum(counts, F.SAMPLES).sum()) and st.hits == int(feat[..., 7].sum())
        assert st.hits == int(want[..., 7].sum())
        # the ids of a pixel that takes no sample stay the caller's
        feat2 = np.zeros((F.H, F.W, 8))
        raw_features(r, e.cam, e.seed, 0, F.SAMPLES, counts, feat2, marks)
        assert np.array_equal(marks, e.ids(counts=counts, onto=marks)) and (marks[counts == 0] == -77).all()
        assert same(feat2, want)
        # counts clip a window too: [1, 3) of each pixel onto its first sample
        head = e.fold(0, 1, counts=counts)
        cont, _ = r.render_features(e.cam, e.seed, 1, 2, counts=counts, features=head.copy())
        assert same(cont, e.fold(0, 3, counts=counts))
        assert r.get_query_stats().rays == int((np.minimum(counts, 3) - np.minimum(counts, 1)).sum())


# ---------------------------------------------- 4. image sizes around the tile
@pytest.mark.parametrize("width,height", [(1, 1), (7, 9), (8, 8), (9, 17), (40, 24)])
def test_image_sizes_around_the_tile(width, height):
    e = F.samples("simple", width, height, 2)
    want = e.fold(0, 2)
    guard_f, guard_i = 16, 8
    feat = np.full(width * height * 8 + guard_f, -12345.0)
    ids = np.full(width * height * 2 + guard_i, -77, np.int32)
    with renderer("simple") as r:
        raw_features(r, e.cam, e.seed, 0, 2, None, feat, ids)
        assert r.get_query_stats().rays == width * height * 2
        # ... and the device form, on guarded device buffers
        import torch
        d_feat = torch.full((width * height * 8 + guard_f,), -12345.0, dtype=torch.float64, device="cuda:0")
        d_ids = torch.full((width * height * 2 + guard_i,), -77, dtype=torch.int32, device="cuda:0")
        rc = rtw._lib.rtw_render_features_device(r.ctx, C.byref(e.cam.raw), C.c_uint64(e.seed), 0, 2, None, 0,
                                                 C.c_void_p(d_feat.data_ptr()), width * height * 64,
                                                 C.c_void_p(d_ids.data_ptr()), width * height * 8,
                                                 C.c_void_p(rtw.torch_stream(0)))
        assert rc == 0
        torch.cuda.synchronize()
    for f, i in ((feat, ids), (d_feat.cpu().numpy(), d_ids.cpu().numpy())):
        assert (f[-guard_f:] == -12345.0).all() and (i[-guard_i:] == -77).all()
        got = f[:-guard_f].reshape(height, width, 8)
        assert same(got, want), where_differs(got, want)
        assert np.array_equal(i[:-guard_i].reshape(height, width, 2), e.ids())


# ------------------------------------------------------- 5. every traversal
@pytest.mark.parametrize("precision", [rtw.RTW_F64, rtw.RTW_F32], ids=["f64", "f32"])
def test_every_traversal_gives_the_brute_force_features(precision):
    e = F.samples("simple")
    counts = _counts_inside_tiles()                 # lanes without a ray in every wave: thieves

    def run(accel, **tuning):
        with renderer("simple", precision, accel, **tuning) as r:
            feat, ids = r.render_features(e.cam, e.seed, 0, F.SAMPLES)
            cf, _ = r.render_features(e.cam, e.seed, 0, F.SAMPLES, counts=counts)
            return feat, ids, cf, r.get_query_stats()

    ref_f, ref_i, ref_c, st = run(rtw.RTW_ACCEL_BRUTE, lds=1)
    assert st.kernel == 1
    assert (ref_i[..., 0] >= 0).sum() > 100 and (ref_i[..., 0] < 0).sum() > 100
    if precision == rtw.RTW_F64:      # the brute-force pass itself is the oracle's
        assert same(ref_f, e.fold(0, F.SAMPLES)) and same(ref_c, e.fold(0, F.SAMPLES, counts=counts))
    # (f32 against f64: no bound can be derived; tools/feature_bench.py prints the differences)
    configs = [("brute, lds 0", rtw.RTW_ACCEL_BRUTE, {"lds": 0}, 0)]
    for kind in (0, 1, 2, 3):
        for lds in (0, 1):
            configs.append((f"bvh_kind {kind}, lds {lds}", rtw.RTW_ACCEL_BVH, {"bvh_kind": kind, "lds": lds},
                            WORLD_OF_KIND[kind]))
    configs.append(("bvh_kind 3, bvh_lds_max 1", rtw.RTW_ACCEL_BVH, {"bvh_kind": 3, "bvh_lds_max": 1}, 3))
    failures = []
    for what, accel, tuning, world in configs:
        f, i, c, st = run(accel, **tuning)
        if st.kernel != world:
            failures.append(f"{what}: ran world {st.kernel}, not {world}")
        if not (np.array_equal(i, ref_i) and same(f, ref_f)):
            failures.append(f"{what}: features differ from brute force at {where_differs(f, ref_f)}")
        if not same(c, ref_c):
            failures.append(f"{what}: features under counts differ from brute force at {where_differs(c, ref_c)}")
        if world >= 2 and not (st.node_visits > 0 and st.sphere_tests > 0):
            failures.append(f"{what}: no traversal work counted")
    assert not failures, "\n".join(failures)


# --------------------------------------------------------- 6. adaptive pairing
def test_features_of_the_samples_an_adaptive_render_took():
    width, height, mn, mx, win = 24, 16, 2, 6, 2
    e = F.samples("simple", width, height, mx)
    with renderer("simple") as r:
        _, counts = r.render_adaptive(e.cam, e.seed, mn, mx, win, 1.0 / 32)
        feat, ids = r.render_features(e.cam, e.seed, 0, mx, counts=counts)
    assert counts.min() >= mn and counts.max() <= mx
    want = e.fold(0, mx, counts=counts)
    assert same(feat, want), where_differs(feat, want)
    assert (feat[..., 7] <= counts).all() and np.array_equal(ids, e.ids())
    albedo, normal, distance, coverage = rtw.feature_means(feat, counts)
    assert np.isfinite(albedo).all() and ((coverage >= 0) & (coverage <= 1)).all()


# ---------------------------------------------------------------- 7. isolation
def test_renders_and_queries_around_a_pass_are_unchanged():
    e = F.samples("simple")
    seg = Q.segments("simple")
    rays = np.ascontiguousarray(seg.rays[:500])
    with renderer("simple") as r:
        img0 = r.render(e.cam, e.seed)
        h0, i0 = r.hit_rays(rays)
        feat, _ = r.render_features(e.cam, e.seed, 0, F.SAMPLES)
        img1 = r.render(e.cam, e.seed)
        h1, i1 = r.hit_rays(rays)
        qs = r.get_query_stats()
        feat2, _ = r.render_features(e.cam, e.seed, 0, F.SAMPLES)
    assert same(img0, img1) and same(h0, h1) and np.array_equal(i0, i1)
    assert qs.rays == len(rays)
    assert same(feat, e.fold(0, F.SAMPLES)) and same(feat2, feat)


# -------------------------------------------------------------- 8. device form
def test_device_form_on_a_side_stream_is_the_host_form():
    import torch
    e = F.samples("simple")
    counts = _counts_inside_tiles()
    want = e.fold(0, F.SAMPLES, counts=counts)
    with renderer("simple") as r:
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            d_counts = torch.from_numpy(counts.astype(np.int32)).to("cuda:0")
            d_feat, d_ids = r.render_features(e.cam, e.seed, 0, 1, counts=d_counts)
            assert d_feat.is_cuda and d_feat.dtype == torch.float64 and d_ids.dtype == torch.int32
            again, none = r.render_features(e.cam, e.seed, 1, 3, counts=d_counts, features=d_feat)
            assert again is d_feat and none is None
        side.synchronize()
        host, host_ids = r.render_features(e.cam, e.seed, 0, F.SAMPLES, counts=counts)
    assert same(d_feat.cpu().numpy(), want) and same(host, want)
    assert np.array_equal(d_ids.cpu().numpy(), host_ids) and np.array_equal(host_ids, e.ids(counts=counts))
    # what the device form refuses: a short or misaligned buffer
    with renderer("simple") as r:
        buf = torch.zeros(F.H * F.W * 8 + 1, dtype=torch.float64, device="cuda:0")
        call = lambda ptr, nbytes: rtw._lib.rtw_render_features_device(   # noqa: E731
            r.ctx, C.byref(e.cam.raw), C.c_uint64(1), 0, 1, None, 0, C.c_void_p(ptr), nbytes, None, 0, None)
        assert call(buf.data_ptr(), F.H * F.W * 64 - 8) == _capi.RTW_E_INVALID
        assert call(buf.data_ptr() + 8, F.H * F.W * 64) == _capi.RTW_E_INVALID
        assert call(buf.data_ptr(), F.H * F.W * 64) == 0


def test_refusals_on_a_context():
    e = F.samples("simple")
    feat = np.zeros((F.H, F.W, 8))
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        rc = rtw._lib.rtw_render_features(r.ctx, C.byref(e.cam.raw), C.c_uint64(1), 0, 1, None,
                                          feat.ctypes.data_as(C.c_void_p), None)
        assert rc == _capi.RTW_E_NO_SCENE
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        r.set_scene(F.scene("simple")[0])
        with pytest.raises(rtw.RenderError) as err:
            r.render_features(e.cam, e.seed, 0, 1)
        assert err.value.code == _capi.RTW_E_UNSUPPORTED


# ------------------------------------------------------------------ the CLI
def test_cli_writes_the_albedo_and_normal_guides(tmp_path):
    """rtw <scene> --features PREFIX (Camera::render_features of the C++ mirror):
    the two PPMs are the Python mirror's features through the same writer."""
    import os
    import subprocess
    width, height, spp, seed = 40, 24, 4, 0x5EED0001
    cfg = tmp_path / "Config.toml"
    cfg.write_text(f"[image]\nimage_width = {width}\nimage_height = {height}\nsamples_per_pixel = {spp}\n"
                   "max_depth = 50\n")
    exe = os.path.join(os.path.dirname(_capi.LIB_PATH), "rtw")
    prefix = str(tmp_path / "guide")
    run = subprocess.run([exe, "simple", "--seed", str(seed), "--config", str(cfg), "--out", str(tmp_path / "image.ppm"),
                          "--features", prefix], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    soa, b = rtw.scenes.simple_soa(seed)
    cam = b.with_vfov(40.0).with_aspect_ratio(width / height).with_max_depth(50).with_image_width(width) \
           .with_image_height(height).with_samples_per_pixel(spp).build()
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        feat, _ = r.render_features(cam, seed, 0, spp)
    _, normal, _, _ = rtw.feature_means(feat, spp)
    rtw.write_ppm(str(tmp_path / "want_albedo.ppm"), np.ascontiguousarray(feat[..., :3]), spp)
    shown = (normal + 1.0) / 2.0
    rtw.write_ppm(str(tmp_path / "want_normal.ppm"), np.ascontiguousarray(shown * shown), 1)
    for what in ("albedo", "normal"):
        got, want = (tmp_path / f"guide_{what}.ppm").read_bytes(), (tmp_path / f"want_{what}.ppm").read_bytes()
        assert got == want and len(got) > width * height * 6, what
    assert len(set((tmp_path / "guide_albedo.ppm").read_text().split("\n")[3:])) > 3     # not one flat colour
