"""Direct lighting as one query (rtw_direct_light) on the GPU.

f64: the sample records, the ids and the sums bit for bit against the case
file (tests/direct_cases.py: the independent restatement's lights_random,
lights_pdf, list hit and colour, with the scattering pdf, the term and the fold
restated in Python floats), and against the composition of the existing queries
on the same context (light_sample, hit_rays, shade_rays' emitted); every light
path and every world give the same bits; calls compose over first_stream and
first_sample; blocks past a workgroup's first; the zero-normal rule; a closed
form; the refusals; the torch device entry; render_direct.

f32: the same identities with the f32 context's own queries bit for bit, the
fold exact, and spdf / term held to f64 numpy on the widened f32 record fields:
|d spdf| <= 2^-19 absolute (normalise, dot and / pi are at most about 16
roundings of values <= 1), |d term| <= 2^-21 relative (one multiply and one
reciprocal-based divide)."""
import ctypes as C

import numpy as np
import pytest

import direct_cases as D
import query_cases as Q
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

LINEAR, LIGHT_BVH, GRID, MIXED = 0, 1, 2, 3
DIRECT_LIGHT = 8                              # rtw_query_stats.is_light_pdf
WORLD_OF_KIND = {0: 2, 1: 3, 2: 4, 3: 5}      # rtw_query_stats.kernel of tuning bvh_kind
WORLDS = [("brute, lds 1", rtw.RTW_ACCEL_BRUTE, {"lds": 1}, 1), ("brute, lds 0", rtw.RTW_ACCEL_BRUTE, {"lds": 0}, 0)] + \
         [(f"bvh_kind {k}", rtw.RTW_ACCEL_BVH, {"bvh_kind": k}, WORLD_OF_KIND[k]) for k in range(4)]


def same(a, b):
    """bit for bit up to the sign of zero, NaN masks equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def rows_off(a, b):
    a, b = np.asarray(a), np.asarray(b)
    ok = (a == b) | (np.isnan(a) & np.isnan(b))
    return np.flatnonzero(~ok.reshape(len(a), -1).all(1))[:8]


def context(soa, precision=rtw.RTW_F64, accel=None, **tuning):
    r = rtw.Renderer(device=0, precision=precision)
    if accel is not None:
        r.set_accel(accel)
    for k, v in tuning.items():
        r.set_tuning(k, v)
    r.set_scene(soa)
    return r


def identities(r, pts, seed, S, direct, samples, ids, first_stream=0, first_sample=0, direct0=None):
    """the record against the context's own queries: {d, pdf, light} == light_sample, {t, ids}
    == hit_rays({p, d}), Le == shade_rays' emitted, direct == the sequential f64 fold of the
    term columns"""
    dt = samples.dtype
    pts = np.asarray(pts, dt)
    n = len(pts)
    live = np.flatnonzero((pts[:, 3:6] != 0).any(1))
    for j in range(S):
        rows = live * S + j
        if len(live) == n:
            d, p, light = r.light_sample(np.ascontiguousarray(pts[:, :3]), seed, first_stream, first_sample + j)
        else:   # (light_sample's stream is first_stream + its own row: one call per live row)
            d, p, light = (np.concatenate(x) for x in zip(*[
                r.light_sample(pts[k:k + 1, :3], seed, first_stream + int(k), first_sample + j) for k in live]))
        assert same(samples[rows, 0:3], d), ("d", j, rows_off(samples[rows, 0:3], d))
        assert same(samples[rows, 3], p), ("pdf", j, rows_off(samples[rows, 3], p))
        assert np.array_equal(ids[rows, 0], light), ("light", j)
        rays = np.ascontiguousarray(np.concatenate([pts[live, :3], samples[rows, 0:3]], 1))
        hits, hid = r.hit_rays(rays)
        assert same(samples[rows, 4], hits[:, 0]), ("t", j, rows_off(samples[rows, 4], hits[:, 0]))
        assert np.array_equal(ids[rows, 1], hid[:, 0]) and np.array_equal(ids[rows, 2], hid[:, 1]), ("ids", j)
        rng = np.ones((len(rows), 4), np.uint64)
        emitted = r.shade_rays(rays, hits, hid, rng)[2]
        assert same(samples[rows, 6:9], emitted), ("Le", j, rows_off(samples[rows, 6:9], emitted))
    base = np.zeros((n, 3)) if direct0 is None else direct0
    assert same(direct, D.fold(base, samples[:, 9:12].astype(np.float64), ids[:, 3], S)), "fold"
    # a term is added exactly where there is a hit, pdf > 0 and spdf > 0
    with np.errstate(invalid="ignore"):
        adds = (ids[:, 1] >= 0) & (samples[:, 3] > 0) & (samples[:, 5] > 0)
    assert np.array_equal(ids[:, 3] != 0, adds)
    assert not samples[~adds, 9:12].any()


# ------------------------------------------------------------------- f64
@pytest.mark.parametrize("name", list(D.CASES))
def test_f64_records_ids_and_sums_are_the_case_files(name):
    soa, pts, S, exp = D.case(name)
    path = {"cornell_box": MIXED, "simple_light": MIXED, "checker": MIXED, "simple": LINEAR,
            "lights64_emissive": GRID}[name]
    with context(soa) as r:
        direct, samples, ids = r.direct_light(pts, D.SEED, S, records=True)
        st = r.get_query_stats()
        assert st.is_light_pdf == DIRECT_LIGHT and st.rays == len(pts) * S and st.hits == int(exp.ids[:, 3].sum())
        assert direct.dtype == np.float64 and samples.dtype == np.float64 and ids.dtype == np.int32
        assert np.array_equal(ids, exp.ids), rows_off(ids, exp.ids)
        for what, lo, hi in (("d", 0, 3), ("pdf", 3, 4), ("t", 4, 5), ("spdf", 5, 6), ("Le", 6, 9), ("term", 9, 12)):
            assert same(samples[:, lo:hi], exp.samples[:, lo:hi]), (what, rows_off(samples[:, lo:hi],
                                                                                 exp.samples[:, lo:hi]))
        assert same(direct, exp.direct), rows_off(direct, exp.direct)
        assert same(r.direct_light(pts, D.SEED, S), direct)          # without records: the same sums
        identities(r, pts, D.SEED, S, direct, samples, ids)
        # the plan's light path ran: the pdf is that path's (light_tests are its walk's)
        r.light_sample(pts[:, :3], D.SEED)
        assert r.get_query_stats().kernel == path


def test_f64_grid_light_bvh_and_linear_list_give_identical_bits():
    soa, pts, S, exp = D.case("lights64_emissive")
    for what, tuning, path in (("grid", {}, GRID), ("light BVH", {"light_grid": 0}, LIGHT_BVH),
                               ("linear", {"light_bvh_min": 1 << 20}, LINEAR)):
        with context(soa, **tuning) as r:
            direct, samples, ids = r.direct_light(pts, D.SEED, S, records=True)
            assert same(samples, exp.samples) and np.array_equal(ids, exp.ids) and same(direct, exp.direct), what
            r.light_sample(pts[:, :3], D.SEED)
            assert r.get_query_stats().kernel == path, what


@pytest.mark.parametrize("what,accel,tuning,world", WORLDS, ids=[w[0] for w in WORLDS])
def test_f64_every_world_gives_identical_bits(what, accel, tuning, world):
    # (scenes::simple runs the world asked for; with 64 lights the f64 plan keeps the tree of
    # bvh_kind 3 out of LDS, and cornell_box has one sphere: there only the bits are compared)
    for name in ("simple", "lights64_emissive", "cornell_box"):
        soa, pts, S, exp = D.case(name)
        with context(soa, accel=accel, **tuning) as r:
            direct, samples, ids = r.direct_light(pts, D.SEED, S, records=True)
            assert name != "simple" or r.get_query_stats().kernel == world
            assert same(samples, exp.samples) and np.array_equal(ids, exp.ids) and same(direct, exp.direct), name


def test_f64_calls_compose_over_streams_and_sample_windows():
    soa, pts, S, exp = D.case("cornell_box")
    assert S == 4
    with context(soa) as r:
        a, h = 1000, 77
        whole = r.direct_light(pts, D.SEED, S, first_stream=a, records=True)
        d0 = r.direct_light(pts[:h], D.SEED, S, first_stream=a, records=True)
        d1 = r.direct_light(pts[h:], D.SEED, S, first_stream=a + h, records=True)
        for x, y0, y1 in zip(whole, d0, d1):
            assert same(np.concatenate([y0, y1]), x)
        assert not same(whole[0], exp.direct)                        # (another stream, another answer)
        # sample windows: (0, 2) then (2, 2) continued == S = 4
        w0 = r.direct_light(pts, D.SEED, 2)
        w1 = r.direct_light(pts, D.SEED, 2, first_sample=2, direct=w0.copy())
        assert same(w1, exp.direct) and not same(w0, exp.direct)
        # a 64-bit first_stream
        big = (1 << 40) + 3
        want = D.Expected(soa, pts[:40], D.SEED, 2, first_stream=big, first_sample=1)
        direct, samples, ids = r.direct_light(pts[:40], D.SEED, 2, first_stream=big, first_sample=1, records=True)
        assert same(samples, want.samples) and np.array_equal(ids, want.ids) and same(direct, want.direct)


@pytest.mark.parametrize("grid,S", [(1, 1), (2, 3)])
def test_f64_blocks_past_a_workgroups_first_and_a_ragged_tail(grid, S):
    soa, pts, _, _ = D.case("cornell_box")
    tiled = np.ascontiguousarray(np.tile(pts, (4, 1)))
    assert len(tiled) == 652 and len(tiled) % 64 and len(tiled) > 2 * 256
    want = D.Expected(soa, tiled, D.SEED, S, first_stream=5)
    assert not same(want.direct[:163], want.direct[163:326])         # distinct streams per tile
    for what, accel, tuning, world in (WORLDS[0], WORLDS[5]):
        with context(soa, accel=accel, query_grid=grid, **tuning) as r:
            direct, samples, ids = r.direct_light(tiled, D.SEED, S, first_stream=5, records=True)
            assert same(samples, want.samples) and np.array_equal(ids, want.ids) and same(direct, want.direct), what


def test_f64_a_zero_normal_row_between_live_rows_is_skipped():
    soa, pts, S, exp = D.case("cornell_box")
    p = pts[:64].copy()
    dead = [3, 17, 40]
    p[dead, 3:6] = 0.0
    p[17, 3] = -0.0                                                  # (-0 is 0)
    start = np.arange(64 * 3, dtype=np.float64).reshape(64, 3) + 0.5
    want = D.Expected(soa, p, D.SEED, S, direct=start)
    with context(soa) as r:
        direct, samples, ids = r.direct_light(p, D.SEED, S, direct=start.copy(), records=True)
        assert same(direct, want.direct) and same(samples, want.samples) and np.array_equal(ids, want.ids)
        assert same(direct[dead], start[dead]) and not same(direct, start)
        for k in dead:
            assert not samples[k * S:(k + 1) * S].any()
            assert (ids[k * S:(k + 1) * S] == [0, -1, 0, 0]).all()
        assert r.get_query_stats().rays == (64 - len(dead)) * S
        # without accumulate the skipped rows keep what the caller's array held: zeros here
        fresh = r.direct_light(p, D.SEED, S)
        assert not fresh[dead].any()
        live = np.setdiff1d(np.arange(64), dead)
        assert same(fresh[live], exp.direct[live])


def test_f64_closed_form_and_its_occluded_twin():
    soa, exp = D.closed_form(False)
    with context(soa) as r:
        direct, samples, ids = r.direct_light(D.CLOSED_POINT, D.SEED, D.CLOSED_S, records=True)
    assert same(direct, exp.direct) and same(samples, exp.samples) and np.array_equal(ids, exp.ids)
    lo, hi = D.CLOSED_TERM_RANGE
    assert (ids[:, 3] == 1).all() and (samples[:, 9] >= lo * (1 - 1e-12)).all() and \
        (samples[:, 9] <= hi * (1 + 1e-12)).all()
    mean = direct[0] / D.CLOSED_S
    print("closed form: mean", mean, "expected", D.CLOSED_EXPECT, "bound", D.CLOSED_BOUND)
    assert (np.abs(mean - D.CLOSED_EXPECT) <= D.CLOSED_BOUND).all()
    soa, exp = D.closed_form(True)
    with context(soa) as r:
        direct, samples, ids = r.direct_light(D.CLOSED_POINT, D.SEED, D.CLOSED_S, records=True)
    assert same(samples, exp.samples) and np.array_equal(ids, exp.ids)
    assert (direct == 0.0).all() and (ids[:, 1] == 1).all() and (samples[:, 3] > 0).all()


def test_f64_an_origin_inside_a_sphere_light_adds_nothing():
    soa, _, _, _ = D.case("lights64_emissive")
    L = np.asarray(soa.lights).reshape(-1, 4)[:8]
    pts = np.ascontiguousarray(np.concatenate([L[:, :3] + 0.25 * L[:, 3:4], np.tile([0.0, 1.0, 0.0], (8, 1))], 1))
    one = Q.with_lights(soa, L[:1])                                   # every draw is light 0
    with context(one) as r:
        direct, samples, ids = r.direct_light(pts[:1], D.SEED, 4, records=True)
        assert np.isnan(samples[:, 0:3]).all()                        # the reference's NaN direction
        assert not direct.any() and not ids[:, 3].any() and (ids[:, 1] == -1).all()
        assert not samples[:, 9:12].any()
        identities(r, pts[:1], D.SEED, 4, direct, samples, ids)
    with context(soa) as r:
        direct, samples, ids = r.direct_light(pts, D.SEED, 4, records=True)
        identities(r, pts, D.SEED, 4, direct, samples, ids)
        assert np.isfinite(direct).all()


def test_refusals():
    soa, pts, S, _ = D.case("cornell_box")
    lib, inv = rtw._lib, _capi.RTW_E_INVALID
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    p8 = np.ascontiguousarray(pts[:8])
    direct, samples, ids = np.zeros((8, 3)), np.zeros((16, 12)), np.zeros((16, 4), np.int32)
    with context(soa) as r:
        with pytest.raises(rtw.RenderError) as e:
            r.direct_light(p8, 1, 0)
        assert e.value.code == inv                                   # n_samples = 0
        with pytest.raises(rtw.RenderError) as e:
            r.direct_light(p8, 1, 1, t_min=-1.0)
        assert e.value.code == inv
        assert lib.rtw_direct_light(r.ctx, None, 8, 1, 0, 0, 2, 0.0, 0, vp(direct), None, None) == inv
        assert lib.rtw_direct_light(r.ctx, vp(p8), 8, 1, 0, 0, 2, 0.0, 0, None, None, None) == inv
        assert lib.rtw_direct_light(r.ctx, None, 0, 1, 0, 0, 2, 0.0, 0, None, None, None) == _capi.RTW_OK
        # n * S over 2^32 with records: refused before anything is read
        assert lib.rtw_direct_light(r.ctx, vp(p8), 1 << 31, 1, 0, 0, 4, 0.0, 0, vp(direct), vp(samples), None) == inv
        # the device form: short and misaligned buffers (host pointers: refused before any is read)
        dev = lambda *a: lib.rtw_direct_light_device(r.ctx, *a, None)   # noqa: E731
        ok_args = [vp(p8), p8.nbytes, 8, 1, 0, 0, 2, 0.0, 0, vp(direct), direct.nbytes, vp(samples), samples.nbytes,
                   vp(ids), ids.nbytes]
        for at, short in ((1, p8.nbytes - 1), (10, direct.nbytes - 1), (12, samples.nbytes - 1), (14, ids.nbytes - 1)):
            a = list(ok_args)
            a[at] = short
            assert dev(*a) == inv, at
        big = np.zeros(16 * 12 + 2)
        mis = big.ctypes.data + (8 if big.ctypes.data % 16 == 0 else 0)   # 8 B off a 16 B boundary
        a = list(ok_args)
        a[11], a[12] = C.c_void_p(mis), samples.nbytes
        assert mis % 16 == 8 and dev(*a) == inv
        a = list(ok_args)
        a[0] = C.c_void_p(mis)
        assert dev(*a) == inv                                         # f64 points: 16 B
    with context(Q.with_lights(D.case("simple")[0], np.zeros((0, 4)))) as r:
        with pytest.raises(rtw.RenderError) as e:
            r.direct_light(p8, 1, 1)
        assert e.value.code == inv                                   # an empty light list
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        with pytest.raises(rtw.RenderError) as e:
            r.direct_light(p8, 1, 1)
        assert e.value.code == _capi.RTW_E_NO_SCENE
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        r.set_scene(soa)
        with pytest.raises(rtw.RenderError) as e:
            r.direct_light(p8, 1, 1)
        assert e.value.code == _capi.RTW_E_UNSUPPORTED


@pytest.mark.parametrize("precision", [rtw.RTW_F64, rtw.RTW_F32], ids=["f64", "f32"])
def test_torch_device_entry_is_the_host_entry(precision):
    import torch
    soa, pts, S, _ = D.case("cornell_box")
    dt = np.float32 if precision == rtw.RTW_F32 else np.float64
    p = np.asarray(pts, dt)
    with context(soa, precision=precision) as r:
        host = r.direct_light(p, D.SEED, S, first_stream=3, records=True)
        t = torch.as_tensor(p, device="cuda:0")
        dev = r.direct_light(t, D.SEED, S, first_stream=3, records=True)
        assert all(x.is_cuda for x in dev) and dev[0].dtype == torch.float64
        for h, d in zip(host, dev):
            assert same(h, d.cpu().numpy())
        # continued on the device: (0, 2) then (2, 2) == S = 4
        w = r.direct_light(t, D.SEED, 2, first_stream=3)
        w2 = r.direct_light(t, D.SEED, 2, first_stream=3, first_sample=2, direct=w)
        assert w2 is w and same(w.cpu().numpy(), host[0])


def test_render_direct_is_its_own_composition():
    soa, b = Q.scene("cornell_box")
    cam = b.copy().with_image_width(40).with_image_height(24).with_samples_per_pixel(2).with_max_depth(4).build()
    seed, ls = 21, 2
    with context(soa) as r:
        got = r.render_direct(cam, seed, light_samples=ls)
        direct = np.zeros((40 * 24, 3))
        for s in range(2):
            rays, _ = r.camera_rays(cam, seed, s)
            hits, ids = r.hit_rays(rays)
            pts = np.ascontiguousarray(hits[:, 1:7])
            before = direct.copy()
            direct = r.direct_light(pts, seed ^ 0x9E3779B97F4A7C15, ls, 0, s * ls, direct=direct)
            miss = ids[:, 0] < 0
            assert same(direct[miss], before[miss])                  # miss rows: skipped by the zero-normal rule
        assert got.shape == (24, 40, 3) and got.dtype == np.float64 and same(got.reshape(-1, 3), direct)
        assert (got > 0).any(-1).sum() >= 200 and np.isfinite(got).all()
        # windows compose: sample 0, then sample 1 continued
        w = r.render_direct(cam, seed, light_samples=ls, first_sample=0, n_samples=1)
        w = r.render_direct(cam, seed, light_samples=ls, first_sample=1, n_samples=1, sums=w)
        assert same(w, got)


# ------------------------------------------------------------------- f32
@pytest.mark.parametrize("name", ["cornell_box", "simple_light", "lights64_emissive", "checker"])
def test_f32_identities_fold_and_the_value_bounds(name):
    soa, pts, S, exp = D.case(name)
    p32 = np.asarray(pts, np.float32)
    with context(soa, precision=rtw.RTW_F32) as r:
        direct, samples, ids = r.direct_light(p32, D.SEED, S, records=True)
        assert samples.dtype == np.float32 and direct.dtype == np.float64
        identities(r, p32, D.SEED, S, direct, samples, ids)          # bit for bit, the fold exact
        st = r.get_query_stats()
    assert np.array_equal(ids[:, 0], exp.ids[:, 0])                  # the light index is f64's
    w = samples.astype(np.float64)
    nrm = np.repeat(p32[:, 3:6].astype(np.float64), S, 0)
    d = w[:, 0:3]
    with np.errstate(invalid="ignore", divide="ignore"):
        spdf = np.maximum((nrm * (d / np.sqrt((d * d).sum(1))[:, None])).sum(1) / np.pi, 0.0)
        e_spdf = np.abs(w[:, 5] - spdf)
        adds = ids[:, 3] != 0
        term = w[adds, 6:9] * w[adds, 5:6] / w[adds, 3:4]
        e_term = np.abs(w[adds, 9:12] - term) / np.where(term != 0, np.abs(term), 1.0)
    print(f"{name} f32: max |d spdf| {e_spdf.max():.3e} (bound {2.0 ** -19:.3e}), "
          f"max rel |d term| {e_term.max() if e_term.size else 0.0:.3e} (bound {2.0 ** -21:.3e}), "
          f"{int(adds.sum())} terms")
    assert adds.sum() >= 30
    assert e_spdf.max() <= 2.0 ** -19
    assert e_term.max() <= 2.0 ** -21
