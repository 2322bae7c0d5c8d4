"""Every kernel of the query launch path past its workgroups' first block of
rays.  A query, the feature pass and the wavefront rounds launch min(blocks,
resident workgroups) workgroups that walk their blocks of 256 rays grid-stride
(the feature pass: waves that take tiles from a counter); on an MI355X a
workgroup makes a second trip only above half a million rays.  Tuning
"query_grid" caps the grid, so trips 2..k run at the shapes the per-query
references cover: n = 769 (4 blocks, the last with one live lane: three waves
of that workgroup hold no ray on their final trip), 1000 (4 blocks, the last of
232 lanes) and 2049 (9 blocks), at grid 1 and 3 (3 divides neither 4 nor 9).

The case builders and the expectations are the per-query tests' own
(query_cases, nee_cases, path_cases, wavefront_cases, feature_cases: the oracle
and the independent restatement), tiled to n; no expected value comes from the
GPU.  f64 is compared bit for bit with equal NaN masks exactly as each query's
own test compares it; f32 is held to that query's f32 expectation and, in
addition, equals the natural grid's output bit for bit.  Two runs at the
natural grid, of the kernels whose workgroups share state across trips, use
n = 2 * 256 * 8 * CUs + 1 rays: eight 4-wave workgroups per CU is the
occupancy ceiling, so at least one workgroup of the real grid makes a second
trip."""
import functools

import numpy as np
import pytest
import torch

import feature_cases as F
import nee_cases as N
import path_cases as P
import query_cases as Q
import ray_tracing_weekend_amd as rtw
import test_gpu_path_advance as TA
import test_gpu_shade_rays as TS
import test_gpu_wavefront_batched as TW
import wavefront_cases as WC
from oracle import oracle as O
from ray_tracing_weekend_amd import _capi
from test_gpu_features import _counts_inside_tiles, where_differs
from test_gpu_query import expect_records, same
from test_gpu_query_lights import restate_pdf

pytestmark = pytest.mark.gpu

BLOCK = 256                                    # kQueryBlock
NS = (769, 1000, 2049)                         # 4, 4 and 9 blocks
GRIDS = (1, 3)
PRECISIONS = [pytest.param(rtw.RTW_F32, id="f32"), pytest.param(rtw.RTW_F64, id="f64")]
WORLD_OF_KIND = {0: 2, 1: 3, 2: 4, 3: 5}      # rtw_query_stats.kernel of tuning bvh_kind
LINEAR, LIGHT_BVH, GRID, MIXED = 0, 1, 2, 3
# the configuration list of tests/test_gpu_occlusion.py: (what, accel, tuning, world)
WORLDS = [("brute, lds 1", rtw.RTW_ACCEL_BRUTE, {"lds": 1}, 1), ("brute, lds 0", rtw.RTW_ACCEL_BRUTE, {"lds": 0}, 0)]
for _kind in (0, 1, 2, 3):
    for _lds in (0, 1):
        WORLDS.append((f"bvh_kind {_kind}, lds {_lds}", rtw.RTW_ACCEL_BVH, {"bvh_kind": _kind, "lds": _lds},
                       WORLD_OF_KIND[_kind]))
WORLDS.append(("bvh_kind 3, bvh_lds_max 1", rtw.RTW_ACCEL_BVH, {"bvh_kind": 3, "bvh_lds_max": 1}, 3))
WORLD_IDS = [w[0].replace(", ", "-").replace(" ", "_") for w in WORLDS]
# the light paths of tests/test_gpu_query_lights.py and test_gpu_light_sample.py: (scene, tuning, path)
LIGHT_PATHS = [("simple", {}, LINEAR), ("lights64", {}, GRID), ("lights64", {"light_grid": 0}, LIGHT_BVH),
               ("lights64", {"light_bvh_min": 1 << 20}, LINEAR), ("cornell_box", {}, MIXED)]
LIGHT_IDS = ["simple-linear", "lights64-grid", "lights64-light_bvh", "lights64-linear", "cornell_box-mixed"]


def tiled(a, n):
    """the first n rows of `a` repeated"""
    a = np.asarray(a)
    reps = -(-n // len(a))
    return np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:n])


def blocks_of(n):
    return -(-n // BLOCK)


def renderer(soa=None, precision=rtw.RTW_F64, accel=rtw.RTW_ACCEL_AUTO, **tuning):
    r = rtw.Renderer(device=0, precision=precision)
    for k, v in tuning.items():
        r.set_tuning(k, v)
    r.set_accel(accel)
    if soa is not None:
        r.set_scene(soa)
    return r


def natural_n():
    """tests/test_gpu_occlusion.py's bound: at most 8 workgroups of 4 waves are resident per CU,
    so the natural grid has at most 8 * CUs workgroups and this count gives one a second block"""
    return 2 * BLOCK * 8 * torch.cuda.get_device_properties(0).multi_processor_count + 1


def bit_equal(a, b):
    """bit for bit, NaN payloads and the sign of zero included: two runs of one kernel"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


# ------------------------------------------------------------------ the key
def test_the_key_is_clamped_refused_below_zero_and_accepted_on_virtual_ranks():
    lib = rtw._lib
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        assert lib.rtw_set_tuning(r.ctx, b"query_grid", -1) == _capi.RTW_E_INVALID
        with pytest.raises(rtw.RenderError) as e:
            r.set_tuning("query_grid", -1)
        assert e.value.code == _capi.RTW_E_INVALID
        for v in (0, 1, 3, 1 << 20, 1 << 40):             # (a huge value is clamped, as "persist" is)
            r.set_tuning("query_grid", v)
        mult, _, slot = r.path_begin(600)                  # 3 blocks under the clamped cap: the natural grid
        assert slot.cpu().numpy().view(np.uint32).tolist() == list(range(600)) and bool((mult == 1).all())
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        assert lib.rtw_set_tuning(r.ctx, b"query_grid", 3) == _capi.RTW_OK
        assert lib.rtw_set_tuning(r.ctx, b"query_grid", -1) == _capi.RTW_E_INVALID
        soa, b = Q.scene("simple")
        r.set_scene(soa)
        cam = b.copy().with_image_width(24).with_image_height(16).with_samples_per_pixel(2).with_max_depth(6).build()
        capped = r.render(cam, 5)                          # the ranks' renders do not read the key
        r.set_tuning("query_grid", 0)
        assert TW.same(r.render(cam, 5), capped)


# ------------------------------------------------------------- path_advance
def workgroup_blocks_follow_each_other(in_slot, keep, out_slot, grid):
    """At grid G one workgroup takes the blocks g, g + G, ... one after another, each with its
    own atomic on the one count: the survivors of block b lie before those of block b + G
    (of the next block of that workgroup that has any)."""
    where = {int(s): k for k, s in enumerate(out_slot.tolist())}
    first = {}
    for b in range(blocks_of(len(in_slot))):
        rows = np.flatnonzero(keep[b * BLOCK:(b + 1) * BLOCK])
        if len(rows):
            first[b] = where[int(in_slot[b * BLOCK + rows[0]])]
    for g in range(grid):
        mine = [first[b] for b in range(g, blocks_of(len(in_slot)), grid) if b in first]
        if mine != sorted(mine):
            return False
    return True


def advance_at_grids(r, rec, want, want_colour, n_slots, last, grids):
    """the device form at each grid (sentinels behind the count are the kernel's to keep):
    {grid: out-state}"""
    keep = np.isin(rec["slot"], want["slot"])
    out = {}
    for grid in grids:
        r.set_tuning("query_grid", grid)
        got, colour, bufs = TA.run_device(r, rec, n_slots, last)
        TA.check(r, rec, want, want_colour, got, colour, bufs, n_slots)     # stats (6, n, m), sentinels, sorted fields
        if grid == 1:        # one workgroup, the blocks in order: the survivors in input order, no sort
            for f in TA.FIELDS:
                assert WC.same(got[f], want[f]), (f, grid)
        if grid:
            assert workgroup_blocks_follow_each_other(rec["slot"], keep, got["slot"], grid), grid
        out[grid] = got
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["mixed", "go"])
@pytest.mark.parametrize("n", NS)
def test_path_advance_later_trips(precision, kind, n):
    with renderer(None, precision) as r:
        for last in (False, True):
            rec, want, want_colour = TA.case(precision, n, kind, last)
            assert (len(want["slot"]) == 0) == last and (kind != "go" or last or len(want["slot"]) == n)
            out = advance_at_grids(r, rec, want, want_colour, n, last, (0,) + GRIDS)
            for grid in GRIDS:                              # the natural grid's bits, block order aside
                a, b = np.argsort(out[grid]["slot"], kind="stable"), np.argsort(out[0]["slot"], kind="stable")
                for f in TA.FIELDS:
                    assert bit_equal(out[grid][f][a], out[0][f][b]), (f, grid)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_path_begin_later_trips(precision):
    dt = TA.dtype_of(precision)
    with renderer(None, precision) as r:
        r.set_tuning("query_grid", 1)
        mult, res, slot = r.path_begin(2049, first_slot=37)
        assert WC.same(mult.cpu().numpy(), np.ones((2049, 3), dt)) and WC.same(res.cpu().numpy(), np.zeros((2049, 3), dt))
        assert slot.cpu().numpy().view(np.uint32).tolist() == list(range(37, 37 + 2049))


# ----------------------------------------------------------------- hit_rays
def check_hits(hits, ids, st, seg, n, world):
    want_hits, want_ids = (tiled(a, n) for a in expect_records(seg))
    assert st.kernel == world and st.is_light_pdf == 0
    assert np.array_equal(ids, want_ids), np.flatnonzero((ids != want_ids).any(1))[:8]
    assert same(hits[:, 0], want_hits[:, 0])                      # t
    assert same(hits[:, 1:4], want_hits[:, 1:4])                  # p
    assert same(hits[:, 4:7], want_hits[:, 4:7])                  # normal, front-face adjusted
    miss = want_ids[:, 0] < 0
    assert not hits[miss].any()
    assert (st.rays, st.hits) == (n, int((~miss).sum()))


@pytest.mark.parametrize("what,accel,tuning,world", WORLDS, ids=WORLD_IDS)
def test_hit_rays_later_trips(what, accel, tuning, world):
    """"simple" in every world: in world 5 the stealing traversal has real work on every trip,
    and the lanes without a ray of a last block enter it as thieves."""
    seg = Q.segments("simple")
    assert np.array_equal(seg.wid, seg.ids)
    with renderer(seg.soa, accel=accel, **tuning) as r:
        for n in NS:
            rays = tiled(seg.rays, n)
            for grid in GRIDS:
                r.set_tuning("query_grid", grid)
                hits, ids = r.hit_rays(rays)
                check_hits(hits, ids, r.get_query_stats(), seg, n, world)


@functools.lru_cache(maxsize=None)
def camera_ids():
    """(primary rays of `simple`, the object each meets by the oracle): the f32 query's expectation"""
    rays = Q.camera_rays("simple", 60, 40)[:2049]
    sc = O.Scene(**Q.scene("simple")[0].__dict__)
    ids = np.array([O.world_hit(sc, r[:3], r[3:])[0] for r in rays])
    rays.flags.writeable = ids.flags.writeable = False
    return rays, ids


@pytest.mark.parametrize("what,accel,tuning,world", WORLDS, ids=WORLD_IDS)
def test_hit_rays_later_trips_f32(what, accel, tuning, world):
    """The f32 query's own expectation (tests/test_gpu_query_lights.py: at most 1 % of camera rays
    pick another object than f64 -- here the oracle's object), and the natural grid's bits."""
    soa, _ = Q.scene("simple")
    cam, want = camera_ids()
    assert (want >= 0).sum() > 500 and (want < 0).sum() > 100
    with renderer(soa, rtw.RTW_F32, accel, **tuning) as r:
        for n in NS:
            rays = tiled(cam, n).astype(np.float32)
            h0, i0 = r.hit_rays(rays)
            assert r.get_query_stats().kernel == world
            for grid in GRIDS:
                r.set_tuning("query_grid", grid)
                h, i = r.hit_rays(rays)
                st = r.get_query_stats()
                share = float((i[:, 0] != tiled(want, n)).mean())
                assert share <= 0.01, (n, grid, share)
                assert (st.kernel, st.rays, st.hits) == (world, n, int((i[:, 0] >= 0).sum()))
                assert bit_equal(h, h0) and np.array_equal(i, i0), (n, grid)
            r.set_tuning("query_grid", 0)


# ----------------------------------------------------------------- occluded
@pytest.mark.parametrize("what,accel,tuning,world", WORLDS, ids=WORLD_IDS)
def test_occluded_later_trips(what, accel, tuning, world):
    soa, rays, t_max, want = N.mixed_batch("simple")
    with renderer(soa, accel=accel, **tuning) as r:
        for n in NS:
            rr, tm, ww = tiled(rays, n), tiled(t_max, n), tiled(want, n)
            for grid in GRIDS:
                r.set_tuning("query_grid", grid)
                occ = r.occluded(rr, tm)
                st = r.get_query_stats()
                assert np.array_equal(occ, ww), (n, grid, np.flatnonzero(occ != ww)[:8])
                assert (st.kernel, st.is_light_pdf, st.rays, st.hits) == (world, 2, n, int(ww.sum()))


@pytest.mark.parametrize("name", ["cornell_box", "simple_transform"])
def test_occluded_later_trips_quads_and_cuboids(name):
    soa, rays, t_max, want = N.mixed_batch(name)
    with renderer(soa) as r:
        for n in NS:
            rr, tm, ww = tiled(rays, n), tiled(t_max, n), tiled(want, n)
            for grid in GRIDS:
                r.set_tuning("query_grid", grid)
                occ = r.occluded(rr, tm)
                st = r.get_query_stats()
                assert np.array_equal(occ, ww), (n, grid, np.flatnonzero(occ != ww)[:8])
                assert st.kernel in (0, 1) and (st.rays, st.hits) == (n, int(ww.sum()))


@functools.lru_cache(maxsize=None)
def camera_truth():
    """(primary rays of `simple`, hit mask, t -- 1 for a miss) by the oracle: the f64 truth the
    f32 any-hit answers are held to"""
    rays, _ = camera_ids()
    sc = O.Scene(**Q.scene("simple")[0].__dict__)
    rec = [O.world_hit(sc, r[:3], r[3:])[:2] for r in rays]
    hit = np.array([k >= 0 for k, _ in rec])
    t = np.array([float(t) if k >= 0 else 1.0 for k, t in rec])
    hit.flags.writeable = t.flags.writeable = False
    return rays, hit, t


@pytest.mark.parametrize("what,accel,tuning,world", WORLDS, ids=WORLD_IDS)
def test_occluded_later_trips_f32(what, accel, tuning, world):
    """tests/test_gpu_nee_f32.py's expectations at every capped grid: "occluded within t_max" is
    "the f32 closest hit of the same context is at t32 <= t_max" at t_max = t32 and just below it,
    exactly; against the f64 truth (here the oracle's) at t / 2 and 2 t at most 1 % of the rays
    differ.  In addition the answers are the natural grid's bytes."""
    soa, _ = Q.scene("simple")
    cam, hit64, t64 = camera_truth()
    assert hit64.sum() > 500 and (~hit64).sum() > 100
    with renderer(soa, rtw.RTW_F32, accel, **tuning) as r:
        for n in NS:
            rays = tiled(cam, n).astype(np.float32)
            half_t, twice_t = tiled(t64 / 2, n).astype(np.float32), tiled(2 * t64, n).astype(np.float32)
            truth = tiled(hit64, n).astype(np.uint8)
            r.set_tuning("query_grid", 0)
            natural = (r.occluded(rays, half_t), r.occluded(rays, twice_t), r.occluded(rays))
            for grid in GRIDS:
                r.set_tuning("query_grid", grid)
                h32, i32 = r.hit_rays(rays)
                hit = i32[:, 0] >= 0
                t32 = np.where(hit, h32[:, 0], np.float32(1.0)).astype(np.float32)
                at = r.occluded(rays, t32)
                st = r.get_query_stats()
                assert (st.kernel, st.is_light_pdf, st.rays, st.hits) == (world, 2, n, int(hit.sum())), (n, grid)
                assert np.array_equal(at, hit.astype(np.uint8)), (n, grid)       # t32 <= t_max at t_max = t32 ...
                assert not r.occluded(rays, np.nextafter(t32, np.float32(-np.inf))).any(), (n, grid)   # ... nothing nearer
                half, twice, inf = r.occluded(rays, half_t), r.occluded(rays, twice_t), r.occluded(rays)
                assert np.array_equal(inf, hit.astype(np.uint8)), (n, grid)
                for name, got, want in (("t / 2", half, np.zeros_like(truth)), ("2 t", twice, truth), ("inf", inf, truth)):
                    share = float((got != want).mean())
                    assert share <= 0.01, (name, n, grid, share)
                for got, first in zip((half, twice, inf), natural):
                    assert np.array_equal(got, first), (n, grid)


def test_occluded_later_trips_f32_mixed_upper_ends_equal_the_natural_grid():
    """A supplement to the test above on rays whose neighbours carry different kinds of t_max
    (path segments; f32 has no bound against f64 at t_max = t itself): the natural grid's bytes."""
    soa, rays, t_max, _ = N.mixed_batch("simple")
    with renderer(soa, rtw.RTW_F32) as r:
        for n in NS:
            rr, tm = tiled(rays, n).astype(np.float32), tiled(t_max, n).astype(np.float32)
            occ0 = r.occluded(rr, tm)
            for grid in GRIDS:
                r.set_tuning("query_grid", grid)
                assert np.array_equal(r.occluded(rr, tm), occ0), (n, grid)
                assert r.get_query_stats().rays == n
            r.set_tuning("query_grid", 0)


# ---------------------------------------------------------------- light_pdf
@functools.lru_cache(maxsize=None)
def pdf_case(name):
    """(soa, rays, the restatement's pdf): the rays of tests/test_gpu_query_lights.py, thinned"""
    soa, _ = Q.scene(name)
    if name == "lights64":
        rays = np.concatenate([Q.lambertian_bounces(Q.segments("simple"))[:150], Q.camera_rays("simple63", 40, 24)[::8],
                               Q.rays_at_lights(soa)])
    else:
        rays = Q.lambertian_bounces(Q.segments(name))[:400]
    rays = np.ascontiguousarray(rays)
    want = restate_pdf(soa, rays)
    rays.flags.writeable = want.flags.writeable = False
    return soa, rays, want


@pytest.mark.parametrize("name,tuning,path", LIGHT_PATHS, ids=LIGHT_IDS)
def test_light_pdf_later_trips(name, tuning, path):
    soa, rays, want = pdf_case(name)
    assert len(rays) >= 100 and (want > 0).sum() >= 5
    with renderer(soa, **tuning) as r:
        for n in NS:
            rr, ww = tiled(rays, n), tiled(want, n)
            for grid in GRIDS:
                r.set_tuning("query_grid", grid)
                pdf = r.light_pdf(rr)
                st = r.get_query_stats()
                assert (st.kernel, st.is_light_pdf, st.rays) == (path, 1, n)
                assert same(pdf, ww), (n, grid, np.flatnonzero(~((pdf == ww) | (np.isnan(pdf) & np.isnan(ww))))[:8])
                if name == "simple":
                    assert st.light_tests == n * 19
    with renderer(soa, rtw.RTW_F32, **tuning) as r:     # f32: the speed mode's values, no bound exists (the
        rr = tiled(rays, 2049).astype(np.float32)       # existing f32 test asserts none): the natural grid's bits
        p0 = r.light_pdf(rr)
        assert r.get_query_stats().kernel == path and (p0 > 0).any()
        for grid in GRIDS:
            r.set_tuning("query_grid", grid)
            assert bit_equal(r.light_pdf(rr), p0), grid


# ------------------------------------------------------------- light_sample
SAMPLE_SEED, FIRST_STREAM, SAMPLE_INDEX = 11, (1 << 33) + 40, 2


@functools.lru_cache(maxsize=None)
def sample_case(name):
    """(soa, 2049 origins, (directions, list indices, pdf) of the restatement): row k draws from
    the stream FIRST_STREAM + k, so a shorter batch's expectation is a prefix"""
    if name == "lights64":
        soa, _ = Q.scene("lights64")
        pts = np.concatenate([N.bounce_points("simple")[1][:120], Q.rays_at_lights(soa, 1)[:, :3]])
    else:
        soa, pts = N.bounce_points(name)
    pts = tiled(pts, max(NS))
    want = N.light_samples(soa, pts, SAMPLE_SEED, FIRST_STREAM, SAMPLE_INDEX)
    for a in (pts, *want):
        a.flags.writeable = False
    return soa, pts, want


@pytest.mark.parametrize("name,tuning,path", LIGHT_PATHS, ids=LIGHT_IDS)
def test_light_sample_later_trips(name, tuning, path):
    """The origins repeat, the streams do not: a later trip must draw from first_stream + k of
    its own k."""
    soa, pts, (want_d, want_i, want_p) = sample_case(name)
    assert len(set(want_i.tolist())) > 1
    with renderer(soa, **tuning) as r:
        for n in NS:
            for grid in GRIDS:
                r.set_tuning("query_grid", grid)
                d, p, light = r.light_sample(pts[:n], SAMPLE_SEED, FIRST_STREAM, SAMPLE_INDEX)
                st = r.get_query_stats()
                assert (st.kernel, st.is_light_pdf, st.rays) == (path, 3, n)
                assert np.array_equal(light, want_i[:n]), (n, grid)
                assert same(d, want_d[:n]), (n, grid, np.flatnonzero(~((d == want_d[:n]) | np.isnan(d)).all(1))[:8])
                assert same(p, want_p[:n]), (n, grid)
    # f32, tests/test_gpu_nee_f32.py's expectations: the list index is an integer draw and equals the
    # restatement's exactly (so a later trip draws from first_stream + k), the fused pdf is the f32
    # light pdf of {origin, direction} of the same context bit for bit; and the natural grid's bits
    with renderer(soa, rtw.RTW_F32, **tuning) as r:
        o32 = pts.astype(np.float32)
        d0, p0, l0 = r.light_sample(o32, SAMPLE_SEED, FIRST_STREAM, SAMPLE_INDEX)
        assert r.get_query_stats().kernel == path and np.array_equal(l0, want_i)
        for grid in GRIDS:
            r.set_tuning("query_grid", grid)
            for n in NS:
                d, p, light = r.light_sample(o32[:n], SAMPLE_SEED, FIRST_STREAM, SAMPLE_INDEX)
                st = r.get_query_stats()
                assert (st.kernel, st.is_light_pdf, st.rays) == (path, 3, n)
                assert light.dtype == np.int32 and np.array_equal(light, want_i[:n]), (n, grid)
                alone = r.light_pdf(np.concatenate([o32[:n], d], 1))
                assert p.dtype == np.float32 and np.array_equal(p, alone, equal_nan=True), (n, grid)
                assert bit_equal(d, d0[:n]) and bit_equal(p, p0[:n]), (n, grid)
                dn, pn, ln = r.light_sample(o32[:n], SAMPLE_SEED, FIRST_STREAM, SAMPLE_INDEX, pdf=False)
                assert pn is None and bit_equal(dn, d) and np.array_equal(ln, light), (n, grid)


# -------------------------------------------------------------- camera_rays
CW, CH = 64, 40                                # 2560 pixels: 2049 consecutive ones fit


@functools.lru_cache(maxsize=None)
def camera_case(name, sample):
    cam, ocam = F.cameras(name, CW, CH)
    rays, rng = P.camera_rays(O.camera_dict(ocam), P.SEED, range(CW * CH), sample)
    rays.flags.writeable = rng.flags.writeable = False
    return cam, rays, rng


@pytest.mark.parametrize("name", ["simple", "simple_defocus"])
def test_camera_rays_later_trips(name):
    from test_gpu_camera_rays import same as same_rays
    sample = 3
    cam, want_rays, want_rng = camera_case(name, sample)
    pix = np.random.default_rng(5).integers(0, CW * CH, max(NS))
    pix[7] = pix[3] = pix[2048] = CW * CH - 1
    with renderer(None) as r:
        for n in NS:
            for grid in GRIDS:
                r.set_tuning("query_grid", grid)
                rays, rng = r.camera_rays(cam, P.SEED, sample, first_pixel=300, n=n)       # consecutive pixels
                st = r.get_query_stats()
                assert (st.is_light_pdf, st.rays) == (4, n)
                assert same_rays(rays, want_rays[300:300 + n]) and np.array_equal(rng, want_rng[300:300 + n]), (n, grid)
                rays, rng = r.camera_rays(cam, P.SEED, sample, pixels=pix[:n])               # a list with repeats
                assert same_rays(rays, want_rays[pix[:n]]) and np.array_equal(rng, want_rng[pix[:n]]), (n, grid)
    with renderer(None, rtw.RTW_F32) as r:              # f32: test_gpu_camera_rays.py's bound, the natural grid's bits
        r0, g0 = r.camera_rays(cam, P.SEED, sample, first_pixel=300, n=2049)
        l0, lg0 = r.camera_rays(cam, P.SEED, sample, pixels=pix)
        if name == "simple":                            # (no defocus: two words in both precisions)
            assert np.abs(r0 - want_rays[300:300 + 2049]).max() < 1e-4
            assert np.array_equal(g0, want_rng[300:300 + 2049])
        for grid in GRIDS:
            r.set_tuning("query_grid", grid)
            rr, gg = r.camera_rays(cam, P.SEED, sample, first_pixel=300, n=2049)
            assert bit_equal(rr, r0) and np.array_equal(gg, g0), grid
            rr, gg = r.camera_rays(cam, P.SEED, sample, pixels=pix)
            assert bit_equal(rr, l0) and np.array_equal(gg, lg0), grid


# --------------------------------------------------------------- shade_rays
SHADE_PATHS = [("simple", {}, LINEAR), ("cornell_box", {}, MIXED), ("lights64", {}, GRID),
               ("lights64", {"light_grid": 0}, LIGHT_BVH)]


@pytest.mark.parametrize("name,tuning,path", SHADE_PATHS, ids=["simple-linear", "cornell_box-mixed", "lights64-grid",
                                                              "lights64-light_bvh"])
def test_shade_rays_later_trips(name, tuning, path):
    """The segments of the oracle's paths (second and later segments start on surfaces), with and
    without pdfs; the RNG state out is the restatement's."""
    b = P.bounces(name)
    assert (b.event == P.SCATTER).any() and len(b.rays) >= 200
    with renderer(b.soa, **tuning) as r:
        for n in NS:
            rays, rng0 = tiled(b.rays, n), tiled(b.rng0, n)
            want = {f: tiled(getattr(b, f), n) for f in TS.FIELDS + ("rng1",)}
            for grid in GRIDS:
                r.set_tuning("query_grid", grid)
                got = TS.shade(r, rays, rng0)
                st = r.get_query_stats()
                TS.check(got, want)
                assert (st.is_light_pdf, st.rays, st.kernel) == (5, n, path)
                assert st.hits == int((want["event"] >= P.REFLECT).sum())
                off = TS.shade(r, rays, rng0, pdfs=False)
                assert off["pdfs"] is None
                TS.check(dict(off, pdfs=got["pdfs"]), want)
    keep = ~np.isnan(b.rays).any(1)
    # f32, test_f32_events_without_a_draw_and_the_light_pdf's expectations in full: the events without a
    # draw are exact from the material kind, the light list's pdf of a SCATTER row is light_pdf of
    # {p, direction}; and the natural grid's bits
    with renderer(b.soa, rtw.RTW_F32, **tuning) as r:
        rays = tiled(b.rays[keep], 2049).astype(np.float32)
        rng0 = tiled(b.rng0[keep], 2049)
        hits, ids = r.hit_rays(rays)
        first = None
        for grid in (0,) + GRIDS:
            r.set_tuning("query_grid", grid)
            rng = rng0.copy()
            out = r.shade_rays(rays, hits, ids, rng, pdfs=True)
            event = out[3]
            mtype = np.asarray(b.soa.mat_type)[ids[:, 1]]
            hit = ids[:, 0] >= 0
            assert (event[~hit] == P.MISS).all() and np.array_equal(rng[~hit], rng0[~hit])
            assert (event[hit & (mtype == rtw.RTW_LAMBERTIAN)] == P.SCATTER).all()
            assert (event[hit & (mtype == rtw.RTW_DIELECTRIC)] == P.REFLECT).all()
            assert (event[hit & ((mtype == rtw.RTW_DIFFUSE_LIGHT) | (mtype == rtw.RTW_INVISIBLE))] == P.ABSORBED).all()
            assert np.isin(event[hit & (mtype == rtw.RTW_METAL)], (P.ABSORBED, P.REFLECT)).all()
            nxt, pdfs = out[0], out[4]
            assert nxt.dtype == np.float32 and pdfs.dtype == np.float32
            sc = event == P.SCATTER
            assert sc.sum() >= 20
            assert TS.same(pdfs[sc, 1], r.light_pdf(np.ascontiguousarray(nxt[sc])))     # of the same context and grid
            if first is None:
                first = (out, rng)
            else:
                assert all(bit_equal(a, c) for a, c in zip(out, first[0])) and np.array_equal(rng, first[1]), grid


# ------------------------------------------------- render_wavefront_batched
@pytest.mark.parametrize("name", ["simple", "cornell_box"])
def test_wavefront_driver_on_one_workgroup(name):
    """40 x 24 x 4 spp at grid 1: path_fold walks 12 blocks in one workgroup, and every round's
    camera rays, begin, closest hit, bounce and advance run on later trips."""
    ref, loop, segments, lambertian = TW.references(name)
    soa, _ = Q.scene(name)
    cam = TW.camera(name)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_chunk(1)
        r.set_scene(soa)
        r.set_tuning("query_grid", 1)
        for batch in (0, 3):
            got = r.render_wavefront_batched(cam, TW.SEED, batch=batch)
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            assert np.array_equal(TW.bits(got), TW.bits(ref)), (batch, int((TW.bits(got) != TW.bits(ref)).sum()))
            assert TW.same(got, loop)
            st = r.get_query_stats()
            assert (st.is_light_pdf, st.rays, st.hits) == (7, segments, lambertian), batch
    _, loop32, _, _ = TW.references(name, rtw.RTW_F32)
    with rtw.Renderer(device=0, precision=rtw.RTW_F32) as r:
        r.set_chunk(1)
        r.set_scene(soa)
        natural = r.render_wavefront_batched(cam, TW.SEED, batch=3)
        r.set_tuning("query_grid", 1)
        for batch in (0, 3):
            got = r.render_wavefront_batched(cam, TW.SEED, batch=batch)
            assert TW.same(got, loop32), batch                 # test_f32_is_the_host_loops_f32's expectation
            assert bit_equal(got, natural), batch


# ---------------------------------------------------------- render_features
@pytest.mark.parametrize("name,worlds", [("simple", (5,)), ("cornell_box", (0, 1))])
@pytest.mark.parametrize("width,height,n_samples", [(F.W, F.H, F.SAMPLES), (9, 17, 2), (17, 25, 2)],
                         ids=["40x24", "9x17", "17x25"])
def test_feature_waves_take_several_tiles(name, worlds, width, height, n_samples):
    """Grid 1 and 2: 4 or 8 waves share 15 tiles (40 x 24), 6 (9 x 17: second tiles at grid 1 only)
    or 12 (17 x 25: second tiles at both grids); at the last two sizes the last tile column is one
    pixel wide and the last row one pixel high, so a wave takes a tile after one partly outside the
    image; under the counts it takes one after a tile whose lanes ran different trip counts."""
    e = F.samples(name, width, height, n_samples)
    want = e.fold(0, n_samples)
    jj, ii = np.mgrid[0:height, 0:width]
    counts = _counts_inside_tiles() if (width, height) == (F.W, F.H) else ((3 * ii + 5 * jj) % (n_samples + 1)).astype(np.uint32)
    assert len(np.unique(counts[:8, :8])) == n_samples + 1
    want_c = e.fold(0, n_samples, counts=counts)
    with renderer(F.scene(name)[0]) as r:
        for grid in (1, 2):
            r.set_tuning("query_grid", grid)
            feat, ids = r.render_features(e.cam, e.seed, 0, n_samples)
            st = r.get_query_stats()
            assert st.kernel in worlds and st.is_light_pdf == 0
            assert np.array_equal(ids, e.ids()), (grid, np.argwhere(ids != e.ids())[:6].tolist())
            assert F.same(feat, want), (grid, where_differs(feat, want))
            assert (st.rays, st.hits) == (height * width * n_samples, int(want[..., 7].sum()))
            feat, ids = r.render_features(e.cam, e.seed, 0, n_samples, counts=counts)
            st = r.get_query_stats()
            assert F.same(feat, want_c), (grid, where_differs(feat, want_c))
            assert np.array_equal(ids, e.ids(counts=counts))
            assert st.rays == int(np.minimum(counts, n_samples).sum()) and st.hits == int(want_c[..., 7].sum())
    with renderer(F.scene(name)[0], rtw.RTW_F32) as r:   # f32: no bound can be derived (test_gpu_features.py): the
        f0, i0 = r.render_features(e.cam, e.seed, 0, n_samples)       # natural grid's bits
        c0, _ = r.render_features(e.cam, e.seed, 0, n_samples, counts=counts)
        for grid in (1, 2):
            r.set_tuning("query_grid", grid)
            f, i = r.render_features(e.cam, e.seed, 0, n_samples)
            assert bit_equal(f, f0) and np.array_equal(i, i0), grid
            assert r.get_query_stats().rays == height * width * n_samples
            assert bit_equal(r.render_features(e.cam, e.seed, 0, n_samples, counts=counts)[0], c0), grid


# --------------------------------------------------------- the natural grid
def test_path_advance_at_the_natural_grid():
    """f64, "mixed": the 1000-row case tiled past the resident grid, every copy with slots of its
    own, so at least one workgroup reuses s_wave / s_base for a second block."""
    n = natural_n()
    base = WC.records(1000, np.float64, "mixed", seed=1001)
    rec = {k: tiled(v, n) for k, v in base.items()}
    rec["slot"] = (rec["slot"] + np.uint32(1000) * (np.arange(n, dtype=np.uint32) // np.uint32(1000))).astype(np.uint32)
    n_slots = 1000 * -(-n // 1000)
    assert len(np.unique(rec["slot"])) == n and int(rec["slot"].max()) < n_slots
    want, want_colour = WC.advance(rec, np.full((n_slots, 3), WC.SENTINEL), TA.BG)
    assert 0 < len(want["slot"]) < n
    print(f"path_advance at the natural grid: {n} paths in {blocks_of(n)} blocks, {len(want['slot'])} survivors")
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        got, colour, bufs = TA.run_device(r, rec, n_slots)
        TA.check(r, rec, want, want_colour, got, colour, bufs, n_slots)     # with WC.blocks_keep_their_order


def test_hit_rays_world_5_at_the_natural_grid():
    n = natural_n()
    seg = Q.segments("simple")
    with renderer(seg.soa) as r:
        hits, ids = r.hit_rays(tiled(seg.rays, n))
        st = r.get_query_stats()
        check_hits(hits, ids, st, seg, n, 5)
        print(f"hit_rays at the natural grid: {n} rays in {blocks_of(n)} blocks, {st.hits} hits, {st.kernel_ms:.2f} ms")


# ---------------------------------------------------------------- isolation
def test_the_cap_changes_no_render_and_leaves_nothing_behind():
    soa, b = Q.scene("simple")
    cam = b.copy().with_image_width(32).with_image_height(24).with_samples_per_pixel(16).with_max_depth(12).build()
    seg = Q.segments("simple")
    rays = tiled(seg.rays, 1000)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        first = r.render(cam, 5)
        stats = (r.stats.segments, r.stats.kernel)
        kernel = r.last_kernel()
        h0, i0 = r.hit_rays(rays)
        q0 = r.get_query_stats()
        r.set_tuning("query_grid", 3)
        capped = r.render(cam, 5)                          # a render under the cap: the same launch
        assert (r.stats.segments, r.stats.kernel) == stats and r.last_kernel() == kernel
        h1, i1 = r.hit_rays(rays)
        q1 = r.get_query_stats()
        r.set_tuning("query_grid", 0)
        again = r.render(cam, 5)
        assert (r.stats.segments, r.stats.kernel) == stats and r.last_kernel() == kernel
        h2, i2 = r.hit_rays(rays)
        q2 = r.get_query_stats()
    assert TW.same(first, capped) and TW.same(first, again)
    assert bit_equal(h0, h1) and bit_equal(h0, h2) and np.array_equal(i0, i1) and np.array_equal(i0, i2)
    assert np.array_equal(i0[:, 0], tiled(seg.ids, 1000))
    for q in (q1, q2):
        assert (q.kernel, q.rays, q.hits) == (q0.kernel, q0.rays, q0.hits)
