"""The material bounce (rtw_shade_rays) on the GPU in f64, bit for bit against
the independent restatement's own pieces (tests/path_cases.py: the unrolled
loop of restate.trace_sample): over the segments of query_cases.segments(name)
every output and the RNG state, through every light path; the branches the
cases must reach; batch tails; MISS rows; pdfs off; device and host entries;
a render before and after; the refusals; and f32.

The two named scenes whose light list is empty while they hold a Lambertian
material (perlin_spheres, plane) are refused with RTW_E_NO_LIGHTS, as the
header states: the reference panics there, and no restatement exists.  Their
materials go through the bounce with a light list added (path_cases.LIT_NAMES).
Bit for bit is meant literally: the sign of zero is compared."""
import numpy as np
import pytest

import path_cases as P
import query_cases as Q
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

LINEAR, LIGHT_BVH, GRID, MIXED = 0, 1, 2, 3
SHADE = 5                                      # rtw_query_stats.is_light_pdf
BLOCK = 256                                    # kQueryBlock
FIELDS = ("event", "emitted", "weight", "next", "pdfs")


def bits(a):
    """the values' bit patterns, every NaN as the one pattern of all ones (payloads aside)"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    u = a.view(np.uint64 if a.dtype == np.float64 else np.uint32).copy()
    u[np.isnan(a)] = ~u.dtype.type(0)
    return u


def same(a, b):
    """bit for bit, the sign of zero included; NaN masks equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


def shade(r, rays, rng0, pdfs=True):
    """dict of shade_rays' outputs for these rays, hit by the same context; rng1 the states after"""
    hits, ids = r.hit_rays(rays)
    rng = np.array(rng0, np.uint64)
    out = r.shade_rays(rays, hits, ids, rng, pdfs=pdfs)
    got = dict(zip(("next", "weight", "emitted", "event"), out[:4]), rng1=rng, hits=hits, ids=ids)
    got["pdfs"] = out[4] if pdfs else None
    return got


def check(got, want, rows=slice(None)):
    """every field of the bounce and the state after it, bit for bit (same())"""
    for f in FIELDS + ("rng1",):
        w = getattr(want, f)[rows] if not isinstance(want, dict) else want[f][rows]
        g = got[f]
        assert g.shape == w.shape and g.dtype == w.dtype, (f, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.flatnonzero((bits(g) != bits(w)).reshape(len(w), int(np.prod(w.shape[1:]))).any(1))
        assert len(bad) == 0, (f, bad[:8], g[bad[:2]], w[bad[:2]])


def renderer(soa, precision=rtw.RTW_F64, **tuning):
    r = rtw.Renderer(device=0, precision=precision)
    for k, v in tuning.items():
        r.set_tuning(k, v)
    r.set_scene(soa)
    return r


PATH_OF = {"cornell_box": MIXED, "simple_light": MIXED, "simple_transform": MIXED, "lights64": GRID}


@pytest.mark.parametrize("name", P.NAMES + P.LIT_NAMES)
def test_every_output_and_the_rng_state_are_the_restatements(name):
    b = P.bounces(name)
    if name in P.NAMES:
        assert same(b.rays, Q.segments(name).rays)   # the unrolled paths are the oracle's segments
    with renderer(b.soa) as r:
        got = shade(r, b.rays, b.rng0)
        st = r.get_query_stats()
        check(got, b)
        assert got["event"].dtype == np.int32
        assert (st.is_light_pdf, st.rays, st.kernel) == (SHADE, len(b.rays), PATH_OF.get(name, LINEAR))
        assert st.hits == int((b.event >= P.REFLECT).sum())
        # MISS rows leave their state untouched and are all zero
        miss = b.event == P.MISS
        assert np.array_equal(got["rng1"][miss], b.rng0[miss])
        for f in ("next", "weight", "emitted", "pdfs"):
            assert not got[f][miss].any()
        assert not got["pdfs"][b.event != P.SCATTER].any()
        # the light list's pdf is rtw_light_pdf_rays of {p, direction}
        sc = b.event == P.SCATTER
        if sc.any():
            assert same(got["pdfs"][sc, 1], r.light_pdf(got["next"][sc]))
        # pdfs off changes nothing else
        off = shade(r, b.rays, b.rng0, pdfs=False)
        assert off["pdfs"] is None
        for f in ("event", "emitted", "weight", "next", "rng1"):
            assert same(off[f], got[f])


def test_the_cases_reach_every_branch_on_the_gpu():
    """Each branch the bounce has occurs at least once in what the tests above
    compared, or in the hand-placed rays compared here."""
    seen = {}
    for name in P.NAMES:
        b = P.bounces(name)
        for w in set(b.what.tolist()):
            seen[w] = seen.get(w, 0) + int((b.what == w).sum())
    b = P.bounces("simple")
    rays, streams = P.hand_placed("simple")
    want = P.expect(b.shader, rays, streams)
    with renderer(b.soa) as r:
        got = shade(r, rays, want["rng0"])
    check(got, want)
    for w in set(want["what"].tolist()):
        seen[w] = seen.get(w, 0) + int((want["what"] == w).sum())
    for what in ("miss", "metal", "metal absorbed", "total internal reflection", "schlick reflection", "refraction",
                 "cosine lobe", "light sphere", "light quad", "light default", "diffuse light"):
        assert seen.get(what, 0) > 0, (what, seen)
    # total internal reflection draws no word
    tir = want["what"] == "total internal reflection"
    assert tir.any() and np.array_equal(got["rng1"][tir], want["rng0"][tir])
    # all four events; textures on both textured materials; a cuboid with its object-space
    # normal and UV; a back face
    events, tex, kinds, back = set(), set(), set(), 0
    for name in P.NAMES:
        b = P.bounces(name)
        events |= set(b.event.tolist())
        tex |= set(zip(b.mtype.tolist(), b.tex.tolist()))
        back += int((~b.front).sum())
        seg = Q.segments(name)
        kinds |= set(seg.kind[seg.ids[seg.ids >= 0]].tolist())
    assert events == {P.MISS, P.ABSORBED, P.REFLECT, P.SCATTER}
    L, D = rtw.RTW_LAMBERTIAN, rtw.RTW_DIFFUSE_LIGHT
    _, t_rays, t_streams = P.textured_lights()   # (compared in test_textured_emitters_and_the_one_sided_plane)
    t_want = P.expect(P.Shader(P.textured_lights()[0]), t_rays, t_streams)
    tex |= set(zip(t_want["mtype"].tolist(), t_want["tex"].tolist()))
    assert {(L, 0), (L, 1), (L, 2), (D, 0), (D, 1), (D, 2)} <= tex, tex
    assert _capi.RTW_PRIM_CUBOID in kinds and back > 0


def test_textured_emitters_and_the_one_sided_plane():
    """DiffuseLight with a Checker and a Noise texture (no named scene holds one): the
    hand-made scene of path_cases.textured_lights; and the checkered plane of `plane`,
    met from below, with a light list added."""
    soa, rays, streams = P.textured_lights()
    want = P.expect(P.Shader(soa), rays, streams)
    D, L = rtw.RTW_DIFFUSE_LIGHT, rtw.RTW_LAMBERTIAN
    kinds = set(zip(want["mtype"].tolist(), want["tex"].tolist()))
    assert {(D, 0), (D, 1), (D, 2), (L, 1)} <= kinds, kinds
    for tex in (1, 2):                         # many different colours are emitted, all ABSORBED
        rows = (want["mtype"] == D) & (want["tex"] == tex)
        assert rows.sum() >= 20 and (want["event"][rows] == P.ABSORBED).all()
        assert len(np.unique(want["emitted"][rows], axis=0)) >= (2 if tex == 1 else 20)
    with renderer(soa) as r:
        got = shade(r, rays, want["rng0"])
    check(got, want)
    assert np.array_equal(got["rng1"][want["mtype"] == D], want["rng0"][want["mtype"] == D])   # an emitter draws nothing
    b = P.bounces("plane+light")
    rays, streams = P.hand_placed("plane+light")
    want = P.expect(b.shader, rays, streams)
    assert (want["event"] == P.SCATTER).all() and not want["front"].any() and (want["tex"] == 1).all()
    assert len(np.unique(want["next"][:, :3], axis=0)) == len(rays)
    with renderer(b.soa) as r:
        got = shade(r, rays, want["rng0"])
    check(got, want)


def lambertian_rows(b):
    return b.event == P.SCATTER


def test_light_paths_give_identical_bits():
    """lights64 through the grid, the light BVH and the linear list; the mixed list
    is cornell_box's and simple_light's only path (checked against the restatement above)."""
    b = P.bounces("lights64")
    got = {}
    for what, tuning, path in (("grid", {}, GRID), ("light BVH", {"light_grid": 0}, LIGHT_BVH),
                               ("linear", {"light_bvh_min": 1 << 20}, LINEAR)):
        with renderer(b.soa, **tuning) as r:
            got[what] = shade(r, b.rays, b.rng0)
            st = r.get_query_stats()
            assert (st.kernel, st.is_light_pdf) == (path, SHADE), what
            assert st.light_tests > 0
        check(got[what], b)
    rows = lambertian_rows(b)
    assert rows.sum() >= 50
    for what in ("grid", "light BVH"):
        for f in FIELDS + ("rng1",):
            assert same(got[what][f][rows], got["linear"][f][rows]), (what, f)


def test_bvh_leaf_light_list():
    soa, _ = Q.scene("simple")
    leaf = Q.with_lights(soa, soa.lights[:5], flags=rtw.RTW_LIGHTS_BVH_LEAF)
    sh = P.Shader(leaf)
    b = P.bounces("simple")
    rows = np.flatnonzero(b.event == P.SCATTER)[:120]
    # the same incoming rays and states on the scene with the leaf-form list
    want = P.expect_from_states(sh, b.rays[rows], b.rng0[rows])
    with renderer(leaf) as r:
        got = shade(r, b.rays[rows], b.rng0[rows])
        assert r.get_query_stats().kernel == LINEAR
    check(got, want)
    assert (want["pdfs"][:, 1] > 0).any()


@pytest.mark.parametrize("n", [0, 1, 63, 65, BLOCK + 1])
def test_batch_tails(n):
    b = P.bounces("simple")
    assert len(b.rays) > BLOCK + 1
    with renderer(b.soa) as r:
        got = shade(r, b.rays[:n], b.rng0[:n])
    assert got["event"].shape == (n,) and got["next"].shape == (n, 6)
    check(got, b, slice(0, n))


def test_device_and_host_entries_are_identical_and_a_render_is_unchanged():
    import torch
    b = P.bounces("cornell_box")
    soa, builder = Q.scene("cornell_box")
    cam = builder.copy().with_image_width(40).with_image_height(24).with_samples_per_pixel(2).with_max_depth(8).build()
    with renderer(b.soa) as r:
        before = r.render(cam, 7)
        got = shade(r, b.rays, b.rng0)
        t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")   # noqa: E731
        t_rng = t(b.rng0.view(np.int64))
        out = r.shade_rays(t(b.rays), t(got["hits"]), t(got["ids"]), t_rng, pdfs=True)
        for f, o in zip(("next", "weight", "emitted", "event", "pdfs"), out):
            assert o.is_cuda and same(o.cpu().numpy(), got[f]), f
        assert np.array_equal(t_rng.cpu().numpy().view(np.uint64), got["rng1"])
        # row slices are as good as whole arrays: each record keeps the alignment it needs
        pad = lambda a: t(np.concatenate([np.zeros_like(a[:1]), a]))[1:]   # noqa: E731
        s_rng = pad(b.rng0.view(np.int64))
        assert s_rng.data_ptr() % 16 == 0 and pad(got["hits"]).data_ptr() % 16 == 8
        out = r.shade_rays(pad(b.rays), pad(got["hits"]), pad(got["ids"]), s_rng, pdfs=True)
        for f, o in zip(("next", "weight", "emitted", "event", "pdfs"), out):
            assert same(o.cpu().numpy(), got[f]), f
        assert np.array_equal(s_rng.cpu().numpy().view(np.uint64), got["rng1"])
        after = r.render(cam, 7)
    assert same(before, after)


def test_four_zero_words_draw_from_the_stream_of_0_0_0():
    """Zeros are no xoshiro256++ state; the header gives such a row the stream of
    (seed 0, pixel 0, sample 0): the restatement's bounce from that state."""
    b = P.bounces("simple")
    rows = np.flatnonzero(b.event != P.MISS)[:100]
    assert (b.mtype[rows] == rtw.RTW_METAL).any() and (b.mtype[rows] == rtw.RTW_LAMBERTIAN).any()
    start = np.tile(np.array(P.R.Rng(0, 0, 0).s, np.uint64), (len(rows), 1))
    want = P.expect_from_states(b.shader, b.rays[rows], start)
    with renderer(b.soa) as r:
        got = shade(r, b.rays[rows], np.zeros((len(rows), 4), np.uint64))
    check(got, want)


def test_refusals():
    b = P.bounces("cornell_box")
    rays, rng = b.rays[:4], np.array(b.rng0[:4])
    hits, ids = np.zeros((4, 9)), np.full((4, 4), -1, np.int32)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:           # no scene
        with pytest.raises(rtw.RenderError) as e:
            r.shade_rays(rays, hits, ids, rng)
        assert e.value.code == _capi.RTW_E_NO_SCENE
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        r.set_scene(b.soa)
        with pytest.raises(rtw.RenderError) as e:
            r.shade_rays(rays, hits, ids, rng)
        assert e.value.code == _capi.RTW_E_UNSUPPORTED
    for name in P.NO_LIGHTS:                   # an empty light list with a Lambertian material
        soa, _ = Q.scene(name)
        assert len(soa.lights) == 0 and (np.asarray(soa.mat_type) == rtw.RTW_LAMBERTIAN).any()
        with renderer(soa) as r:
            with pytest.raises(rtw.RenderError) as e:
                r.shade_rays(rays, hits, ids, rng)
            assert e.value.code == _capi.RTW_E_NO_LIGHTS
    with renderer(b.soa) as r:                 # wrong shapes and dtypes never reach the library
        with pytest.raises(rtw.RenderError):
            r.shade_rays(rays, hits[:3], ids, rng)
        with pytest.raises(rtw.RenderError):
            r.shade_rays(rays, hits, ids, rng.astype(np.int64))


def test_f32_events_without_a_draw_and_the_light_pdf():
    """f32: the events that involve no draw are exact from the material kind of
    ids; the answers are deterministic from call to call; the light list's pdf of a
    SCATTER row is light_pdf of {p, direction} of the same context bit for bit.
    The values of every branch (directions, weights, pdfs, texture colours, the state
    after the draws) are held to the law of the f32 forms in
    tests/test_gpu_f32_records.py (test_shade_rays)."""
    for name in ("simple", "cornell_box", "lights64"):
        b = P.bounces(name)
        rays = b.rays[~np.isnan(b.rays).any(1)].astype(np.float32)
        rng0 = np.array(b.rng0[~np.isnan(b.rays).any(1)])
        with renderer(b.soa, rtw.RTW_F32) as r:
            hits, ids = r.hit_rays(rays)
            rng = rng0.copy()
            nxt, weight, emitted, event, pdfs = r.shade_rays(rays, hits, ids, rng, pdfs=True)
            rng2 = rng0.copy()
            again = r.shade_rays(rays, hits, ids, rng2, pdfs=True)
            for a, c in zip((nxt, weight, emitted, event, pdfs), again):
                assert same(a, c)
            assert np.array_equal(rng, rng2)
            assert nxt.dtype == np.float32 and pdfs.dtype == np.float32
            mtype = np.asarray(b.soa.mat_type)[ids[:, 1]]
            hit = ids[:, 0] >= 0
            assert (event[~hit] == P.MISS).all() and np.array_equal(rng[~hit], rng0[~hit])
            assert (event[hit & (mtype == rtw.RTW_LAMBERTIAN)] == P.SCATTER).all()
            assert (event[hit & (mtype == rtw.RTW_DIELECTRIC)] == P.REFLECT).all()
            assert (event[hit & ((mtype == rtw.RTW_DIFFUSE_LIGHT) | (mtype == rtw.RTW_INVISIBLE))] == P.ABSORBED).all()
            assert np.isin(event[hit & (mtype == rtw.RTW_METAL)], (P.ABSORBED, P.REFLECT)).all()
            sc = event == P.SCATTER
            assert sc.sum() >= 20
            assert same(pdfs[sc, 1], r.light_pdf(np.ascontiguousarray(nxt[sc])))
