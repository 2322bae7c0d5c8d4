"""tests/f32_forms.py is itself right (CPU, no GPU needed).

Its reference-form evaluation (f32_form=False, float64, f64's uniforms) on f64
inputs equals the independent restatement (tests/indep/restate.py, through the
cases of query_cases / nee_cases / path_cases) bit for bit: hit records, the
light list's pdf, light samples and the whole bounce.  The f32-only forms are
held against the reference's forms in f64, the inversion sampler against its
law by chi-square, and the calibration (float32) against the law (float64) on
every case of tests/test_gpu_f32_records.py: it takes another branch on at most
0.25 % of each group."""
import math

import numpy as np
import pytest

import f32_forms as FF
import f32_record_cases as RC
import nee_cases as N
import path_cases as P
import query_cases as Q
from indep import restate as R
from oracle import oracle as O


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_vectorised_xoshiro_is_the_scalar_one():
    pix = np.array([0, 1, 77, 959, 2 ** 31 + 5], np.uint64)
    s = FF.rng_seed(7, pix, 3)
    gs = [R.Rng(7, int(p), 3) for p in pix]
    assert [tuple(map(int, row)) for row in s] == [tuple(g.s) for g in gs]
    mask = np.array([True, False, True, True, False])
    for _ in range(5):
        w = FF.rng_next(s, mask)
        for k, g in enumerate(gs):
            if mask[k]:
                assert int(w[k]) == g.next_u64()
    for n in (1, 3, 19, 64, 1000):
        idx = FF.rng_index(s, n)
        assert [int(i) for i in idx] == [g.gen_index(n) for g in gs]
    assert [tuple(map(int, row)) for row in s] == [tuple(g.s) for g in gs]
    F = FF.Forms(np.float64, False)
    U = FF.Uniforms(F, False)
    w = FF.rng_next(s)
    want = [g.next_u64() for g in gs]
    assert same(U.std(w), [(v >> 11) * 2.0 ** -53 for v in want])
    assert same(U.open01(w), [1.0 + (v >> 12) * 2.0 ** -52 - (1.0 - R.EPS / 2.0) for v in want])
    U32 = FF.Uniforms(FF.Forms(np.float32), True)
    assert same(U32.std(w), [np.float32((v >> 40) * 2.0 ** -24) for v in want])
    assert same(U32.open01(w), [np.float32((v >> 41) * 2.0 ** -23 + 2.0 ** -24) for v in want])
    r = np.linspace(0.0, 1.0, 4001)[:-1]
    sn, cs = FF._sincos_2pi_fdlibm(r)
    ref = [R.sincos_2pi(float(x)) for x in r]
    assert same(sn, [a for a, _ in ref]) and same(cs, [b for _, b in ref])


def restated_hits(soa, rays):
    w = R.World(soa)
    out = []
    for r in rays:
        out.append(w.hit(tuple(map(float, r[:3])), tuple(map(float, r[3:]))))
    return out


@pytest.mark.parametrize("name", ["simple", "cornell_box", "simple_transform", "plane+light"])
def test_reference_form_hit_records_equal_the_restatement(name):
    if name == "plane+light":
        soa, _ = P.scene(name)
        rays = P.hand_placed(name)[0]
    elif name == "simple_transform":        # small cuboids in a wide view: rays aimed at them, not path segments
        soa = Q.scene(name)[0]
        rays = RC.aimed_rays(soa, 400, 3)
    else:
        seg = Q.segments(name)
        rows = np.sort(np.concatenate([np.flatnonzero(seg.ids >= 0)[:300], np.flatnonzero(seg.ids < 0)[:100]]))
        soa, rays = seg.soa, seg.rays[rows]
    S = FF.stage(soa, np.float64)
    got = FF.closest_hit(S, rays, np.float64, f32_form=False, sphere_form="t")
    recs = restated_hits(soa, rays)
    hit = np.array([r is not None for r in recs])
    assert np.array_equal(got["id"] >= 0, hit) and hit.sum() >= 20
    for key, want in (("t", [r.t for r in recs if r]), ("p", [r.p for r in recs if r]),
                      ("normal", [r.normal for r in recs if r]), ("u", [r.u for r in recs if r]),
                      ("v", [r.v for r in recs if r]), ("mat", [r.mat for r in recs if r]),
                      ("front", [int(r.front) for r in recs if r])):
        assert same(got[key][hit], want), (name, key)


@pytest.mark.parametrize("name", ["simple", "lights64", "cornell_box"])
def test_reference_form_light_pdf_equals_the_restatement(name):
    seg = Q.segments(name)
    rays = Q.lambertian_bounces(seg)[:300]
    if name != "cornell_box":
        rays = np.concatenate([rays, Q.rays_at_lights(seg.soa, 2)[:200]])
    S = FF.stage(seg.soa, np.float64)
    got = FF.lights_pdf(S, rays, np.float64, f32_form=False)["pdf"]
    w = R.World(seg.soa)
    want = [w.lights_pdf(tuple(map(float, r[:3])), tuple(map(float, r[3:]))) for r in rays]
    assert same(got, want) and (np.asarray(want) > 0).sum() > 20


@pytest.mark.parametrize("name", ["simple", "lights64", "cornell_box"])
def test_reference_form_light_samples_equal_the_restatement(name):
    soa, pts = N.bounce_points(name)
    d, idx, pdf = N.light_samples(soa, pts, 7, 1000, 3)
    got = FF.light_sample(FF.stage(soa, np.float64), pts, 7, 1000, 3, np.float64, f32_form=False, bits32=False)
    assert np.array_equal(got["index"], idx) and same(got["dir"], d) and same(got["pdf"], pdf)


def records_of(segs):
    """(hits [n, 9], ids [n, 4]) of restated records (path_cases segments); object id 0 for a hit"""
    n = len(segs)
    hits, ids = np.zeros((n, 9)), np.zeros((n, 4), np.int64)
    for k, rec in enumerate(segs):
        if rec is None:
            ids[k, 0] = -1
            continue
        hits[k] = (rec.t, *rec.p, *rec.normal, rec.u, rec.v)
        ids[k] = (0, rec.mat, int(rec.front), 0)
    return hits, ids


def check_bounce(soa, rays, recs, rng0, want):
    S = FF.stage(soa, np.float64)
    hits, ids = records_of(recs)
    got = FF.shade(S, rays, hits, ids, rng0, np.float64, f32_form=False, bits32=False)
    assert np.array_equal(got["event"], want["event"])
    assert np.array_equal(got["what"], want["what"]), [(a, b) for a, b in zip(got["what"], want["what"]) if a != b][:5]
    for key in ("next", "weight", "emitted", "pdfs"):
        assert same(got[key], want[key]), key
    assert np.array_equal(got["state"], want["rng1"])
    return got


@pytest.mark.parametrize("name", ["simple", "cornell_box", "lights64", "plane+light", "perlin_spheres+light"])
def test_reference_form_bounce_equals_the_restatement(name):
    b = P.bounces(name)
    k = slice(0, 500)
    want = dict(event=b.event[k], what=b.what[k], next=b.next[k], weight=b.weight[k], emitted=b.emitted[k],
                pdfs=b.pdfs[k], rng1=b.rng1[k])
    check_bounce(b.soa, b.rays[k], [sg["rec"] for sg in b.segs[k]], b.rng0[k], want)


def test_reference_form_bounce_on_the_hand_made_cases():
    for soa, rays, streams in ((P.textured_lights()[0], *P.textured_lights()[1:]),
                               (P.scene("simple")[0], *P.hand_placed("simple")),
                               (P.scene("plane+light")[0], *P.hand_placed("plane+light"))):
        sh = P.Shader(soa)
        want = P.expect(sh, rays, streams)
        recs = restated_hits(soa, rays)
        check_bounce(soa, rays, recs, want["rng0"], want)


def test_reference_form_camera_rays_equal_the_restatement():
    _, b = Q.scene("simple")
    for angle in (0.0, 0.6):
        cam = O.camera_dict(Q.oracle_cam(b.copy().with_defocus_angle(angle), 64, 40, 2, 5))
        pix = np.arange(0, 64 * 40, 7)
        for s in (0, 1):
            want, rng = P.camera_rays(cam, 7, pix, s)
            got, st = FF.camera_rays(cam, 7, pix, s, np.float64, f32_form=False, bits32=False, store=np.float64)
            assert same(got, want) and np.array_equal(st, rng)


def test_cancellation_free_forms_against_the_reference_forms():
    """x = r^2 / d^2: x / (1 + sqrt(1 - x)) against 1 - sqrt(1 - x) (the pdf), and
    w (2 - w) against 1 - z^2, z = 1 + r1 (cos_max - 1) (sphere_random), all in f64.  From x = 1e-6 the
    relative difference stays below 1e-9 (the reference form carries about 2^-52 / (x / 2)
    <= 4.4e-10 there); down to x = 1e-12 the f32 form follows the series x / 2 + x^2 / 8."""
    F32, F64 = FF.Forms(np.float64, True), FF.Forms(np.float64, False)
    x = np.exp(np.random.default_rng(5).uniform(np.log(1e-6), np.log(0.999), 20000))
    a, b = FF.one_minus_cos_max(F32, x), FF.one_minus_cos_max(F64, x)
    rel = np.abs(a - b) / b
    print(f"1 - cos_max, x in [1e-6, 1): largest relative difference {rel.max():.3e}")
    assert rel.max() < 1e-9
    # (the reference's 1 - z^2 carries about 2^-52 / (x r1 / 4): the bound holds from r1 = 0.1 on; for
    # smaller r1 it is the reference's form that is inaccurate, the f32 form is a plain product)
    r1 = np.random.default_rng(6).uniform(0.1, 1.0, 20000)
    w = r1 * a
    z = 1.0 + r1 * (np.sqrt(1.0 - x) - 1.0)
    s32, s64 = w * (2.0 - w), 1.0 - z * z
    rel = np.abs(s32 - s64) / s32
    print(f"1 - z^2, x in [1e-6, 1), r1 in [0.1, 1]: largest relative difference {rel.max():.3e}")
    assert rel.max() < 1e-9
    x = np.exp(np.random.default_rng(7).uniform(np.log(1e-12), np.log(1e-6), 20000))
    series = x / 2 + x * x / 8
    rel = np.abs(FF.one_minus_cos_max(F32, x) - series) / series
    assert rel.max() < 1e-12
    # the two-pass pdf and Sphere::pdf_value's f32 form are one formula
    c, o = (np.full(3, 0.5), np.full(3, 2.0), np.full(3, -1.0)), (np.zeros(3), np.zeros(3), np.array([0.0, 1.0, 2.0]))
    d = FF.sub(c, o)
    assert same(FF.light_pdf_f32(F32, c, np.float64(0.5), o), FF.sphere_pdf_value(F32, c, np.float64(0.5), o, d)[0])


CHI2_63_1M6 = 131.37         # the 1 - 1e-6 quantile of chi-square(63)


def test_inversion_sampler_law():
    """2^16 points of the f32 form's unit_sphere from the streams (7, k, 0), in f64: all inside
    the ball; |p|^3, p.z / |p| and the azimuth are uniform.  64 bins each, chi-square against
    uniform below the 1 - 1e-6 quantile of chi-square(63).  Deterministic; the statistics
    are |p|^3: 53.8, p.z / |p|: 63.8, azimuth: 55.7."""
    F = FF.Forms(np.float64, True)
    U = FF.Uniforms(F, True)
    n = 1 << 16
    s = FF.rng_seed(7, np.arange(n, dtype=np.uint64), 0)
    p = FF.unit_sphere(F, U, s)
    l = np.sqrt(FF.dot(p, p))
    assert (l < 1.0).all()
    ok = l > 0
    stats = []
    for name, x in (("|p|^3", l ** 3), ("p.z / |p|", (p[2][ok] / l[ok] + 1) / 2),
                    ("azimuth", np.arctan2(p[1][ok], p[0][ok]) / (2 * math.pi) % 1.0)):
        h = np.bincount(np.minimum((x * 64).astype(int), 63), minlength=64)
        e = len(x) / 64
        chi = float(((h - e) ** 2 / e).sum())
        stats.append((name, chi))
        print(f"inversion sampler, {name}: chi-square(63) = {chi:.1f}")
    assert all(chi < CHI2_63_1M6 for _, chi in stats), stats


@pytest.mark.parametrize("group", RC.GROUPS)
def test_calibration_alone_stays_within_the_cap(group):
    """The float32 evaluation against the float64 one, on the rows the GPU test sends: it takes
    another discrete decision on at most 0.25 % of the group (so the kernel's 1 % cap is not
    used up by the inputs), and every such row is near its decision."""
    case = RC.case(group)
    law, cal = case.law(), case.calibration()
    differ, margin_ok = case.disagree(law, cal)
    share = float(differ.mean())
    print(f"{group}: calibration and law decide differently on {int(differ.sum())} of {len(differ)} rows "
          f"({100 * share:.3f} %)")
    assert len(differ) >= case.min_rows
    assert share <= 0.0025
    assert margin_ok[differ].all()
