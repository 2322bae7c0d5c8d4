"""The f32 query kernels' values, record by record, against the law of their
own forms (tests/f32_forms.py evaluated in float64 on the inputs as the f32
kernel sees them), with the allowance taken from the calibration (the same
code in float32, numpy's correctly rounded operations) on the same rows.

For every real-valued output x of a query (a scalar, or a vector taken as a
whole with the inf-norm) the row error is e = |x - law| / max(|law|, floor),
for the kernel's x and for the calibration's.  FLOORS below states the floor
per quantity.  Over a group's compared rows (at least 1000 unless the case
says otherwise):

  * the kernel's p50, p99 and max are each at most 4 x the calibration's
    statistic of the same name on the same rows;
  * the kernel's value is finite where the law's is, NaN / inf where it is;
  * integer outputs are equal.

Why 4: the f32 mode's worst single operation is a * v_rcp(b), one ulp of the
reciprocal plus half of the product against numpy's half ulp -- a factor of 3;
v_sqrt / v_rsq are one ulp against a half; contraction to FMA only removes
roundings.  Rounded up: 4.  The bound is computed at test time from the
calibration; no measured number is stored here.

Decisions.  f32 and the law may take different branches within rounding of a
decision (the nearest object, a silhouette, the front face at grazing
incidence, a cuboid's face, Metal's keep, total internal reflection, Schlick
against the draw, the lights that pass the light test, a checker cell, the
unit disk's rejection).  A row is NEAR A DECISION when one of its margins in
the law (f32_record_cases: |disc| normalised, the gap to the second nearest
object, the distance to a quad's border, |d . n| / |d|, |ratio sin - 1|,
|reflectance - u|, the distance to a checker edge, ||p|^2 - 1|) is at most
4 x the 99th percentile of the calibration's error in that margin over the
group.  A row
whose observable integer outputs differ, or one of whose values is off by more
than GROSS x the calibration's largest error (a branch that shows in no
integer output: which lights counted, reflect or refract), is left out of the
value comparison ONLY when it is near a decision; otherwise it stays in and
fails the bound (values) or the test outright (integers).  At most 1 % of a
group may be left out.  The lobe coin and the list index are exact in both
precisions and are never excluded: they are compared on every row.

Every measured ratio is printed as a line "F32REC {json}"."""
import json

import numpy as np
import pytest

import f32_forms as FF
import f32_record_cases as RC
import ray_tracing_weekend_amd as rtw

pytestmark = pytest.mark.gpu

ALLOW = RC.ALLOW
GROSS = 64.0
CAP = 0.01
# the floor of max(|law|, floor) per quantity: "own": none but the smallest normal number (the
# quantity's own size is its scale: t, a direction's length, a pdf, a colour); 1.0: a component
# of a unit vector and the O(1) surface coordinates (u, v) of spheres, quads and cuboids;
# "origin": a point, the ray origin's (for a bounce: the hit point's) norm; a plane's (u, v)
# are coordinates of the hit point: the larger of 1 and the origin's norm.
FLOORS = {"own": np.finfo(np.float32).tiny}

TRAVERSALS = ((rtw.RTW_ACCEL_BRUTE, {"lds": 1}), (rtw.RTW_ACCEL_BRUTE, {"lds": 0}), (rtw.RTW_ACCEL_BVH, {"bvh_kind": 0}),
              (rtw.RTW_ACCEL_BVH, {"bvh_kind": 1}), (rtw.RTW_ACCEL_BVH, {"bvh_kind": 2}),
              (rtw.RTW_ACCEL_BVH, {"bvh_kind": 3}))


def norm(x, vector):
    x = np.abs(np.asarray(x, np.float64))
    return x.max(1) if vector else x


def row_error(x, law, vector, floor):
    with np.errstate(all="ignore"):
        law = np.asarray(law, np.float64)
        return norm(np.asarray(x, np.float64) - law, vector) / np.maximum(norm(law, vector), floor)


def finite_pattern(x, vector):
    x = np.asarray(x, np.float64)
    nan, inf = np.isnan(x), np.isinf(x)
    return (nan.any(1), inf.any(1)) if vector else (nan, inf)


def judge(group, case, kernel, law=None, cal=None, near=None, min_rows=None):
    """the comparison of the module docstring; returns the report lines"""
    law = case.law() if law is None else law
    cal = case.calibration() if cal is None else cal
    near = case.near_decision() if near is None else near
    n = case.n
    min_rows = case.min_rows if min_rows is None else min_rows
    assert n >= min_rows, (group, n)
    differ = case.differ(law, kernel)
    # a row on which the calibration itself decides otherwise (test_f32_forms_host.py: at most
    # 0.25 %, each near its decision) has no calibration: it counts as left out
    no_cal = case.differ(law, cal)
    errs, gross, pattern_bad = {}, np.zeros(n, bool), np.zeros(n, bool)
    for key, vector, floor_name in case.REALS:
        floor = FLOORS.get(floor_name, case.floor(floor_name))
        ek, ec = row_error(kernel[key], law[key], vector, floor), row_error(cal[key], law[key], vector, floor)
        assert case.valued(key).sum() >= min_rows, (group, key, int(case.valued(key).sum()))
        ok = np.isfinite(norm(law[key], vector)) & case.valued(key)
        kn, ki = finite_pattern(kernel[key], vector)
        ln, li = finite_pattern(law[key], vector)
        pattern_bad |= (kn != ln) | (ki != li)
        # the calibration's own NaN / inf where the law is finite: such a row has no calibration
        # either; it counts as left out and must be near a decision like every other
        lost = ok & ~np.isfinite(ec)
        if lost.any():
            print(f"{group} {key}: the calibration is not finite on {int(lost.sum())} rows where the law is "
                  f"(the kernel on {int((lost & ~np.isfinite(ek)).sum())} of them)")
        no_cal = no_cal | lost
        ok &= ~no_cal
        top = ec[ok].max() if ok.any() else 0.0
        with np.errstate(invalid="ignore"):
            gross |= ok & ~(ek <= GROSS * top)
        errs[key] = (ek, ec, ok)
    stray = differ & ~near
    for row in np.flatnonzero(stray | (pattern_bad & ~near))[:6]:
        print(f"{group} row {row}: far from a decision, kernel / law / calibration:")
        for key in tuple(k for k, _, _ in case.REALS) + tuple(case.INTS):
            print(f"    {key}: {np.asarray(kernel[key])[row]} / {np.asarray(law[key])[row]} / {np.asarray(cal[key])[row]}")
        print(f"    margins {case.margins(law)[row]} thresholds {case.thresholds()}")
    assert not stray.any(), (group, "integer outputs differ far from any decision", np.flatnonzero(stray)[:8].tolist())
    out = near & (differ | gross | pattern_bad | no_cal)
    keep = ~out
    share = float(out.mean())
    lines, failures = [], []
    if share > CAP:
        failures.append(f"{100 * share:.3f} % of the rows left out (cap {100 * CAP:.0f} %)")
    if (no_cal & ~near).any():
        failures.append(f"the calibration decides otherwise far from a decision on rows {np.flatnonzero(no_cal & ~near)[:8].tolist()}")
    if (pattern_bad & keep).any():
        failures.append(f"NaN / inf pattern differs on rows {np.flatnonzero(pattern_bad & keep)[:8].tolist()}")
    for key, (ek, ec, ok) in errs.items():
        rows = keep & ok
        if not rows.any():
            continue
        rec = dict(group=group, quantity=key, rows=int(rows.sum()), excluded=int(out.sum()), near=int(near.sum()))
        for name, q in (("p50", 50), ("p99", 99), ("max", 100)):
            k, c = float(np.percentile(ek[rows], q)), float(np.percentile(ec[rows], q))
            rec[name] = dict(kernel=k, calibration=c, ratio=(k / c if c > 0 else (0.0 if k == 0 else float("inf"))))
            if not k <= ALLOW * c:
                worst = int(np.flatnonzero(rows)[np.argmax(np.nan_to_num(ek[rows], nan=np.inf))])
                failures.append(f"{key} {name}: kernel {k:.3e} > {ALLOW:.0f} x calibration {c:.3e} (worst row {worst}: "
                                f"kernel {np.asarray(kernel[key])[worst]}, law {np.asarray(law[key])[worst]})")
        lines.append(rec)
        print("\nF32REC " + json.dumps(rec))
    assert not failures, (group, failures)
    return lines


def context(soa, robust, accel=rtw.RTW_ACCEL_AUTO, **tuning):
    r = rtw.Renderer(device=0, precision=rtw.RTW_F32)
    r.set_tuning("robust", 1 if robust else 0)
    for k, v in tuning.items():
        r.set_tuning(k, v)
    r.set_accel(accel)
    r.set_scene(soa)
    return r


def hit_dict(hits, ids):
    return dict(t=hits[:, 0], p=hits[:, 1:4], normal=hits[:, 4:7], u=hits[:, 7], v=hits[:, 8], id=ids[:, 0],
                mat=ids[:, 1], front=ids[:, 2], kind=ids[:, 3])


# ------------------------------------------------------------------ hit_rays
@pytest.mark.parametrize("group", list(RC.HIT_GROUPS))
def test_hit_records(group):
    case = RC.case(group)
    robust = case.form == "robust"
    spheres = case.S.n_sph > 0
    law = case.law()
    seen = []
    for accel, tuning in (TRAVERSALS if spheres else TRAVERSALS[:1]):
        with context(case.soa, robust, accel, **tuning) as r:
            k = hit_dict(*r.hit_rays(case.rays))
            if not seen and group in ("hit/poles/u", "hit/cornell_box", "hit/simple/robust"):
                r.set_tuning("query_grid", 1)              # blocks past a workgroup's first: the same answers
                g1 = hit_dict(*r.hit_rays(case.rays))
                assert all(np.array_equal(k[key], g1[key], equal_nan=True) for key in k), group
        if not seen:
            judge(group, case, k)
        seen.append(k)
    # the traversals answer alike wherever each agrees with the law: ids, and t to the bit
    for k in seen[1:]:
        both = (k["id"] == law["id"]) & (seen[0]["id"] == law["id"])
        assert both.mean() >= 1 - 2 * CAP
        for key in ("id", "mat", "front", "kind", "t"):
            assert np.array_equal(k[key][both], seen[0][key][both]), (group, key)


# ----------------------------------------------------------------- light_pdf
@pytest.mark.parametrize("group", list(RC.PDF_GROUPS))
def test_light_pdf(group):
    case = RC.case(group)
    with context(case.soa, case.robust, **case.tuning) as r:
        pdf = r.light_pdf(case.rays)
        st = r.get_query_stats()
        print(f"{group}: light path {st.kernel}")
        if group == "pdf/lights64/grid":
            r.set_tuning("query_grid", 1)
            assert np.array_equal(pdf, r.light_pdf(case.rays), equal_nan=True)
    if group == "pdf/far":
        assert np.isfinite(pdf).all() and (pdf > 0).all()      # where the reference's form gives inf in f32
    if group == "pdf/inside":
        assert np.isnan(pdf).sum() >= 32
    judge(group, case, dict(pdf=pdf))


# -------------------------------------------------------------- light_sample
@pytest.mark.parametrize("group", list(RC.SAMPLE_GROUPS))
def test_light_sample(group):
    case = RC.case(group)
    with context(case.soa, case.robust) as r:
        d, pdf, idx = r.light_sample(case.origins, RC.SEED, case.first_stream, case.sample)
        if group == "sample/lights64":
            r.set_tuning("query_grid", 1)
            d1, p1, i1 = r.light_sample(case.origins, RC.SEED, case.first_stream, case.sample)
            assert np.array_equal(d, d1, equal_nan=True) and np.array_equal(pdf, p1, equal_nan=True)
    law = case.law()
    assert np.array_equal(idx, law["index"])                   # exact in both precisions: every row
    judge(group, case, dict(dir=d, pdf=pdf, index=idx))
    # in the law's arithmetic: a sphere light's direction lies inside its cone, a quad's ends on the quad
    S, o, dd = case.S, case.origins.astype(np.float64), d.astype(np.float64)
    for k, (kind, j) in enumerate(S.lref):
        rows = np.flatnonzero((idx == k) & np.isfinite(dd).all(1))
        if not len(rows):
            continue
        if kind == "sphere":
            to = S.light_c[j][None, :] - o[rows]
            cosv = (dd[rows] * to).sum(1) / np.sqrt((dd[rows] ** 2).sum(1) * (to ** 2).sum(1))
            with np.errstate(invalid="ignore"):
                cos_max = np.sqrt(1.0 - S.light_r[j] ** 2 / (to ** 2).sum(1))
            ok = np.isnan(cos_max) | (cosv >= cos_max - 4 * 2.0 ** -24)
            assert ok.all(), (group, k, float((cos_max - cosv)[~ok].max()))
        elif kind == "quad":
            Qd = S.lquads[j]
            F = FF.Forms(np.float64)
            al, be = FF.quad_uv(F, Qd, FF.sub(FF.v3(o[rows] + dd[rows]), FF.v3(Qd["q"])))
            tol = 4 * 2.0 ** -24 * max(1.0, float(np.abs(o[rows]).max()) / float(np.sqrt(Qd["area"])))
            assert (al >= -tol).all() and (al <= 1 + tol).all() and (be >= -tol).all() and (be <= 1 + tol).all(), group
            off = np.abs(FF.dot(FF.sub(FF.v3(o[rows] + dd[rows]), FF.v3(Qd["q"])), FF.v3(Qd["n"])))
            assert (off <= tol * np.sqrt(Qd["area"])).all(), group


# --------------------------------------------------------------- camera_rays
@pytest.mark.parametrize("group", list(RC.CAMERA_GROUPS))
def test_camera_rays(group):
    case = RC.case(group)
    rays, states = [], []
    with rtw.Renderer(device=0, precision=rtw.RTW_F32) as r:
        for s in (0, 1):
            ry, st = r.camera_rays(case.cam, RC.SEED, s, pixels=case.pixels)
            rays.append(ry)
            states.append(st)
        r.set_tuning("query_grid", 1)
        ry, st = r.camera_rays(case.cam, RC.SEED, 1, pixels=case.pixels)
        assert np.array_equal(ry, rays[1]) and np.array_equal(st, states[1])
    rays = np.concatenate(rays)
    judge(group, case, dict(origin=rays[:, :3], direction=rays[:, 3:], state=np.concatenate(states)))


# ---------------------------------------------------------------- shade_rays
@pytest.fixture(scope="module")
def shaded():
    """every batch through hit_rays and shade_rays of one f32 context each; the law and the
    calibration on the SAME f32 records"""
    batches = RC.shade_batches()
    records, outs = [], []
    for b in batches:
        with context(b.soa, b.robust) as r:
            hits, ids = r.hit_rays(b.rays)
            rng = b.states.copy()
            nxt, weight, emitted, event, pdfs = r.shade_rays(b.rays, hits, ids, rng, pdfs=True)
            if b.name == "simple":
                r.set_tuning("query_grid", 1)
                rng1 = b.states.copy()
                again = r.shade_rays(b.rays, hits, ids, rng1, pdfs=True)
                assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(again, (nxt, weight, emitted, event, pdfs)))
                assert np.array_equal(rng, rng1)
        records.append((hits, ids))
        outs.append(dict(next=nxt, weight=weight, emitted=emitted, event=event, pdfs=pdfs, state=rng,
                         origin=np.sqrt((hits[:, 1:4].astype(np.float64) ** 2).sum(1))))
    _, law, cal = RC.shade_setup(records)
    return batches, law, cal, outs


@pytest.mark.parametrize("group", list(RC.SHADE_GROUPS))
def test_shade_rays(shaded, group):
    batches, law, cal, outs = shaded
    case = RC.SHADE_GROUPS[group]().use(batches, law, cal)
    # the lobe coin and the list index are exact: the state after the draws is equal on every
    # Lambertian row whose other draws are exact too (the index, the two direction words)
    if case.what in ("light sphere", "light quad", "cosine lobe", "diffuse light", "total internal reflection", "metal",
                     "metal absorbed"):
        k = case.pool(outs)
        assert np.array_equal(k["state"], case.law()["state"]), group
    judge(group, case, case.pool(outs))
