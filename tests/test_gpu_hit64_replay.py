"""The f32 render's f64 hit-point path (kOptHit64), pinned transition by transition.

A module fixture builds render_f32.hip with -DRTW_TRACE=f32 (the Makefile's own
rule and flags, rtw_probes.hpp), links it with the product's other objects into
a variant librtw.so under pytest's tmp dir and runs ONE child process
(tests/hit64_trace_child.py) that renders every variant of tests/hit64_cases.py
with 64 pixels traced and writes one .npz.  tests/hit64_replay.py then replays
every traced sample: each check takes segment k as traced and predicts segment
k + 1 or the sample's end.  If the child fails, no test of this module runs.

Exact, bit for bit (f64, the reference's operation order, no FMA): the own
sphere's re-hit t and its refusal, the winner's t (sphere_t_ref64, plane_t_ref64,
the f32 t where the f64 test misses), the hit point as the next origin, the
Dielectric direction on either face with its Open01 word drawn only when
refraction is possible, Metal with fuzz 0, dither64 on every direction that came
through it, the sphere carried as the ray's own, every termination and every
sample's segment count.

Under the 4 x rule (the kernel's error against the law at p50,
p99 and max within 4 x a correctly rounded evaluation's of the same form):
the Lambertian direction (law: mixture_direction in np.longdouble; calibration:
the same in f64 without FMA -- the kernel's unit contracts, see `lambertian`
below) and fuzzy Metal's unit-ball offset (law: the f32 form in f64 on the
24-bit uniforms; calibration: the form in f32).

The object picked equals the f64 brute force's, except rows within rounding of
a decision: the two candidates' f64 t closer than 4 x the p99 of the f32
calibration's error in t over the group; at most 1 % of a group.

Every quantity goes to profiles/hit64_replay.jsonl (profiles/hit64_replay_pytest_gpu.txt
is this file's run with -s, kept by hand as profiles/f32_records_pytest_gpu.txt is).

Set RTW_HIT64_TRACE_LIB to a prebuilt trace library to judge it instead (the
mutants of CHANGELOG.md are run this way: profiles/hit64_replay_mutants.txt).
"""
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import hit64_cases as hc
import hit64_replay as hr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
BUILD = os.path.join(ROOT, "ray_tracing_weekend_amd", "build")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PROFILE = os.path.join(ROOT, "profiles", "hit64_replay.jsonl")
MIN_ROWS, MAX_OUT = 1000, 0.01

GROUPS = [
    "own-sphere re-hit taken", "own-sphere re-hit refused", "other sphere", "plane", "termination: miss",
    "dielectric refract front", "dielectric refract back", "dielectric Schlick reflect front",
    "dielectric Schlick reflect back", "dielectric TIR front", "dielectric TIR back",
    "metal fuzz 0", "metal fuzz > 0", "termination: metal absorbed",
    "lambertian to light sphere", "lambertian cosine sphere", "lambertian to light plane", "lambertian cosine plane",
    "termination: depth exhausted", "stash round trip (to)", "stash round trip (cosine)",
]


def build_trace_lib(tmp):
    """the RTW_TRACE=f32 variant of librtw.so: render_f32.hip by the Makefile's rule
    (its flags, the define appended to the compiler), the other objects the product's"""
    def make(*args):
        return subprocess.run(["make", "-s", "-j16", "-C", CSRC, *args], check=True, capture_output=True, text=True,
                              timeout=900).stdout.split()
    objs = make("host-objs") + [os.path.join(BUILD, f"render_{u}.o") for u in ("f64", "f64_lgrid")]
    missing = [o for o in objs if not os.path.exists(o)]
    if missing:
        make(*missing)
    obj = os.path.join(tmp, "obj")
    make(f"HIPCC={HIPCC} -DRTW_TRACE=f32", f"OBJ={obj}", f"OUT={obj}", os.path.join(obj, "render_f32.o"))
    lib = os.path.join(tmp, "librtw.so")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, os.path.join(obj, "render_f32.o"),
                    *objs, "-ldl"], check=True, capture_output=True, timeout=300)
    return lib


class Judged:
    pass


@pytest.fixture(scope="module")
def judged(tmp_path_factory):
    t0 = time.time()
    tmp = str(tmp_path_factory.mktemp("hit64_replay"))
    lib = os.environ.get("RTW_HIT64_TRACE_LIB") or build_trace_lib(tmp)
    t_build = time.time() - t0
    npz = os.path.join(tmp, "trace.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hit64_trace_child.py"), npz],
                       env=dict(os.environ, RTW_LIB_OVERRIDE=lib), capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        pytest.fail("the traced renders failed:\n" + r.stdout[-2000:] + r.stderr[-4000:], pytrace=False)
    t_run = time.time() - t0 - t_build
    J = judge(np.load(npz))
    J.times = dict(build_s=round(t_build, 1), child_s=round(t_run, 1), replay_s=round(time.time() - t0 - t_build - t_run, 1))
    print("hit64 replay fixture:", J.times)
    with open(PROFILE, "w") as f:
        for rec in J.records():
            f.write(json.dumps(rec) + "\n")
    return J


def judge(data):
    J = Judged()
    J.data, J.rep, J.renders, J.agree, J.colour = data, hr.Report(), {}, {}, {}
    base, replays = {}, {}
    for name, (scene, _accel, _tuning, _want) in hc.VARIANTS.items():
        if scene not in replays:
            soa, cam = hc.SCENES[scene]()
            replays[scene] = hr.Replay(soa, hc.camera_dict(cam), hc.SEED)
        seg, col = data["seg/" + name], data["col/" + name]
        J.renders[name], paths = hr.judge_render(replays[scene], J.rep, name, hc.pixels(scene), seg, col,
                                                 base.get(scene), coop=name == "lights64/coop")
        J.colour[name] = judge_colours(replays[scene], paths, col, tuple(int(x) for x in data["kernel/" + name]))
        if scene not in base:
            base[scene] = (seg, col, paths)
        else:
            # the same traced ray (origin and direction bits) -> the same object and the same t64 bits
            b = base[scene][0]
            ray = (seg[..., 2:8].view(np.uint64) == b[..., 2:8].view(np.uint64)).all(-1) & (seg[..., 0] != -2.0)
            hit = (seg[..., 0] == b[..., 0]) & (seg[..., 1].view(np.uint64) == b[..., 1].view(np.uint64))
            J.agree[name] = (int(ray.sum()), int((ray & ~hit).sum()), int((seg[..., 0] != -2.0).sum()))
    J.replays = replays

    def records():
        rep = J.rep
        for g in sorted(rep.rows):
            e = rep.err.get(g)
            rec = dict(group=g, rows=rep.rows[g], failed=len(rep.fails.get(g, [])), left_out=len(rep.out.get(g, [])))
            if e:
                rec.update(rule_4x(e))
            yield rec
        for name, (n, same_n, lost) in J.renders.items():
            yield dict(render=name, kernel=[int(x) for x in data["kernel/" + name]], samples=n,
                       equal_to_first_variant=same_n, replay_ended_early=lost, same_ray_rows=J.agree.get(name))
        for name, c in J.colour.items():
            yield dict(colour=name, **{k: v for k, v in c.items() if k != "far"})
        yield dict(fixture=getattr(J, "times", None))
    J.records = records
    return J


COLOUR_MARGIN = 2.0 ** -20


def judge_colours(rp, paths, col, kernel):
    """The traced samples' colours against the law along the traced path.  Non-finite
    patterns must equal the law's (or the f32 calibration's); a finite sample is left
    out only where one of its Lambertian bounces has a decision of the law (a light's
    hit test, the face of the f32 normal) within COLOUR_MARGIN = 2^-20 -- 16 f32
    roundings of a quantity normalised to 1 -- of flipping, or where the correctly
    rounded f32 evaluation itself is not finite."""
    keys, law, cal, margin = hr.colour_laws(rp, paths, kernel)
    got = np.array([col[k, s, :3] for k, s in keys]).reshape(-1, 3)
    def pattern(a, b):
        return ((np.isnan(a) == np.isnan(b)) & (np.isinf(a) == np.isinf(b))).all(-1)
    # non-finite where the law is, or (an f32 overflow, an f32 sqrt of a rounded negative) where
    # the correctly rounded f32 evaluation is
    ok = pattern(got, law) | pattern(got, cal)
    fin = np.isfinite(got).all(-1) & np.isfinite(law).all(-1)
    near = (margin < COLOUR_MARGIN) | (fin & ~np.isfinite(cal).all(-1))
    use = fin & ~near
    ek, ec = np.abs(got - law).max(-1)[use], np.abs(cal - law).max(-1)[use]
    out = dict(samples=len(keys), finite=int(fin.sum()), nonzero=int((fin & (got != 0).any(-1)).sum()),
               left_out=int((fin & near).sum()), pattern_differs=int((~ok).sum()))
    for q, name in ((50, "p50"), (99, "p99"), (100, "max")):
        out["kernel_" + name], out["calib_" + name] = float(np.percentile(ek, q)), float(np.percentile(ec, q))
    return out


def rule_4x(e):
    k = np.array([x[0][0] for x in e], np.float64)
    c = np.array([x[1] for x in e], np.float64)
    out = dict(bit_equal=int(sum(bool(x[0][1]) for x in e)), n=len(e))
    for q, name in ((50, "p50"), (99, "p99"), (100, "max")):
        out["kernel_" + name], out["calib_" + name] = float(np.percentile(k, q)), float(np.percentile(c, q))
    return out


# ---------------------------------------------------------------------- the tests
EXACT = ["ray origin is the f64 hit point", "exact direction", "dither64", "own sphere carried",
         "own-sphere re-hit taken", "own-sphere re-hit refused", "other sphere", "plane", "segment count",
         "termination: miss", "termination: metal absorbed", "termination: plane metal absorbed",
         "termination: invisible", "termination: depth exhausted"]


@pytest.mark.parametrize("group", EXACT)
def test_exact_checks_hold_bit_for_bit(judged, group):
    rep = judged.rep
    rows, fails = rep.rows.get(group, 0), rep.fails.get(group, [])
    print(group, "rows", rows, "failed", len(fails), fails[:5])
    assert rows > 0, "no row reached this check"
    assert not fails, f"{len(fails)} of {rows} rows: {fails[:5]}"


@pytest.mark.parametrize("group", GROUPS)
def test_every_group_is_reached(judged, group):
    rep = judged.rep
    rows, out = rep.rows.get(group, 0), len(rep.out.get(group, []))
    print(group, "rows", rows, "left out", out)
    assert rows >= MIN_ROWS, f"{group}: {rows} rows"
    assert out <= MAX_OUT * rows


@pytest.mark.parametrize("group", ["lambertian to light sphere", "lambertian cosine sphere",
                                   "lambertian to light plane", "lambertian cosine plane", "metal fuzz > 0"])
def test_directions_under_the_4x_rule(judged, group):
    """The Lambertian direction: mixture_direction<double> in the f32 unit is compiled
    with -ffp-contract=on and carries no contract(off) pragma, so its bits are the
    no-FMA law's only where no product feeds an add; it is held to the law in
    np.longdouble within 4 x the no-FMA f64 evaluation's own error."""
    r = rule_4x(judged.rep.err[group])
    print(group, r)
    for q in ("p50", "p99", "max"):
        assert r["kernel_" + q] <= 4.0 * r["calib_" + q], (group, q, r)


@pytest.mark.parametrize("group", ["picked: miss", "picked: own sphere", "picked: plane", "picked: sphere"])
def test_the_object_picked_is_the_f64_closest(judged, group):
    rep = judged.rep
    rows, out = rep.rows.get(group, 0), rep.out.get(group, [])
    margin, worst = picked_margin(judged, group, out)
    print(group, "rows", rows, "differ", len(out), "margin", margin, "worst gap", worst)
    with open(PROFILE, "a") as f:
        f.write(json.dumps(dict(picked=group, rows=rows, differ=len(out), margin_t=margin, worst_gap=worst)) + "\n")
    assert rows >= MIN_ROWS
    assert len(out) <= MAX_OUT * rows
    far = [o for o in out if not o["gap"] < margin]
    assert not far, far[:5]


def picked_margin(J, group, out):
    """4 x the p99 of the f32 calibration's error in t (the form in f32 against the
    form in f64, both on the f32 ray and sphere) over the rows that differ and every
    16th row that agrees; each differing row gets its gap: the f64 t of the two candidates"""
    errs, worst = [], 0.0
    for o in J.rep.agreed.get(group, []):
        sc = J.replays[o["tag"].split("/")[0]].sc
        S = sc.sph[o["obj"] - sc.sbase]
        a, b = hr.sphere_t_f32(S, hr.v32(o["o"]), hr.v32(o["d"]), True), \
            hr.sphere_t_f32(S, hr.v32(o["o"]), hr.v32(o["d"]), False)
        if a == a and b == b:
            errs.append(abs(a - b))
    for o in out:
        sc = J.replays[o["tag"].split("/")[0]].sc
        t_first = o["hits"][0][0] if o["hits"] else hr.INF
        t_obj = o["t"] if o["obj"] >= 0 else hr.INF
        if o["obj"] >= 0 and o["first"] < 0:
            t_first = hr.INF
        o["gap"] = abs(t_first - t_obj) if t_first != t_obj else 0.0
        if o["gap"] == hr.INF:
            # one side misses: a graze.  The gap is the chord the f64 hit cuts, t2 - t1
            k = (o["first"] if o["first"] >= 0 else o["obj"]) - sc.sbase
            o["gap"] = chord(sc.sph64[k], o["o"], o["d"]) if k >= 0 else hr.INF
        worst = max(worst, o["gap"])
        for ident in (o["obj"], o["first"]):
            if ident >= sc.sbase:
                S = sc.sph[ident - sc.sbase]
                a, b = hr.sphere_t_f32(S, hr.v32(o["o"]), hr.v32(o["d"]), True), \
                    hr.sphere_t_f32(S, hr.v32(o["o"]), hr.v32(o["d"]), False)
                if a == a and b == b:
                    errs.append(abs(a - b))
    return (4.0 * float(np.percentile(errs, 99)) if errs else 0.0), worst


def chord(S, o, d):
    oc = hr.RS.sub(o, S[:3])
    a, hb = hr.RS.dot(d, d), hr.RS.dot(oc, d)
    disc = hb * hb - a * (hr.RS.dot(oc, oc) - S[3] * S[3])
    return 2.0 * hr.RS.sqrt(max(disc, 0.0)) / a


def test_the_variants_agree_on_the_same_ray(judged):
    """brute force, the four BVH kinds, the LDS tree with stealing, the robust sphere
    form, the light grid (cooperative and per lane) and the light BVH: for the same
    traced ray the same object and the same t64 bits"""
    for name, (rays, differ, segs) in judged.agree.items():
        print(name, "segments", segs, "rays equal to the first variant's", rays, "of which object or t64 differ", differ)
        assert rays >= 0.9 * segs, name
        assert differ == 0, name


def test_replays_that_ended_early_are_few(judged):
    for name, (n, same_n, lost) in judged.renders.items():
        print(name, "samples", n, "equal to the first variant's", same_n, "replay ended early", lost)
        assert lost <= MAX_OUT * n, name


@pytest.mark.parametrize("name", list(hc.VARIANTS))
def test_the_samples_colour_along_the_traced_path(judged, name):
    """the only record-level check of the render's own light pdf sums (lights_pdf_sum_pk
    with the sampled light, the grid's and the light BVH's deferred weights)"""
    c = judged.colour[name]
    print(name, c)
    assert c["pattern_differs"] == 0
    assert c["left_out"] <= MAX_OUT * c["samples"]
    for q in ("p50", "p99", "max"):
        assert c["kernel_" + q] <= 4.0 * c["calib_" + q], (name, q, c)
