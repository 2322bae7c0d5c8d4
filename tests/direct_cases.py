"""Shading points and expected answers for the direct-lighting tests
(tests/test_direct_host.py, tests/test_gpu_direct_light.py).  Everything here is
computed on the CPU from the independent restatement (tests/indep/restate.py:
World.lights_random, lights_pdf, the list hit, colour, Rng), once per test run
(lru_cache) -- nothing touches the GPU.  The scattering pdf, the term and the
fold are restated here in Python floats:

    for s in first_sample .. first_sample + S - 1:
        g = Rng(seed, first_stream + k, s)
        d = lights.random(p, g);  pdf = lights.pdf_value(p, d)
        rec = world.hit(p, d)                         # EPS..=inf
        Le = emitted(rec)                             # DiffuseLight's texture, else black
        spdf = max(dot(normal, normalize(d)) / PI, 0)
        if rec and pdf > 0 and spdf > 0:  direct[k] += (Le * spdf) / pdf

The points are the Lambertian bounce points of the oracle's paths
(tests/query_cases.py), with the normal of the hit they start on."""
import functools
import math

import numpy as np

import query_cases as Q
import ray_tracing_weekend_amd as rtw
from indep import restate as R

EPS = Q.EPS
SEED = 0xD1EC7


def hit_with_id(w, o, d):
    """restate.World.hit (bounded_hit of every object, the first minimum of t) with the
    object's index: planes, quads, cuboids, spheres -- the queries' object id"""
    best, best_id = None, -1
    for k, ob in enumerate(w.objects):
        if not ob.aabb.is_hit(o, d, EPS, R.INF):
            continue
        rec = ob.hit(o, d, EPS, R.INF)
        if rec is not None and (best is None or rec.t < best.t):
            best, best_id = rec, k
    return best, best_id


class Expected:
    """samples [n * S, 12] {d, pdf, t, spdf, Le, term}, ids [n * S, 4] {light index, object or
    -1, material, added}, direct [n, 3] -- the law of include/rtw.h in Python floats."""

    def __init__(self, soa, points, seed, S, first_stream=0, first_sample=0, direct=None):
        w = R.World(soa)
        n = len(points)
        self.samples = np.zeros((n * S, 12))
        self.ids = np.zeros((n * S, 4), np.int32)
        self.direct = np.zeros((n, 3)) if direct is None else np.array(direct, np.float64)
        for k, row in enumerate(points):
            p, nrm = tuple(map(float, row[:3])), tuple(map(float, row[3:6]))
            if nrm == (0.0, 0.0, 0.0):
                self.ids[k * S:(k + 1) * S, 1] = -1
                continue
            acc = [float(x) for x in self.direct[k]]
            for j in range(S):
                s = first_sample + j
                idx = R.Rng(seed, first_stream + k, s).gen_index(len(w.lights))
                d = tuple(w.lights_random(p, R.Rng(seed, first_stream + k, s)))
                pdf = w.lights_pdf(p, d)
                rec, obj = hit_with_id(w, p, d)
                Le = (0.0, 0.0, 0.0)
                if rec is not None and w.mat_type[rec.mat] == R.DIFFUSE_LIGHT:
                    Le = tuple(w.colour(rec.mat, rec.u, rec.v, rec.p))
                spdf = R.fmax(R.fdiv(R.dot(nrm, R.normalize(d)), R.PI), 0.0)
                adds = rec is not None and pdf > 0.0 and spdf > 0.0
                term = R.divs(R.muls(Le, spdf), pdf) if adds else (0.0, 0.0, 0.0)
                if adds:
                    acc = [acc[c] + term[c] for c in range(3)]
                r = k * S + j
                self.samples[r] = (*d, pdf, rec.t if rec is not None else 0.0, spdf, *Le, *term)
                self.ids[r] = (idx, obj, rec.mat if rec is not None else 0, int(adds))
            self.direct[k] = acc

    @property
    def term(self):
        return self.samples[:, 9:12]

    @property
    def nonzero_terms(self):
        return int((self.term != 0).any(-1).sum())

    @property
    def reach_emitter(self):
        return int((self.samples[:, 6:9] != 0).any(-1).sum())


def bounce_points(name):
    """[n, 6] {p, normal}: the origin of every segment of the oracle's paths that follows a hit
    on a Lambertian surface, with the normal of that hit (the previous row of Segments.hits)."""
    seg = Q.segments(name)
    lam = np.asarray(seg.soa.mat_type)[seg.mat] == rtw.RTW_LAMBERTIAN
    keep = np.nonzero((seg.prev >= 0) & lam[np.maximum(seg.prev, 0)])[0]
    assert np.array_equal(seg.rays[keep, :3], seg.hits[keep - 1, 1:4]), "a bounce starts where the last hit was"
    assert (seg.wid[keep - 1] == seg.prev[keep]).all()
    return seg.soa, np.ascontiguousarray(np.concatenate([seg.rays[keep, :3], seg.hits[keep - 1, 4:7]], -1))


def emissive_lights64():
    """scenes lights64 (the first 64 spheres as the light list) with those spheres' own
    materials made DiffuseLight: each emits its albedo"""
    soa, _ = Q.scene("lights64")
    mats = np.asarray(soa.sphere_mat[:64], np.int64)
    assert len(set(mats)) == 64 and not set(mats) & set(np.asarray(soa.sphere_mat[64:], np.int64)) \
        and not set(mats) & set(np.asarray(soa.plane_mat, np.int64)), "the 64 materials are the lights' alone"
    d = dict(soa.__dict__)
    d["mat_type"] = np.array(soa.mat_type, np.uint32)
    d["mat_type"][mats] = rtw.RTW_DIFFUSE_LIGHT
    return rtw.SceneSoA(**d)


def checker_simple_light():
    """simple_light with its light's texture a Checker (8 x 8 over the quad's uv) of the
    light's own colour and another one"""
    soa, _ = Q.scene("simple_light")
    d = dict(soa.__dict__)
    light_mat = int(np.nonzero(np.asarray(soa.mat_type) == rtw.RTW_DIFFUSE_LIGHT)[0][0])
    old = int(soa.mat_tex[light_mat])
    nt = len(soa.tex_type)
    d["tex_type"] = np.concatenate([soa.tex_type, [R.TEX_SOLID, R.TEX_CHECKER]]).astype(np.uint32)
    d["tex_params"] = np.concatenate([soa.tex_params, [[6.0, 1.0, 0.5, 0.0], [0.0, 0.0, 0.0, 8.0]]])
    d["tex_refs"] = np.concatenate([soa.tex_refs, [[0, 0], [old, nt]]]).astype(np.uint32)
    d["mat_tex"] = np.array(soa.mat_tex, np.uint32)
    d["mat_tex"][light_mat] = nt + 1
    return rtw.SceneSoA(**d)


def closed_form_scene(blocker):
    """One DiffuseLight sphere, r = 1 at (0, 4, 0), Le = 3, alone in the world and the list;
    with `blocker` an opaque (Lambertian) sphere of r = 0.5 at (0, 2, 0) in between"""
    sph, smat = [[0.0, 4.0, 0.0, 1.0]], [0]
    if blocker:
        sph.append([0.0, 2.0, 0.0, 0.5])
        smat.append(1)
    return rtw.SceneSoA(spheres=np.array(sph), sphere_mat=np.array(smat, np.uint32),
                        mat_type=np.array([rtw.RTW_DIFFUSE_LIGHT, rtw.RTW_LAMBERTIAN], np.uint32),
                        mat_params=np.array([[3.0, 3.0, 3.0, 0.0, 0.0], [0.5, 0.5, 0.5, 0.0, 0.0]]),
                        lights=np.array([[0.0, 4.0, 0.0, 1.0]]))


CLOSED_S = 4096
CLOSED_POINT = np.array([[0.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
CLOSED_LE, CLOSED_R, CLOSED_D = 3.0, 1.0, 4.0
# the irradiance integral of a sphere seen from a point on its axis: Le r^2 / D^2
CLOSED_EXPECT = CLOSED_LE * CLOSED_R ** 2 / CLOSED_D ** 2
# every term lies in [Le Omega cos(theta_max) / pi, Le Omega / pi], Omega = 2 pi (1 - cos(theta_max)):
# sigma <= half that range, and the mean of S terms is held to six standard errors
_COS_MAX = math.sqrt(1.0 - CLOSED_R ** 2 / CLOSED_D ** 2)
_OMEGA = 2.0 * math.pi * (1.0 - _COS_MAX)
CLOSED_TERM_RANGE = (CLOSED_LE * _OMEGA * _COS_MAX / math.pi, CLOSED_LE * _OMEGA / math.pi)
CLOSED_BOUND = 6.0 * 0.5 * (CLOSED_TERM_RANGE[1] - CLOSED_TERM_RANGE[0]) / math.sqrt(CLOSED_S)

# name: (the least number of non-zero terms the case must have, or None)
CASES = {"cornell_box": 200, "simple_light": 30, "simple": None, "lights64_emissive": 200, "checker": None}


@functools.lru_cache(maxsize=None)
def case(name):
    """(soa, points [n, 6], S, Expected) of a named case; the CPU conditions of the case are
    asserted here, before any GPU answer is compared"""
    if name == "cornell_box":
        (soa, pts), S = bounce_points("cornell_box"), 4
    elif name == "simple_light":
        (soa, pts), S = bounce_points("simple_light"), 4
    elif name == "simple":
        (soa, pts), S = bounce_points("simple"), 2
    elif name == "lights64_emissive":
        soa, S = emissive_lights64(), 2
        o = Q.rays_at_lights(soa, 2)[:, :3]
        pts = np.ascontiguousarray(np.concatenate([o, np.tile([0.0, -1.0, 0.0], (len(o), 1))], -1))
    elif name == "checker":
        soa, S = checker_simple_light(), 4
        pts = bounce_points("simple_light")[1]
    else:
        raise KeyError(name)
    exp = Expected(soa, pts, SEED, S)
    assert np.isfinite(exp.term).all() and np.isfinite(exp.direct).all(), f"{name}: a non-finite term"
    if CASES[name] is not None:
        assert exp.nonzero_terms >= CASES[name], f"{name}: {exp.nonzero_terms} non-zero terms"
    if name == "simple":   # 19 sphere lights that do not emit: every term and every sum is exactly 0
        assert len(soa.lights) == 19 and not (np.asarray(soa.mat_type) == rtw.RTW_DIFFUSE_LIGHT).any()
        assert exp.nonzero_terms == 0 and (exp.direct == 0.0).all()
    if name == "checker":  # both colours of the checker are met
        assert len({tuple(r) for r in exp.samples[:, 6:9] if r.any()}) == 2
    return soa, pts, S, exp


@functools.lru_cache(maxsize=None)
def closed_form(blocker):
    """(soa, Expected) of the closed-form case, S = CLOSED_S samples at one point"""
    soa = closed_form_scene(blocker)
    return soa, Expected(soa, CLOSED_POINT, SEED, CLOSED_S)


def fold(direct0, term, added, S):
    """the sequential f64 fold of the term columns [n * S, 3] into direct0 [n, 3]: one add per
    sample that added a term, in sample order"""
    out = np.array(direct0, np.float64)
    for k in range(len(out)):
        for j in range(S):
            if added[k * S + j]:
                out[k] = out[k] + np.asarray(term[k * S + j], np.float64)
    return out
