"""Shading points and expected answers for the ambient-occlusion tests
(tests/test_ambient_host.py, tests/test_gpu_ambient.py).  Everything here is
computed on the CPU from the independent restatement (tests/indep/restate.py:
Rng, cosine_hemisphere, Onb) and the any-hit restatement (nee_cases.any_hit,
every AABB gate on) only, once per test run (lru_cache) -- nothing touches the
GPU.  The law of include/rtw.h in Python floats:

    for s in first_sample .. first_sample + S - 1:
        g = Rng(seed, first_stream + k, s)
        d = Onb(normal).transform(cosine_hemisphere(g))       # CosinePdf::generate: two draws
        occ = any(ob.aabb.is_hit(p, d, t_min, t_max) and ob.hit(p, d, t_min, t_max) for ob in world)
        open[k] += not occ

A NaN ray and an empty or NaN range answer 0 (open); a point whose normal is
exactly (0, 0, 0) is skipped.  As nee_cases.reference does, the expectation
asserts that no sphere's gate changes an answer (the kernel models none).

The points are direct_cases.bounce_points (the Lambertian bounce points of the
oracle's paths, with their normals) and direct_cases' lights64 points.  Each
case's t_max and S are chosen so that the restatement alone gives at least 10 %
open and at least 10 % occluded pairs: case() asserts it before any GPU answer
is compared.

t_min.  The bounce points lie on their surfaces, and with the reference's t_min
= f64::EPSILON a ray may meet its own surface at t ~ 1e-15 (the reference's
self-intersection, camera.rs:473).  That decision does not survive rounding the
inputs: on the restatement alone, with {p, d} merely rounded to f32 and
widened again, 73 of simple's 412 pairs and 40 of simple_light's 176 answer
otherwise at t_min = EPS (1 of cornell_box's 652, 0 of lights64's 512), and none
of any case's at t_min = 1e-3.  An ambient-occlusion pass offsets its rays, so
the cases take T_MIN = 1e-3, where the f32 context can be held to the f64 case
file.  The reference's own t_min keeps its bit-for-bit check in f64: eps_case()
is simple and simple_light at t_min = EPS."""
import functools
import math

import numpy as np

import direct_cases as D
import nee_cases as N
import query_cases as Q
import ray_tracing_weekend_amd as rtw
from indep import restate as R

EPS = Q.EPS
INF = float("inf")
SEED = 0xA0C1
T_MIN = 1e-3
MIN_SHARE = 0.10


def zero_normal(nrm):
    return nrm[0] == 0.0 and nrm[1] == 0.0 and nrm[2] == 0.0


def direction(nrm, seed, stream, s):
    """CosinePdf::new(normal).generate(rng) from the start of Rng(seed, stream, s)"""
    return R.Onb(nrm).transform(R.cosine_hemisphere(R.Rng(seed, stream, s)))


class Expected:
    """directions [n * S, 3], occluded [n * S] uint8, open [n] uint32 -- the law in Python
    floats; gate_changes: the pairs a sphere's own AABB gate would answer otherwise."""

    def __init__(self, soa, points, seed, S, t_max, t_min=EPS, first_stream=0, first_sample=0, open=None):
        w = R.World(soa)
        n = len(points)
        self.directions = np.zeros((n * S, 3))
        self.occluded = np.zeros(n * S, np.uint8)
        self.open = np.zeros(n, np.uint32) if open is None else np.array(open, np.uint32)
        self.t_min, self.t_max = float(t_min), float(t_max)
        self.live = np.zeros(n * S, bool)
        self.gate_changes = 0
        empty = not (t_max >= t_min)          # (NaN too)
        for k, row in enumerate(points):
            p, nrm = tuple(map(float, row[:3])), tuple(map(float, row[3:6]))
            if zero_normal(nrm):
                continue
            for j in range(S):
                d = tuple(direction(nrm, seed, first_stream + k, first_sample + j))
                r = k * S + j
                self.directions[r] = d
                self.live[r] = True
                occ = False
                if not empty and not any(math.isnan(x) for x in (*p, *d)):
                    on, model, _ = N.any_hit(w, p, d, float(t_min), float(t_max))
                    self.gate_changes += int(on != model)
                    occ = on
                self.occluded[r] = occ
                self.open[k] += 0 if occ else 1
        assert self.gate_changes == 0, f"a sphere's AABB gate changes {self.gate_changes} answers"

    @property
    def pairs(self):
        return int(self.live.sum())

    @property
    def n_open(self):
        return int((self.live & (self.occluded == 0)).sum())

    @property
    def n_occluded(self):
        return int(self.occluded.sum())


def lights64_points():
    """direct_cases' lights64 points: origins around the scene, the normal (0, -1, 0)"""
    soa, _ = Q.scene("lights64")
    o = Q.rays_at_lights(soa, 2)[:, :3]
    return soa, np.ascontiguousarray(np.concatenate([o, np.tile([0.0, -1.0, 0.0], (len(o), 1))], -1))


# name: (t_max, S) -- simple against the sky; the others within a finite reach
CASES = {"simple": (INF, 2), "cornell_box": (400.0, 4), "simple_light": (4.0, 4), "lights64": (100.0, 4)}
EPS_CASES = ("simple", "simple_light")


@functools.lru_cache(maxsize=None)
def case(name, t_min=T_MIN):
    """(soa, points [n, 6], S, t_max, Expected) of a named case at t_min; the CPU conditions of
    the case are asserted here, before any GPU answer is compared"""
    t_max, S = CASES[name]
    soa, pts = lights64_points() if name == "lights64" else D.bounce_points(name)
    assert len(pts) <= 250 and S <= 4
    exp = Expected(soa, pts, SEED, S, t_max, t_min)
    assert exp.pairs == len(pts) * S, f"{name}: a zero normal among the points"
    assert exp.n_open >= MIN_SHARE * exp.pairs, f"{name}: {exp.n_open} of {exp.pairs} pairs open"
    assert exp.n_occluded >= MIN_SHARE * exp.pairs, f"{name}: {exp.n_occluded} of {exp.pairs} pairs occluded"
    assert np.array_equal(exp.open, S - exp.occluded.reshape(-1, S).sum(1, dtype=np.uint32))
    return soa, pts, S, t_max, exp


def eps_case(name):
    """a case of EPS_CASES at the reference's own t_min = f64::EPSILON (f64 only: see above)"""
    assert name in EPS_CASES
    return case(name, EPS)


# ---- the closed form: one sphere above a point.  The cosine-weighted share of the hemisphere a
# sphere of radius r at distance D along the normal blocks is sin^2(theta_max) = r^2 / D^2.
CLOSED_S = 4096
CLOSED_POINT = np.array([[0.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
CLOSED_R, CLOSED_D = 1.0, 4.0
CLOSED_BLOCKED = CLOSED_R ** 2 / CLOSED_D ** 2                      # 1/16
# six standard errors of a Bernoulli(1/16) mean over S samples
CLOSED_BOUND = 6.0 * math.sqrt(CLOSED_BLOCKED * (1.0 - CLOSED_BLOCKED) / CLOSED_S)
CLOSED_NEAR = 2.5                                                   # a t_max below D - r: nothing in reach


def closed_form_scene():
    """One sphere, r = 1 at (0, 4, 0), alone in the world; the light list is empty"""
    return rtw.SceneSoA(spheres=np.array([[0.0, CLOSED_D, 0.0, CLOSED_R]]), sphere_mat=np.array([0], np.uint32),
                        mat_type=np.array([rtw.RTW_LAMBERTIAN], np.uint32),
                        mat_params=np.array([[0.5, 0.5, 0.5, 0.0, 0.0]]))


@functools.lru_cache(maxsize=None)
def closed_form(near):
    """(soa, t_max, Expected) of the closed-form case, S = CLOSED_S samples at one point"""
    soa = closed_form_scene()
    t_max = CLOSED_NEAR if near else INF
    return soa, t_max, Expected(soa, CLOSED_POINT, SEED, CLOSED_S, t_max, T_MIN)
