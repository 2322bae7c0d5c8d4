"""Rays, upper range ends and expected answers for the any-hit and light-sample
tests (tests/test_gpu_occlusion.py, test_gpu_light_sample.py, test_gpu_nee_*.py).
Everything here is computed on the CPU from the oracle's path segments
(tests/query_cases.py) and the independent restatement (tests/indep/restate.py),
once per test run (lru_cache) -- nothing touches the GPU.

The any-hit restatement is hittable_list.rs:395-406 over lo..=hi: every object
behind its AABB gate (bounded_hit), the range never shrunk:

    any(ob.aabb.is_hit(o, d, lo, hi) and ob.hit(o, d, lo, hi) is not None for ob in objects)

The kernel models the gates of planes, quads and cuboids and none for a sphere
(neither does the closest-hit query: a sphere's own box is not staged; only a
sphere of negative radius, whose inverted box the reference never passes, is
staged as never hit).
any_hit() therefore returns three answers: every gate on (the reference, what
the GPU is compared with), the spheres' gates off (the kernel's model), and
every gate off.  The tests assert on the CPU, before a GPU answer is compared,
that the first two agree on every batch they use -- a sphere's gate never
changes an answer -- and on scenes::simple that all three do.  The third cannot
hold everywhere: a Transformed<Cuboid> is hit in object space along a direction
that also took the translation (transformations.rs:112-114), so its t is not
the world-space gate's, and the gate does reject such hits (cornell_box: 2 of
240 rays); there the gate is part of the answer and the kernel applies it."""
import functools
import math

import numpy as np

import query_cases as Q
from indep import restate as R

EPS = Q.EPS
INF = float("inf")
NAN = float("nan")
KINDS = ("inf", "t", "below t", "t / 2", "2 t", "uniform (0, 2 t)", "NaN", "0", "< t_min")
MAX_RAYS = 240          # per scene: the restatement is a Python loop over every object


def any_hit(world, o, d, lo, hi):
    """(every AABB gate on, the spheres' gates off, every gate off)"""
    met = [ob for ob in world.objects if ob.hit(o, d, lo, hi) is not None]
    gate = [ob.aabb.is_hit(o, d, lo, hi) for ob in met]
    return any(gate), any(g or (isinstance(ob, R.Sphere) and ob.r >= 0) for g, ob in zip(gate, met)), bool(met)


def any_hit_batch(soa, rays, t_max, t_min=EPS):
    """uint8 [3, n]: the answers of any_hit's three forms"""
    w = R.World(soa)
    out = np.zeros((3, len(rays)), np.uint8)
    for k, (r, hi) in enumerate(zip(rays, t_max)):
        out[:, k] = any_hit(w, tuple(map(float, r[:3])), tuple(map(float, r[3:])), float(t_min), float(hi))
    return out


def reference(soa, rays, t_max, t_min=EPS, every_gate=False):
    """The expected bytes: the reference's answer, after asserting that no sphere's gate (with
    every_gate: no gate at all) changes one on these rays."""
    on, model, off = any_hit_batch(soa, rays, t_max, t_min)
    assert np.array_equal(on, model), f"a sphere's AABB gate changes {int((on != model).sum())} answers"
    if every_gate:
        assert np.array_equal(on, off), f"an AABB gate changes {int((on != off).sum())} answers"
    return on


@functools.lru_cache(maxsize=None)
def simple_segments():
    """The inputs of the CPU check: scenes::simple, seed 0x5EED0001, 40 x 24, pixels (0..40 step 5) x
    (0..24 step 4), samples 0 and 1, path seed 7, depth 50: 239 segments, 143 hit."""
    return Q.Segments("simple", Q.GRID_COARSE, (0, 1))


@functools.lru_cache(maxsize=None)
def segment_rays(name):
    """(soa, rays [n, 6], hit mask, t) of a case: the oracle's path segments, thinned to at
    most MAX_RAYS (every third a miss where there are enough of both)."""
    seg = simple_segments() if name == "simple" else Q.segments(name)
    hit = seg.ids >= 0
    idx = np.arange(len(seg.rays))
    if len(idx) > MAX_RAYS:
        h, m = idx[hit], idx[~hit]
        nh = min(len(h), MAX_RAYS - min(len(m), MAX_RAYS // 3))
        nm = min(len(m), MAX_RAYS - nh)
        pick = lambda a, n: a[np.linspace(0, len(a) - 1, n).round().astype(int)] if n else a[:0]   # noqa: E731
        idx = np.sort(np.concatenate([pick(h, nh), pick(m, nm)]))
    return seg.soa, np.ascontiguousarray(seg.rays[idx]), hit[idx], seg.t[idx]


def t_max_of_kind(kind, t, u):
    """the upper end of KINDS[kind] for a ray whose closest hit is at t (u: a uniform in (0, 1))"""
    return (INF, t, math.nextafter(t, -INF), t / 2, 2 * t, 2 * t * u, NAN, 0.0, EPS / 2)[kind]


@functools.lru_cache(maxsize=None)
def mixed_batch(name):
    """(soa, rays, t_max, expected uint8) -- consecutive rays carry different kinds of t_max
    (ray k: KINDS[k % 9]), so neighbouring lanes diverge.  A miss takes t = 1."""
    soa, rays, hit, t = segment_rays(name)
    rng = np.random.default_rng(0xA11)
    tt = np.where(hit, t, 1.0)
    t_max = np.array([t_max_of_kind(k % len(KINDS), float(tt[k]), float(rng.uniform(1e-6, 1.0)))
                      for k in range(len(rays))])
    return soa, rays, t_max, reference(soa, rays, t_max, every_gate=name in ("simple", "simple63", "plane"))


@functools.lru_cache(maxsize=None)
def simple_identities():
    """The conditions the reference meets on simple_segments(), per kind of t_max:
    {kind: any_hit_batch's three rows} over all 239 segments."""
    seg = simple_segments()
    hit = seg.ids >= 0
    tt = np.where(hit, seg.t, 1.0)
    out = {}
    for kind in (0, 1, 2, 3, 4):
        t_max = np.array([t_max_of_kind(kind, float(t), 0.5) for t in tt])
        out[kind] = any_hit_batch(seg.soa, seg.rays, t_max)
    return seg, out


# ------------------------------------------------------------ light sampling
def light_samples(soa, origins, seed, first_stream, sample):
    """(directions [n, 3], list indices [n], pdf [n]) of restate's lights_random / lights_pdf
    with point k on the stream Rng(seed, first_stream + k, sample)"""
    w = R.World(soa)
    n_list = len(w.lights)
    dirs, idx, pdf = np.zeros((len(origins), 3)), np.zeros(len(origins), np.int32), np.zeros(len(origins))
    for k, o in enumerate(origins):
        o = tuple(map(float, o))
        idx[k] = R.Rng(seed, first_stream + k, sample).gen_index(n_list)
        d = w.lights_random(o, R.Rng(seed, first_stream + k, sample))
        dirs[k] = d
        pdf[k] = w.lights_pdf(o, tuple(d))
    return dirs, idx, pdf


@functools.lru_cache(maxsize=None)
def bounce_points(name, limit=300):
    """Lambertian bounce points of the oracle's paths (the integrator's shading points)"""
    seg = Q.segments(name)
    return seg.soa, np.ascontiguousarray(Q.lambertian_bounces(seg)[:limit, :3])
