"""Rays, start states and expected answers for the radiance tests
(tests/test_radiance_host.py, tests/test_gpu_radiance.py).

The law of include/rtw.h (rtw_radiance_rays) restated twice:

  * law_path / Expected: in Python floats, from the independent restatement only
    (tests/indep/restate.py: Rng, World.hit; path_cases.Shader.bounce, the body of
    restate.trace_sample's loop).  Nothing touches the GPU; the host test holds it
    against restate.trace_sample on camera rays.

        for s in first_sample .. first_sample + S - 1:
            g = Rng(seed, first_stream + k, s)  or  the caller's state rng[k]
            mult, res, r = (1, 1, 1), 0, rays[k]
            for round in 0 .. max_depth - 1:
                rec = world.hit(r, EPS..=INF);  event, emitted, weight, next = bounce(rec, g)
                MISS:     colour = mult * background + res; break
                ABSORBED: colour = mult * emitted + res;    break
                SCATTER:  res += mult * emitted;  mult *= weight;  r = next
                REFLECT:  mult *= weight;  r = next
            else: colour = 0 + res
            radiance[k] += colour

  * compose: the same loop over a context's own queries (hit_rays, shade_rays) and
    wavefront_cases.advance, in the context's precision -- what the fused kernel
    must equal bit for bit in f32 too.

A start state of four zero words is no xoshiro256++ state: as rtw_shade_rays, the
stream of (0, 0, 0) stands in from the path's first hit on, and a path that never
hits leaves the words as they are."""
import functools

import numpy as np

import path_cases as P
import query_cases as Q
import wavefront_cases as WF
from indep import restate as R
from oracle import oracle as O

W, H = 25, 15                 # 375 rays: the second block of 256 is ragged, its last wave partial
DEPTH = 8
SEED = 0x5AD1A
SAMPLES = (0, 1, 2)
SIZES = (1, 63, 64, 65, 257)
ZERO3 = (0.0, 0.0, 0.0)
same = WF.same


def start_states(seed, first_stream, n, s):
    """[n, 4] uint64: Rng(seed, first_stream + k, s) from its start"""
    return np.array([R.Rng(seed, first_stream + k, s).s for k in range(n)], np.uint64)


def law_path(shader, ray, state, max_depth, bg):
    """One path of the law in Python floats: (colour, segments, the state afterwards)"""
    g = R.Rng(0, 0, 0)
    g.s = [int(x) for x in state]
    o, d = tuple(map(float, ray[:3])), tuple(map(float, ray[3:6]))
    mult, res = (1.0, 1.0, 1.0), ZERO3
    bg = tuple(map(float, bg))
    for segments in range(1, max_depth + 1):
        rec = shader.world.hit(o, d)
        if rec is not None and not any(g.s):
            g = R.Rng(0, 0, 0)
        b = shader.bounce(o, d, rec, g)
        if b["event"] == P.MISS:
            return R.add(R.mulv(mult, bg), res), segments, tuple(g.s)
        if b["event"] == P.ABSORBED:
            return R.add(R.mulv(mult, b["emitted"]), res), segments, tuple(g.s)
        if b["event"] == P.SCATTER:
            res = R.add(res, R.mulv(mult, b["emitted"]))
        mult = R.mulv(mult, b["weight"])
        o, d = b["next"][:3], b["next"][3:]
    return R.add(ZERO3, res), max_depth, tuple(g.s)


class Expected:
    """colours [n * S, 3], segments [n * S] uint32, radiance [n, 3], rng [n, 4] (rng mode) --
    the law in Python floats"""

    def __init__(self, soa, rays, seed, S=1, max_depth=DEPTH, bg=ZERO3, first_stream=0, first_sample=0, rng=None,
                 radiance=None):
        shader = P.Shader(soa)
        n = len(rays)
        assert rng is None or S == 1
        self.colours = np.zeros((n * S, 3))
        self.segments = np.zeros(n * S, np.uint32)
        self.radiance = np.zeros((n, 3)) if radiance is None else np.array(radiance, np.float64)
        self.rng = None if rng is None else np.array(rng, np.uint64)
        for k in range(n):
            for j in range(S):
                state = self.rng[k] if rng is not None else R.Rng(seed, first_stream + k, first_sample + j).s
                c, segs, after = law_path(shader, rays[k], state, max_depth, bg)
                self.colours[k * S + j], self.segments[k * S + j] = c, segs
                self.radiance[k] = self.radiance[k] + np.array(c)
                if rng is not None:
                    self.rng[k] = after


def compose(r, rays, rng0, max_depth, bg):
    """The loop of the context's own queries on these rays and start states:
    (colours [n, 3] and segments [n] uint32 of the one sample, the states afterwards).
    hit_rays, shade_rays and wavefront_cases.advance, in the rays' dtype."""
    rays = np.ascontiguousarray(rays)
    dt, n = rays.dtype, len(rays)
    colour = np.zeros((n, 3), dt)
    segs = np.zeros(n, np.uint32)
    rng_out = np.array(rng0, np.uint64)
    st = dict(rays=rays, rng=rng_out.copy(), mult=np.ones((n, 3), dt), res=np.zeros((n, 3), dt),
              slot=np.arange(n, dtype=np.int64))
    for depth in range(max_depth):
        if len(st["slot"]) == 0:
            break
        cur = np.ascontiguousarray(st["rays"])
        rng = np.ascontiguousarray(st["rng"])
        hits, ids = r.hit_rays(cur)
        nxt, weight, emitted, event = r.shade_rays(cur, hits, ids, rng)
        segs[st["slot"]] += 1
        rng_out[st["slot"]] = rng
        rec = dict(mult=st["mult"], res=st["res"], slot=st["slot"], event=event, weight=weight, emitted=emitted,
                   nxt=nxt, rng=rng)
        st, colour = WF.advance(rec, colour, bg, last=depth == max_depth - 1)
    return colour, segs, rng_out


def fold(radiance0, colours, S):
    """radiance0 [n, 3] + the rows' colours as f64, one add per sample in sample order"""
    out = np.array(radiance0, np.float64)
    c = np.asarray(colours).astype(np.float64).reshape(len(out), S, 3)
    for j in range(S):
        out = out + c[:, j]
    return out


# ---- the scenes of the GPU tests, each with the camera of its case file at 25 x 15
def lights64_emissive():
    import direct_cases as D
    return D.emissive_lights64(), Q.scene("lights64")[1]


def checker():
    import direct_cases as D
    return D.checker_simple_light(), Q.scene("simple_light")[1]


SCENES = ("cornell_box", "simple", "simple_light", "checker", "lights64_emissive")


@functools.lru_cache(maxsize=None)
def scene(name):
    """(soa, camera builder) of a named case"""
    if name == "lights64_emissive":
        return lights64_emissive()
    if name == "checker":
        return checker()
    return Q.scene(name)


def camera(name, depth=DEPTH, spp=len(SAMPLES)):
    _, b = scene(name)
    return b.copy().with_image_width(W).with_image_height(H).with_samples_per_pixel(spp).with_max_depth(depth).build()


def oracle_camera(name, depth=DEPTH, spp=len(SAMPLES)):
    _, b = scene(name)
    return Q.oracle_cam(b.copy(), W, H, spp, depth)


@functools.lru_cache(maxsize=None)
def oracle_samples(name, depth=DEPTH):
    """[len(SAMPLES), H * W, 3]: the oracle's traced sample of every pixel"""
    soa, _ = scene(name)
    ocam, sc = oracle_camera(name, depth), O.Scene(**soa.__dict__)
    out = np.zeros((len(SAMPLES), H * W, 3))
    for a, s in enumerate(SAMPLES):
        for pix in range(H * W):
            out[a, pix] = O.trace_sample(ocam, sc, SEED, pix % W, pix // W, s)[0]
    return out


# ---- lanes out of phase: rays that miss at round 0 alternate with rays inside the closed box
def cornell_phase_rays(n=64):
    """even rows: from outside the box into the empty half space (a miss at round 0);
    odd rows: from the box's middle towards its walls (paths of many rounds)"""
    rng = np.random.default_rng(5)
    rays = np.zeros((n, 6))
    for k in range(n):
        if k % 2 == 0:
            rays[k] = (278.0, 278.0, -900.0, rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), -1.0)
        else:
            d = rng.normal(size=3)
            rays[k] = (278.0 + rng.uniform(-60, 60), 278.0 + rng.uniform(-60, 60), 278.0, *d)
    return rays


# ---- closed forms
LIGHT_E = (3.0, 0.5, 7.25)


def inside_a_light():
    """One DiffuseLight sphere of r = 10 about the origin: every ray from inside meets it
    and is absorbed with colour (1, 1, 1) * E + 0 = E exactly"""
    import ray_tracing_weekend_amd as rtw
    return rtw.SceneSoA(spheres=np.array([[0.0, 0.0, 0.0, 10.0]]), sphere_mat=np.array([0], np.uint32),
                        mat_type=np.array([rtw.RTW_DIFFUSE_LIGHT], np.uint32),
                        mat_params=np.array([[*LIGHT_E, 0.0, 0.0]]))


def rays_from_inside(n=65):
    rng = np.random.default_rng(9)
    return np.ascontiguousarray(np.concatenate([rng.uniform(-3, 3, (n, 3)), rng.normal(size=(n, 3))], 1))
