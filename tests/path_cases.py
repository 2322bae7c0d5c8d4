"""Expected camera rays and bounces for the path-query tests
(tests/test_gpu_camera_rays.py, test_gpu_shade_rays.py, test_gpu_wavefront.py),
from the independent restatement's own pieces (tests/indep/restate.py) --
nothing here touches the GPU, and each reference is computed once per test run
and shared.

restate.trace_sample's loop is unrolled here so that every segment yields what
the two queries answer: the incoming ray, the record of world.hit, the RNG words
before and after the bounce, and the event, emitted, weight, next ray and the
three pdf values.  unroll() asserts that its colour is trace_sample's: the
unrolled loop is the restated one.

A NoiseTexture is not restated in tests/indep (World.colour raises): such a
colour is the oracle's O.texture_colour, as in tests/feature_cases.py."""
import functools

import numpy as np

import query_cases as Q
from indep import restate as R
from oracle import oracle as O

MISS, ABSORBED, REFLECT, SCATTER = 0, 1, 2, 3
SEED = Q.SEED
ZERO3 = (0.0, 0.0, 0.0)


def get_ray(cam, seed, pix, s):
    """Camera::get_ray of pixel index pix = j * W + i, sample s: (origin,
    direction, the stream after its draws) -- the head of restate.trace_sample."""
    W = cam["image_width"]
    i, j = pix % W, pix // W
    g = R.Rng(seed, pix, s)
    scale = R.uniform_inclusive_scale(-0.5, 0.5)
    ox = g.uniform(-0.5, scale)
    oy = g.uniform(-0.5, scale)
    ps = R.add(R.add(cam["pixel00_loc"], R.muls(cam["pixel_delta_u"], float(i) + ox)),
               R.muls(cam["pixel_delta_v"], float(j) + oy))
    if cam["defocus_angle"] <= R.EPS:
        origin = tuple(cam["center"])
    else:
        p = R.unit_disk(g)
        origin = R.add(R.add(cam["center"], R.muls(cam["defocus_disk_u"], p[0])), R.muls(cam["defocus_disk_v"], p[2]))
    return origin, R.sub(ps, origin), g


def camera_rays(cam, seed, pixels, s):
    """(rays [n, 6], rng [n, 4] uint64) of get_ray for these pixel indices"""
    rays, rng = np.zeros((len(pixels), 6)), np.zeros((len(pixels), 4), np.uint64)
    for k, pix in enumerate(pixels):
        o, d, g = get_ray(cam, seed, int(pix), s)
        rays[k], rng[k] = (*o, *d), g.s
    return rays, rng


class Shader:
    """The body of restate.trace_sample's loop after world.hit, one call a bounce."""

    def __init__(self, soa):
        self.soa, self.world = soa, R.World(soa)
        self.osc = O.Scene(**soa.__dict__)

    def colour(self, rec):
        try:
            return tuple(self.world.colour(rec.mat, rec.u, rec.v, rec.p))
        except NotImplementedError:             # NoiseTexture: the oracle's
            return tuple(O.texture_colour(self.osc, int(self.soa.mat_tex[rec.mat]), rec.u, rec.v, rec.p))

    def tex_kind(self, rec):
        """the kind of the texture the material's colour ends in (0 solid, 1 checker, 2 noise)"""
        w = self.world
        if w.mat_tex is None:
            return R.TEX_SOLID
        return w.tex[w.mat_tex[rec.mat]][0]

    def bounce(self, o, d, rec, g):
        """dict(event, emitted, weight, next, pdfs, what): `what` names the branch taken"""
        w = self.world
        if rec is None:
            return dict(event=MISS, emitted=ZERO3, weight=ZERO3, next=ZERO3 + ZERO3, pdfs=ZERO3, what="miss")
        mtype = w.mat_type[rec.mat]
        emitted = self.colour(rec) if mtype == R.DIFFUSE_LIGHT else ZERO3
        gone = dict(event=ABSORBED, emitted=emitted, weight=ZERO3, next=ZERO3 + ZERO3, pdfs=ZERO3)
        if mtype == R.METAL:
            albedo, fuzz = w.mat_params[rec.mat][:3], w.mat_params[rec.mat][3]
            reflected = R.reflect(R.normalize(d), rec.normal)
            dirn = R.add(reflected, R.muls(R.unit_sphere(g), fuzz))
            if not R.dot(dirn, rec.normal) > 0.0:
                return dict(gone, what="metal absorbed")
            return dict(event=REFLECT, emitted=emitted, weight=tuple(albedo), next=(*rec.p, *dirn), pdfs=ZERO3,
                        what="metal")
        if mtype == R.DIELECTRIC:
            ior = w.mat_params[rec.mat][4]
            ratio = R.fdiv(1.0, ior) if rec.front else ior
            unit = R.normalize(d)
            cos_t = R.fmin(R.dot(unit, R.neg(rec.normal)), 1.0)
            sin_t = R.sqrt(1.0 - cos_t * cos_t)
            if ratio * sin_t > 1.0:
                dirn, what = R.reflect(unit, rec.normal), "total internal reflection"
            else:
                r0 = R.fdiv(1.0 - ratio, 1.0 + ratio)
                r0 = r0 * r0
                x = 1.0 - cos_t
                refl = r0 + (1.0 - r0) * (x * ((x * x) * (x * x)))
                if refl > g.open01():
                    dirn, what = R.reflect(unit, rec.normal), "schlick reflection"
                else:
                    dirn, what = R.refract(unit, rec.normal, ratio), "refraction"
            return dict(event=REFLECT, emitted=emitted, weight=(1.0, 1.0, 1.0), next=(*rec.p, *dirn), pdfs=ZERO3,
                        what=what)
        if mtype == R.LAMBERTIAN:
            att = self.colour(rec)
            uvw = R.Onb(rec.normal)
            if g.standard() < 0.5:
                L = w.lights[g.gen_index(len(w.lights))]
                what = "light default" if L is None else ("light sphere" if isinstance(L, R.Sphere) else "light quad")
                dirn = (1.0, 0.0, 0.0) if L is None else L.random(rec.p, g)
            else:
                dirn, what = uvw.transform(R.cosine_hemisphere(g)), "cosine lobe"
            cosine_value = R.fmax(R.fdiv(R.dot(R.normalize(dirn), uvw.w), R.PI), 0.0)
            lpdf = w.lights_pdf(rec.p, dirn)
            pdf = lpdf * 0.5 + cosine_value * 0.5
            spdf = R.fmax(R.fdiv(R.dot(rec.normal, R.normalize(dirn)), R.PI), 0.0)
            weight = R.divs(R.muls(att, spdf), pdf)
            return dict(event=SCATTER, emitted=emitted, weight=weight, next=(*rec.p, *dirn), pdfs=(pdf, lpdf, spdf),
                        what=what)
        return dict(gone, what="diffuse light" if mtype == R.DIFFUSE_LIGHT else "invisible")


def unroll(shader, cam, seed, pix, s, check=True):
    """The segments of sample s of pixel index pix: a list of dicts (ray, rec,
    rng0, rng1, the bounce's fields, mult and res before the bounce) and the
    sample's colour.  The colour is asserted to be restate.trace_sample's."""
    o, d, g = get_ray(cam, seed, pix, s)
    mult, res = (1.0, 1.0, 1.0), ZERO3
    bg = tuple(cam["background"])
    out, colour = [], None
    for _ in range(cam["max_depth"]):
        rec = shader.world.hit(o, d)
        seg = dict(ray=(*o, *d), rec=rec, rng0=tuple(g.s), mult=mult, res=res, pix=pix, s=s)
        seg.update(shader.bounce(o, d, rec, g))
        seg["rng1"] = tuple(g.s)
        out.append(seg)
        if seg["event"] == MISS:
            colour = R.add(R.mulv(mult, bg), res)
        elif seg["event"] == ABSORBED:
            colour = R.add(R.mulv(mult, seg["emitted"]), res)
        if colour is not None:
            break
        if seg["event"] == SCATTER:
            res = R.add(res, R.mulv(mult, seg["emitted"]))
        mult = R.mulv(mult, seg["weight"])
        o, d = seg["next"][:3], seg["next"][3:]
    if colour is None:
        colour = R.add(ZERO3, res)
    if check and shader.world.mat_tex is not None and any(k == 2 for k, _, _ in shader.world.tex):
        check = False                          # (trace_sample does not restate a NoiseTexture)
    if check:
        W = cam["image_width"]
        want, segs = R.trace_sample(cam, shader.world, seed, pix % W, pix // W, s)
        assert segs == len(out) and _same(colour, want), (pix, s, colour, want)
    return out, colour


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def grid(name):
    """(pixels, samples) of query_cases.segments(name), in its order"""
    if name == "simple":
        return Q.GRID_SIMPLE, (0, 1)
    if name == "simple63":
        return Q.GRID_FULL, (0, 1)
    if name in ("simple_transform", "simple_light"):
        return Q.GRID_FULL, (0,)
    return Q.GRID_COARSE, (0, 1)


# the sphere light the scenes without a light list are given (NO_LIGHTS below), so that
# their materials reach the bounce: above the scene, not a world object
ADDED_LIGHT = ((0.0, 12.0, 0.0, 2.0),)


def scene(name):
    """(SceneSoA, CameraBuilder): query_cases.scene's, or for "<name>+light" that scene
    with ADDED_LIGHT as its light list"""
    if name.endswith("+light"):
        soa, b = Q.scene(name[:-len("+light")])
        return Q.with_lights(soa, ADDED_LIGHT), b
    return Q.scene(name)


class Bounces:
    """Every segment of the paths of query_cases.segments(name), as arrays row
    for row with its rays: rays [n, 6], rng0 / rng1 [n, 4] uint64, event [n],
    emitted / weight [n, 3], next [n, 6], pdfs [n, 3], what [n] (the branch), and
    per segment the restated record (rec) with the texture kind of its colour."""

    def __init__(self, name, W=40, H=24, depth=50):
        soa, b = scene(name)
        self.name, self.soa = name, soa
        self.shader = Shader(soa)
        self.cam = O.camera_dict(Q.oracle_cam(b.copy(), W, H, 2, depth))
        pixels, samples = (Q.GRID_FULL, (0,)) if name.endswith("+light") else grid(name)
        segs = []
        for (i, j) in pixels:
            for s in samples:
                segs += unroll(self.shader, self.cam, SEED, j * W + i, s)[0]
        self.segs = segs
        n = len(segs)
        col = lambda key, width, dtype=np.float64: np.ascontiguousarray(   # noqa: E731
            np.array([sg[key] for sg in segs], dtype).reshape(n, width))
        self.rays, self.next = col("ray", 6), col("next", 6)
        self.rng0, self.rng1 = col("rng0", 4, np.uint64), col("rng1", 4, np.uint64)
        self.emitted, self.weight, self.pdfs = col("emitted", 3), col("weight", 3), col("pdfs", 3)
        self.event = np.array([sg["event"] for sg in segs], np.int32)
        self.what = np.array([sg["what"] for sg in segs])
        self.tex = np.array([-1 if sg["rec"] is None else self.shader.tex_kind(sg["rec"]) for sg in segs])
        self.mtype = np.array([-1 if sg["rec"] is None else self.shader.world.mat_type[sg["rec"].mat] for sg in segs])
        self.front = np.array([True if sg["rec"] is None else sg["rec"].front for sg in segs])


@functools.lru_cache(maxsize=None)
def bounces(name):
    return Bounces(name)


# every scene rtw_scene_named accepts, plus lights64; the two whose light list is empty while
# they hold a Lambertian material are refused by rtw_shade_rays (RTW_E_NO_LIGHTS) -- the
# reference panics there (hittable_list.rs:417), and restate's gen_index(0) never returns
NO_LIGHTS = ("perlin_spheres", "plane")
NAMES = ("cornell_box", "debug", "checkered_spheres", "simple", "simple_light", "simple_transform", "lights64")
# ... and those two with a light list added: every pixel, one sample, so that their
# textured materials go through the bounce as well
LIT_NAMES = tuple(n + "+light" for n in NO_LIGHTS)


@functools.lru_cache(maxsize=None)
def textured_lights():
    """A hand-made scene for the emitters no named scene holds: DiffuseLight spheres with
    a Checker and a Noise texture (and a Solid one), over a checkered Lambertian ground
    sphere, one of the emitters in the light list.  (SceneSoA, rays [n, 6], streams [n]):
    rays onto every sphere from several sides, hits at many (u, v, p)."""
    import ray_tracing_weekend_amd as rtw
    checker = rtw.CheckerTexture.new_with_colours((4.0, 0.5, 0.25), (0.25, 0.5, 4.0), 0.125)
    centres = {"checker": (-3.0, 1.0, 0.0), "noise": (0.0, 1.0, 0.0), "solid": (3.0, 1.0, 0.0)}
    world = rtw.HittableList([
        rtw.Sphere((0.0, -1000.0, 0.0), 1000.0, rtw.Lambertian(rtw.CheckerTexture.new_with_colours(
            (0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.32))),
        rtw.Sphere(centres["checker"], 1.0, rtw.DiffuseLight(checker)),
        rtw.Sphere(centres["noise"], 1.0, rtw.DiffuseLight(rtw.NoiseTexture.new(4.0))),
        rtw.Sphere(centres["solid"], 1.0, rtw.DiffuseLight((7.0, 6.0, 5.0)))])
    lights = rtw.HittableList([rtw.Sphere(centres["noise"], 1.0, rtw.INVISIBLE)])
    soa = rtw.flatten(world, lights)
    rng = np.random.default_rng(23)
    rays = []
    for c in centres.values():
        for _ in range(24):                    # from a point around the sphere towards a point inside it
            o = np.array(c) + rng.normal(size=3) * 4.0
            o[1] = abs(o[1]) + 0.5
            aim = np.array(c) + rng.uniform(-0.6, 0.6, 3)
            rays.append((*o, *(aim - o)))
    for _ in range(12):                        # and onto the ground between them
        o = np.array((rng.uniform(-5, 5), 6.0, rng.uniform(-3, 3)))
        rays.append((*o, rng.uniform(-0.3, 0.3), -1.0, rng.uniform(-0.3, 0.3)))
    return soa, np.ascontiguousarray(np.array(rays, np.float64)), np.arange(len(rays)) + 5000


def hand_placed(name):
    """Hand-placed rays for the branches the sampled paths of `name` may not
    reach: (rays [n, 6], streams [n] -- the pixel index whose (SEED, pixel, 0)
    stream each ray's bounce draws from).  Expected answers: expect()."""
    rays = []
    if name == "plane+light":
        # the plane (y = 0, normal +y) is met only by rays that go its normal's way
        # (plane.rs: denom > EPSILON): from below, upwards, across many checker cells
        g = np.random.default_rng(31)
        for _ in range(80):
            rays.append((g.uniform(-9, 9), -g.uniform(0.5, 4), g.uniform(-9, 9), g.uniform(-1, 1), 1.0, g.uniform(-1, 1)))
    if name == "simple":
        # the three big spheres (glass at the origin, Lambertian at x = -4, metal at x = 4,
        # radius 1, centres at y = 1): straight down on each, grazing the glass, and from
        # inside the glass at angles beyond the critical one (total internal reflection)
        for cx in (0.0, -4.0, 4.0):
            for dx in (0.0, 0.3, 0.7, 0.95, 0.999):
                rays.append((cx + dx, 5.0, 0.0, 0.0, -1.0, 0.0))
        for off in (0.3, 0.75, 0.9, 0.97):
            rays.append((off, 1.0, 0.0, 0.0, 0.0, 1.0))        # from inside, off-centre: sin(incidence) = off
    return np.ascontiguousarray(np.array(rays, np.float64).reshape(-1, 6)), np.arange(len(rays)) + 1000


def expect(shader, rays, streams, seed=SEED, sample=0, states=False):
    """The bounces of these rays, ray k drawing from Rng(seed, streams[k], sample) from its
    start: the arrays of Bounces (rng0, rng1, event, emitted, weight, next, pdfs, what, front)."""
    out = dict(rng0=[], rng1=[], event=[], emitted=[], weight=[], next=[], pdfs=[], what=[], front=[], mtype=[],
               tex=[])
    for r, st in zip(rays, streams):
        o, d = tuple(map(float, r[:3])), tuple(map(float, r[3:]))
        g = R.Rng(seed, 0, sample)
        if states:
            g.s = [int(x) for x in st]         # the state itself
        else:
            g = R.Rng(seed, int(st), sample)
        out["rng0"].append(tuple(g.s))
        rec = shader.world.hit(o, d)
        b = shader.bounce(o, d, rec, g)
        out["rng1"].append(tuple(g.s))
        out["front"].append(True if rec is None else rec.front)
        out["mtype"].append(-1 if rec is None else shader.world.mat_type[rec.mat])
        out["tex"].append(-1 if rec is None else shader.tex_kind(rec))
        for k in ("event", "emitted", "weight", "next", "pdfs", "what"):
            out[k].append(b[k])
    res = {k: np.array(v, np.uint64) for k, v in out.items() if k in ("rng0", "rng1")}
    res.update({k: np.array(out[k], np.float64) for k in ("emitted", "weight", "next", "pdfs")})
    res["mtype"], res["tex"] = np.array(out["mtype"]), np.array(out["tex"])
    res["event"], res["what"], res["front"] = np.array(out["event"], np.int32), np.array(out["what"]), np.array(out["front"])
    return res


def expect_from_states(shader, rays, rng0):
    """expect() for rays whose bounces start from the given xoshiro256++ states [n, 4]"""
    return expect(shader, rays, rng0, states=True)
