"""The cases of tests/test_gpu_f32_records.py: per group the inputs an f32 query
is sent, and the two CPU evaluations of tests/f32_forms.py on them -- the law
(float64) and the calibration (float32).  Nothing here touches the GPU; each
evaluation is computed once per test run and shared.  tests/test_f32_forms_host.py
checks on the CPU that the calibration alone takes another discrete decision
than the law on at most 0.25 % of every group.

A case names its real-valued outputs (REALS: key, whether it is a vector taken
as a whole, and the floor of its relative error), its integer outputs (INTS),
and the margins of its discrete decisions (MARGINS: keys whose value in the law
is the distance of the row from a decision).  A row is NEAR A DECISION when one
of its margins in the law is at most 4 x the 99th percentile of the calibration's
error in that margin over the group (the kernel's allowance against the calibration,
see the GPU test).  Only such rows may be left out of the value comparison."""
import functools

import numpy as np

import f32_forms as FF
import nee_cases as N
import path_cases as P
import query_cases as Q
from oracle import oracle as O

ALLOW = 4.0                       # kernel error / calibration error, per statistic
SEED = 7


def _cached(fn):
    return functools.lru_cache(maxsize=None)(fn)


class Case:
    min_rows = 1000
    REALS, INTS, MARGINS = (), (), ()

    def evaluate(self, dtype):
        raise NotImplementedError

    def law(self):
        if not hasattr(self, "_law"):
            self._law = self.evaluate(np.float64)
        return self._law

    def calibration(self):
        if not hasattr(self, "_cal"):
            self._cal = self.evaluate(np.float32)
        return self._cal

    def margins(self, out):
        """[n, len(MARGINS)] of a dict's margins (a list's margin: its smallest entry)"""
        cols = []
        for k in self.MARGINS:
            m = np.asarray(out[k], np.float64)
            cols.append(m.min(1) if m.ndim == 2 and m.shape[1] else (m if m.ndim == 1 else np.full(len(m), np.inf)))
        return np.stack(cols, 1) if cols else np.zeros((self.n, 0))

    def thresholds(self):
        """per margin: ALLOW x the 99th percentile of the calibration's error in it over the group
        (relative above 1) -- not the largest: one ill-conditioned row must not widen it for all"""
        a, b = self.margins(self.law()), self.margins(self.calibration())
        both = np.isfinite(a) & np.isfinite(b)
        with np.errstate(all="ignore"):
            err = np.where(both, np.abs(a - b) / np.maximum(1.0, np.abs(a)), 0.0)
        return ALLOW * np.percentile(err, 99, axis=0) if len(err) else np.zeros(a.shape[1])

    def near_decision(self):
        a = self.margins(self.law())
        return (np.abs(a) <= self.thresholds()[None, :]).any(1)

    def differ(self, law, other):
        """rows whose observable discrete outputs differ"""
        d = np.zeros(self.n, bool)
        for k in self.INTS:
            x, y = np.asarray(law[k]), np.asarray(other[k])
            d |= (x != y) if x.ndim == 1 else (x != y).any(1)
        return d

    def disagree(self, law, other):
        return self.differ(law, other), self.near_decision()

    def valued(self, key):
        """the rows on which output `key` carries a value to compare (default: all)"""
        return np.ones(self.n, bool)


# ------------------------------------------------------------------ hit_rays
class HitCase(Case):
    REALS = (("t", False, "own"), ("p", True, "origin"), ("normal", True, 1.0), ("u", False, "uv"), ("v", False, "uv"))
    INTS = ("id", "mat", "front", "kind")
    MARGINS = ("gap", "near", "edge", "facing")

    def __init__(self, soa, rays, form, min_rows=1000):
        self.soa, self.rays = soa, np.ascontiguousarray(rays, np.float32)
        self.form, self.n, self.min_rows = form, len(rays), min_rows
        self.S = FF.stage(soa, np.float32)

    def evaluate(self, dtype):
        return FF.closest_hit(self.S, self.rays, dtype, True, self.form)

    def differ(self, law, other):
        d = Case.differ(self, law, other)
        # a cuboid's face is a decision too: it shows in the (object-space) normal
        return d | (np.abs(np.asarray(law["normal"], np.float64) - np.asarray(other["normal"], np.float64)).max(1) > 0.5)

    def valued(self, key):
        return self.law()["id"] >= 0           # a miss is zeros: its integer outputs are compared, no value

    def floor(self, what):
        if what == "origin":
            return np.sqrt((self.rays[:, :3].astype(np.float64) ** 2).sum(1))
        if what == "uv":          # a plane's (u, v) are coordinates of the point; every other kind's are O(1)
            on_plane = self.law()["kind"] == FF.PRIM_PLANE
            return np.where(on_plane, np.maximum(1.0, self.floor("origin")), 1.0)
        return what


BIG_Z = 4.0          # the three big spheres stand aside of the pole, at z = BIG_Z


@_cached
def ground_sphere_scene():
    """The Book-1 layout with its ground as a SPHERE, (0, -1000, 0) of radius 1000 (scenes::simple
    of this build stages the ground as a plane): that sphere and the three big ones -- glass,
    Lambertian, Metal, radius 1 -- moved to z = BIG_Z so that rays at the pole pass them by."""
    import ray_tracing_weekend_amd as rtw
    world = rtw.HittableList([
        rtw.Sphere((0.0, -1000.0, 0.0), 1000.0, rtw.Lambertian((0.5, 0.5, 0.5))),
        rtw.Sphere((0.0, 1.0, BIG_Z), 1.0, rtw.Dialectric(1.5)),
        rtw.Sphere((-4.0, 1.0, BIG_Z), 1.0, rtw.Lambertian((0.4, 0.2, 0.1))),
        rtw.Sphere((4.0, 1.0, BIG_Z), 1.0, rtw.Metal((0.7, 0.6, 0.5), 0.0))])
    lights = rtw.HittableList([rtw.Sphere((0.0, 12.0, 0.0), 2.0, rtw.INVISIBLE)])
    return rtw.flatten(world, lights)


def pole_rays():
    """1024 rays onto the r = 1000 ground sphere of ground_sphere_scene() within 0.5 of its pole
    from y in [1, 6], 256 onto the tops and bottoms of the three big spheres (from inside the
    glass one too, for the back face), and the ray straight down the axis: 1281.
    A direction is (aim - origin) times a factor in [0.5, 2]: with the bare difference the hit
    is at t = 1 exactly, c = -2 hb - a and the discriminant hb^2 - a c = (hb + a)^2 is a perfect
    square -- correctly rounded f32 arithmetic then returns t to 4e-8 at the median where any
    other length of the same ray gives 1e-5 (the cancellation of -hb - sqrt(disc)), and the
    calibration would not be one of the form."""
    g = np.random.default_rng(41)
    rays = []
    for _ in range(1024):
        aim = np.array((g.uniform(-0.5, 0.5), 0.0, g.uniform(-0.5, 0.5)))
        aim[1] = np.sqrt(1e6 - aim[0] ** 2 - aim[2] ** 2) - 1000.0
        o = np.array((aim[0] + g.uniform(-1, 1), g.uniform(1.0, 6.0), aim[2] + g.uniform(-1, 1)))
        rays.append((*o, *((aim - o) * g.uniform(0.5, 2.0))))
    for k in range(256):
        cx = (0.0, -4.0, 4.0)[k % 3]
        top = (k // 3) % 2 == 0
        aim = np.array((cx + g.uniform(-0.02, 0.02), 2.0 if top else 0.0, BIG_Z + g.uniform(-0.02, 0.02)))
        if cx == 0.0 and k % 4 == 0:                           # from inside the glass sphere
            o = np.array((cx + g.uniform(-0.3, 0.3), 1.0 + g.uniform(-0.3, 0.3), BIG_Z + g.uniform(-0.3, 0.3)))
        elif top:
            o = np.array((cx + g.uniform(-0.5, 0.5), g.uniform(3.0, 6.0), BIG_Z + g.uniform(-0.5, 0.5)))
        else:                                                  # towards the bottom, from beside the sphere
            o = np.array((cx + g.choice((-1.0, 1.0)) * g.uniform(1.5, 3.0), g.uniform(0.05, 0.3),
                          BIG_Z + g.uniform(-1.0, 1.0)))
        rays.append((*o, *((aim - o) * g.uniform(0.5, 2.0))))
    rays.append((0.0, 3.0, 0.0, 0.0, -1.0, 0.0))
    return np.array(rays)


def aimed_rays(soa, n, seed):
    """rays from around the scene towards points on (and a little beside) its quads and cuboids"""
    g = np.random.default_rng(seed)
    S = FF.stage(soa, np.float64)
    targets = []
    for Qd in S.quads:
        targets.append(lambda Qd=Qd: Qd["q"] + g.uniform(-0.1, 1.1) * Qd["u"] + g.uniform(-0.1, 1.1) * Qd["v"])
    for B in S.boxes:
        targets.append(lambda B=B: B["lo"] + g.uniform(-0.1, 1.1, 3) * (B["hi"] - B["lo"]))
    rays = []
    for k in range(n):
        aim = targets[k % len(targets)]()
        o = np.array((g.uniform(-9, 9), g.uniform(0.3, 12), g.uniform(-9, 9)))
        rays.append((*o, *(aim - o)))
    return np.array(rays)


def upward_rays():
    """path_cases.hand_placed("plane+light")'s rays from below the plane, tiled with jitter to 1000"""
    base = P.hand_placed("plane+light")[0]
    g = np.random.default_rng(43)
    reps = -(-1000 // len(base))
    rays = np.concatenate([base] * reps)[:1000]
    return rays + g.uniform(-0.05, 0.05, rays.shape) * (np.arange(len(rays))[:, None] >= len(base))


# ----------------------------------------------------------------- light_pdf
class PdfCase(Case):
    REALS = (("pdf", False, "own"),)
    MARGINS = ("margin",)

    def __init__(self, soa, rays, robust, tuning=None, min_rows=1000):
        self.soa, self.rays = soa, np.ascontiguousarray(rays, np.float32)
        self.robust, self.tuning, self.n, self.min_rows = robust, dict(tuning or {}), len(rays), min_rows
        self.S = FF.stage(soa, np.float32)

    def evaluate(self, dtype):
        return FF.lights_pdf(self.S, self.rays, dtype, True, self.robust)

    def differ(self, law, other):
        return (law["hits"] != other["hits"]).any(1) if "hits" in other else np.zeros(self.n, bool)

    def floor(self, what):
        return what


def far_lights():
    """three sphere lights of radius 0.5 at distances 1e2, 1e3, 1e4 from the origins (points
    within 2 of the scene's origin), and 1000 rays aimed inside their cones"""
    soa, _ = Q.scene("simple")
    dirs = np.array(((0.6, 0.64, 0.48), (-0.48, 0.8, 0.36), (0.0, 0.6, -0.8)))
    lights = [(*(d * r), 0.5) for d, r in zip(dirs, (1e2, 1e3, 1e4))]
    soa = Q.with_lights(soa, lights)
    g = np.random.default_rng(47)
    rays = []
    for k in range(1000):
        L = np.array(lights[k % 3])
        o = g.uniform(-2.0, 2.0, 3)
        off = g.normal(size=3)
        off *= 0.4 * g.uniform(0.0, 1.0) / np.linalg.norm(off)       # within 0.4 of the centre: inside the cone
        rays.append((*o, *((L[:3] + off - o) * g.uniform(0.5, 2.0))))
    return soa, np.array(rays)


def inside_lights():
    """origins inside the lights of scenes::simple: the pdf is NaN by arithmetic (sqrt(1 - x), x > 1)"""
    soa, _ = Q.scene("simple")
    g = np.random.default_rng(53)
    rays = []
    li = np.asarray(soa.lights).reshape(-1, 4)
    for k in range(65):
        L = li[k % len(li)]
        d = g.normal(size=3)
        rays.append((*(L[:3] + 0.4 * abs(L[3]) * d / np.linalg.norm(d)), *g.normal(size=3)))
    return soa, np.array(rays)


# -------------------------------------------------------------- light_sample
class SampleCase(Case):
    REALS = (("dir", True, "own"), ("pdf", False, "own"))
    INTS = ("index",)
    MARGINS = ("margin",)
    first_stream, sample = 1000, 3

    def __init__(self, soa, origins, robust, min_rows=1000):
        self.soa, self.origins = soa, np.ascontiguousarray(origins, np.float32)
        self.robust, self.n, self.min_rows = robust, len(origins), min_rows
        self.S = FF.stage(soa, np.float32)

    def evaluate(self, dtype):
        return FF.light_sample(self.S, self.origins, SEED, self.first_stream, self.sample, dtype, True, True,
                               self.robust)

    def floor(self, what):
        return what


def tiled_points(name, n=1200):
    soa, pts = N.bounce_points(name)
    return soa, np.concatenate([pts] * (-(-n // len(pts))))[:n]


# --------------------------------------------------------------- camera_rays
class CameraCase(Case):
    REALS = (("origin", True, 1.0), ("direction", True, "own"))
    INTS = ("state",)
    MARGINS = ("disk",)
    W, H = 64, 40

    def __init__(self, name, defocus_angle=None):
        _, b = Q.scene(name)
        if defocus_angle is not None:
            b = b.copy().with_defocus_angle(defocus_angle)
        self.cam = b.copy().with_image_width(self.W).with_image_height(self.H).with_samples_per_pixel(2) \
                    .with_max_depth(50).build()
        ocam = Q.oracle_cam(b.copy(), self.W, self.H, 2, 50)
        self.camd = O.camera_dict(ocam)
        self.pixels = np.concatenate([np.arange(self.W * self.H), [0]])
        self.n = 2 * len(self.pixels)

    def evaluate(self, dtype):
        rays, states, disk = [], [], []
        F = FF.Forms(dtype)
        U = FF.Uniforms(F, True)
        for s in (0, 1):
            r, st = FF.camera_rays(self.camd, SEED, self.pixels, s, dtype)
            rays.append(r)
            states.append(st)
            # the margin of the unit disk's rejection test, over the tries a stream makes
            m = np.full(len(self.pixels), np.inf)
            if self.camd["defocus_angle"] > FF.EPS:
                g = FF.rng_seed(SEED, self.pixels.astype(np.uint64), s)
                FF.rng_next(g), FF.rng_next(g)
                pend = np.ones(len(g), bool)
                while pend.any():
                    x = F.two * U.std(FF.rng_next(g, pend)) - F.one
                    z = F.two * U.std(FF.rng_next(g, pend)) - F.one
                    l2 = (x * x + z * z).astype(np.float64)
                    m = np.where(pend, np.minimum(m, np.abs(l2 - 1.0)), m)
                    pend &= ~(l2 < 1)
            disk.append(m)
        rays = np.concatenate(rays)
        return dict(origin=rays[:, :3], direction=rays[:, 3:], state=np.concatenate(states), disk=np.concatenate(disk))

    def floor(self, what):
        return what


# ---------------------------------------------------------------- shade_rays
WHATS = ("metal", "metal absorbed", "refraction", "schlick reflection", "total internal reflection", "light sphere",
         "light quad", "cosine lobe", "diffuse light")


class ShadeBatch:
    """One scene's rows: rays and stream states; the records come from the f32 context under
    test (the GPU test) or from the calibration's own closest hit (the CPU check)."""

    def __init__(self, name, soa, rays, states, form):
        self.name, self.soa = name, soa
        self.rays, self.states = np.ascontiguousarray(rays, np.float32), np.ascontiguousarray(states, np.uint64)
        self.form, self.robust = form, form == "robust"
        self.S = FF.stage(soa, np.float32)

    def cpu_records(self):
        h = FF.closest_hit(self.S, self.rays, np.float32, True, self.form)
        hits = np.concatenate([h["t"][:, None], h["p"], h["normal"], h["u"][:, None], h["v"][:, None]], 1)
        ids = np.stack([h["id"], h["mat"], h["front"], h["kind"]], 1)
        return hits.astype(np.float32), ids.astype(np.int32)

    def evaluate(self, dtype, hits, ids):
        return FF.shade(self.S, self.rays, hits, ids, self.states, dtype, True, True, self.robust)


def _fresh(n, tile):
    return FF.rng_seed(SEED + 100, np.arange(n, dtype=np.uint64), tile)


RARE = {"metal absorbed": 10, "light quad": 2, "schlick reflection": 2}     # branches a fresh stream often leaves


def _replicated(rays, states, what, target=1100):
    """rows repeated so that every branch in `what` reaches about `target` rows, each repeat on
    a fresh stream (the records are inputs: rays may repeat)"""
    out_r, out_s = [rays], [states]
    for w in np.unique(what):
        rows = np.flatnonzero(what == w)
        reps = min(-(-target * RARE.get(str(w), 1) // len(rows)) - 1, 4000)
        for t in range(reps):
            out_r.append(rays[rows])
            out_s.append(_fresh(len(rows), 1000 * (1 + list(np.unique(what)).index(w)) + t))
    return np.concatenate(out_r), np.concatenate(out_s)


@_cached
def shade_batches():
    out = []
    sources = []
    for name in ("simple", "cornell_box", "lights64", "plane+light", "perlin_spheres+light"):
        b = P.bounces(name)
        sources.append((name, b.soa, b.rays, b.rng0))
    soa, rays, streams = P.textured_lights()
    sources.append(("textured_lights", soa, rays, FF.rng_seed(P.SEED, streams.astype(np.uint64), 0)))
    for name in ("simple", "plane+light"):      # (the sampled paths of plane+light never meet its one-sided plane)
        rays, streams = P.hand_placed(name)
        sources.append((name + "/hand", P.scene(name)[0], rays, FF.rng_seed(P.SEED, streams.astype(np.uint64), 0)))
    for name, soa, rays, states in sources:
        batch = ShadeBatch(name, soa, rays, states, "robust" if name.startswith(("simple", "lights64")) else "u")
        hits, ids = batch.cpu_records()
        what = batch.evaluate(np.float32, hits, ids)["what"]
        keep = np.isin(what, WHATS)
        if not keep.any():
            continue
        r, s = _replicated(batch.rays[keep], batch.states[keep], what[keep],
                           target=1100 if name in ("simple", "cornell_box", "simple/hand") else 300)
        if len(r) % 256 == 0:
            r, s = r[:-1], s[:-1]
        out.append(ShadeBatch(name, soa, r, s, batch.form))
    # Metal with fuzz 1: the inversion vector dominates the direction
    b = P.bounces("simple")
    soa = b.soa
    d = dict(soa.__dict__)
    mp = np.array(soa.mat_params, np.float64).reshape(-1, 5).copy()
    mp[np.asarray(soa.mat_type).reshape(-1) == FF.METAL, 3] = 1.0
    d["mat_params"] = mp
    import ray_tracing_weekend_amd as rtw
    fz = rtw.SceneSoA(**d)
    metal = b.mtype == FF.METAL
    r, s = _replicated(b.rays[metal], b.rng0[metal], np.full(int(metal.sum()), "metal"), target=1300)
    out.append(ShadeBatch("simple/fuzz1", fz, r, s, "robust"))
    return tuple(out)


SHADE_REALS = (("next_p", True, "origin"), ("next_d", True, "own"), ("weight", True, "own"), ("emitted", True, "own"),
               ("pdf", False, "own"), ("lpdf", False, "own"), ("spdf", False, "own"))


def pooled(outs, which):
    """pool per-batch dicts (law, calibration or kernel) over this case's rows; `which`:
    per batch the row mask"""
    keys = ("next_p", "next_d", "weight", "emitted", "pdf", "lpdf", "spdf", "event", "state", "margin",
            "light_margin", "origin")
    res = {k: [] for k in keys}
    for o, m in zip(outs, which):
        if not m.any():
            continue
        res["next_p"].append(o["next"][m, :3])
        res["next_d"].append(o["next"][m, 3:])
        for k, col in (("pdf", 0), ("lpdf", 1), ("spdf", 2)):
            res[k].append(o["pdfs"][m, col])
        for k in ("weight", "emitted", "event", "state"):
            res[k].append(o[k][m])
        res["margin"].append(o["margin"][m] if "margin" in o else np.zeros(int(m.sum())))
        lm = o.get("light_margin")
        res["light_margin"].append(np.full(int(m.sum()), np.inf) if lm is None or lm.shape[1] == 0
                                   else np.asarray(lm, np.float64)[m].min(1))
        res["origin"].append(o["origin"][m])
    return {k: np.concatenate(v) for k, v in res.items()}


def shade_setup(records=None):
    """(batches, law outputs, calibration outputs, per `what` the row masks).  records: per batch
    (hits, ids) of the f32 context under test; None: the calibration's own closest hit."""
    batches = shade_batches()
    if records is None:
        records = _cpu_records()
    law, cal = [], []
    for b, (h, i) in zip(batches, records):
        for dtype, dst in ((np.float64, law), (np.float32, cal)):
            o = b.evaluate(dtype, h, i)
            o["origin"] = np.sqrt((np.asarray(h, np.float64)[:, 1:4] ** 2).sum(1))
            dst.append(o)
    return batches, law, cal


@_cached
def _cpu_records():
    return tuple(b.cpu_records() for b in shade_batches())


@_cached
def _cpu_shade():
    return shade_setup()


class ShadeGroup(Case):
    """One branch of the bounce (what), over every batch (fuzz1: the fuzz-1 batch alone)"""
    REALS = SHADE_REALS
    INTS = ("event", "state")
    MARGINS = ("margin", "light_margin")

    def __init__(self, what, fuzz1=False):
        self.what, self.fuzz1 = what, fuzz1

    def use(self, batches, law, cal):
        pick = [(b.name == "simple/fuzz1") == self.fuzz1 for b in batches]
        self.masks = [(o["what"] == self.what) & p for o, p in zip(law, pick)]
        self._law, self._cal = pooled(law, self.masks), pooled(cal, self.masks)
        self._origin = self._law["origin"]
        self.n = len(self._origin)
        self.pool = lambda outs: pooled(outs, self.masks)
        return self

    def floor(self, what):
        return self._origin if what == "origin" else what


# ------------------------------------------------------------------- the table
def _simple_camera_rays():
    return Q.scene("simple")[0], Q.camera_rays("simple", 120, 80)


HIT_GROUPS = {
    "hit/simple/u": lambda: HitCase(*_simple_camera_rays(), "u"),
    "hit/simple/robust": lambda: HitCase(*_simple_camera_rays(), "robust"),
    "hit/poles/u": lambda: HitCase(ground_sphere_scene(), pole_rays(), "u"),
    "hit/poles/robust": lambda: HitCase(ground_sphere_scene(), pole_rays(), "robust"),
    "hit/cornell_box": lambda: HitCase(Q.scene("cornell_box")[0], _jittered_camera_rays("cornell_box", 60, 60), "u"),
    "hit/simple_transform": lambda: HitCase(Q.scene("simple_transform")[0], np.concatenate(
        [Q.camera_rays("simple_transform", 60, 60), aimed_rays(Q.scene("simple_transform")[0], 2501, 59)]), "u"),
    "hit/cornell_box/aimed": lambda: HitCase(Q.scene("cornell_box")[0], _cornell_aimed(), "u"),
    "hit/plane+light": lambda: HitCase(P.scene("plane+light")[0], upward_rays(), "u"),
}


def _jittered_camera_rays(name, W, H):
    """Camera::get_ray of sample 0 of every pixel (the rays through the pixel centres of this
    symmetric, axis-aligned scene run along its quads' borders: decisions, not values)"""
    import feature_cases as F
    _, ocam = F.cameras(name, W, H)
    return P.camera_rays(O.camera_dict(ocam), SEED, range(W * H), 0)[0]


def _cornell_aimed():
    soa, _ = Q.scene("cornell_box")
    g = np.random.default_rng(61)
    S = FF.stage(soa, np.float64)
    B = S.boxes[0]
    rays = []
    for _ in range(1101):
        aim = B["lo"] + g.uniform(-0.05, 1.05, 3) * (B["hi"] - B["lo"])
        o = np.array((g.uniform(20, 535), g.uniform(20, 535), g.uniform(-700, 200)))
        rays.append((*o, *(aim - o)))
    return np.array(rays)


def _pdf_rays(name, per_light):
    seg = Q.segments("simple")
    soa = Q.scene(name)[0]
    rays = np.concatenate([Q.lambertian_bounces(seg), Q.rays_at_lights(soa, per_light)])
    return soa, rays[:-1] if len(rays) % 256 == 0 else rays


def _cornell_pdf_rays():
    """the Lambertian next rays of cornell_box's paths and, from the same shading points, rays
    aimed at and beside its quad light: 1001 distinct rays for the mixed list"""
    soa = Q.scene("cornell_box")[0]
    b = Q.lambertian_bounces(Q.segments("cornell_box"))
    q = np.asarray(soa.light_quads, np.float64).reshape(-1, 9)[0]
    g = np.random.default_rng(67)
    rays = [tuple(r) for r in b]
    k = 0
    while len(rays) < 1001:
        o = b[k % len(b), :3]
        aim = q[:3] + g.uniform(-0.25, 1.25) * q[3:6] + g.uniform(-0.25, 1.25) * q[6:9]
        rays.append((*o, *((aim - o) * g.uniform(0.5, 2.0))))
        k += 1
    rays = np.array(rays)
    assert len(np.unique(rays.astype(np.float32), axis=0)) == len(rays)
    return rays


PDF_GROUPS = {
    "pdf/simple": lambda: PdfCase(*_pdf_rays("simple", 50), False),
    "pdf/simple/robust": lambda: PdfCase(*_pdf_rays("simple", 50), True),
    "pdf/lights64/grid": lambda: PdfCase(*_pdf_rays("lights64", 14), True, {}),
    "pdf/lights64/light_bvh": lambda: PdfCase(*_pdf_rays("lights64", 14), True, {"light_grid": 0}),
    "pdf/lights64/linear": lambda: PdfCase(*_pdf_rays("lights64", 14), True, {"light_bvh_min": 1 << 20}),
    "pdf/cornell_box": lambda: PdfCase(Q.scene("cornell_box")[0], _cornell_pdf_rays(), False),
    "pdf/far": lambda: PdfCase(*far_lights(), True),
    "pdf/inside": lambda: PdfCase(*inside_lights(), True, min_rows=65),
}

SAMPLE_GROUPS = {
    "sample/simple": lambda: SampleCase(*tiled_points("simple"), True),
    "sample/lights64": lambda: SampleCase(*tiled_points("lights64"), True),
    "sample/cornell_box": lambda: SampleCase(*tiled_points("cornell_box"), False),
    "sample/far": lambda: SampleCase(far_lights()[0], far_lights()[1][:, :3], True),
}

CAMERA_GROUPS = {
    "camera/simple": lambda: CameraCase("simple"),
    "camera/simple_defocus": lambda: CameraCase("simple", 0.6),       # the Book-1 final scene's defocus_angle
}

SHADE_GROUPS = {"shade/" + w: (lambda w=w: ShadeGroup(w)) for w in WHATS}
SHADE_GROUPS["shade/metal/fuzz1"] = lambda: ShadeGroup("metal", fuzz1=True)

ALL = {**HIT_GROUPS, **PDF_GROUPS, **SAMPLE_GROUPS, **CAMERA_GROUPS,
       **{k: (lambda f=f: f().use(*_cpu_shade())) for k, f in SHADE_GROUPS.items()}}
GROUPS = tuple(ALL)


@_cached
def case(group):
    return ALL[group]()
