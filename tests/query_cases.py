"""Rays and expected answers for the ray-query tests (tests/test_gpu_query*.py),
all from the oracle (O.trace_path / O.world_hit) and the independent
restatement (tests/indep/restate.py) -- nothing here touches the GPU, and each
reference is computed once per test run and shared.

Path segments are the hard rays: origins on surfaces, self-intersection
re-hits at t ~ 1e-16, grazing exits."""
import functools

import numpy as np

import ray_tracing_weekend_amd as rtw
from indep import restate as R
from oracle import oracle as O

EPS = 2.220446049250313e-16
SEED = 7


def oracle_cam(builder, W, H, spp, depth):
    b = builder.with_image_width(W).with_image_height(H).with_samples_per_pixel(spp).with_max_depth(depth)
    raw = b.raw
    kw = {}
    for name in ("background", "vfov", "lookfrom", "lookat", "vup", "defocus_angle", "focus_dist"):
        v = getattr(raw, name)
        kw[name] = tuple(v) if not isinstance(v, (int, float)) else v
    return O.camera_build(image_width=W, image_height=H, samples_per_pixel=spp, max_depth=depth, **kw)


def cut_spheres(soa, n):
    """The scene with its first n spheres only."""
    d = dict(soa.__dict__)
    d["spheres"], d["sphere_mat"] = soa.spheres[:n].copy(), soa.sphere_mat[:n].copy()
    return rtw.SceneSoA(**d)


def with_lights(soa, lights, flags=0):
    """The scene with a light list of these spheres only."""
    d = dict(soa.__dict__)
    d["lights"] = np.ascontiguousarray(lights, np.float64).reshape(-1, 4)
    d["light_quads"], d["light_kinds"], d["n_light_other"] = np.zeros((0, 9)), None, 0
    d["light_flags"] = flags
    return rtw.SceneSoA(**d)


def rays_at_lights(soa, per_light=4, seed=17):
    """Rays from points around the scene towards (and a little beside) each light
    sphere: most of them have a light pdf > 0."""
    rng = np.random.default_rng(seed)
    out = []
    for L in np.asarray(soa.lights).reshape(-1, 4):
        for _ in range(per_light):
            o = np.array([rng.uniform(-12, 12), rng.uniform(0.5, 6), rng.uniform(-12, 12)])
            aim = L[:3] + rng.uniform(-1, 1, 3) * 0.7 * abs(L[3])
            out.append(list(o) + list(aim - o))
    return np.ascontiguousarray(out, np.float64)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(SceneSoA, CameraBuilder) of a named case."""
    if name == "simple":
        return rtw.scenes.simple_soa(0x5EED0001, 11)
    if name == "simple63":
        # its 63 small spheres sit at x in [-11, -8] on the far side of the field: the
        # camera is turned towards them, so that the sampled paths meet them
        soa, b = rtw.scenes.simple_soa(0x5EED0001, 11)
        return cut_spheres(soa, 63), b.with_lookat((-9.5, 0.2, 0.0)).with_vfov(30.0)
    if name == "lights64":      # the scene's first 64 spheres as its light list
        soa, b = rtw.scenes.simple_soa(0x5EED0001, 11)
        return with_lights(soa, soa.spheres[:64]), b
    return rtw.scenes.named_soa(name)


def object_tables(soa):
    """(material id, primitive kind) by object id: planes, quads, cuboids, spheres."""
    mats = [np.asarray(a, np.int64).reshape(-1) for a in (soa.plane_mat, soa.quad_mat, soa.box_mat, soa.sphere_mat)]
    kinds = [np.full(len(m), k, np.int64) for k, m in enumerate(mats)]
    return np.concatenate(mats), np.concatenate(kinds)


class Segments:
    """The segments of oracle paths: rays [n, 6], the id and t trace_path met, the
    previous segment's id (-2 for a primary ray), and O.world_hit's record."""

    def __init__(self, name, pixels, samples, W=40, H=24, depth=50):
        soa, b = scene(name)
        self.soa, self.sc = soa, O.Scene(**soa.__dict__)
        self.cam = oracle_cam(b.copy(), W, H, max(samples) + 1, depth)
        rays, ids, ts, prev = [], [], [], []
        for (i, j) in pixels:
            for s in samples:
                _, path = O.trace_path(self.cam, self.sc, SEED, i, j, s, cap=depth + 1)
                last = -2
                for row in path:
                    rays.append(row[:6])
                    ids.append(int(row[6]))
                    ts.append(row[7])
                    prev.append(last)
                    last = int(row[6])
        self.rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        self.ids, self.t, self.prev = np.array(ids, np.int64), np.array(ts, np.float64), np.array(prev, np.int64)
        n = len(self.rays)
        self.hits = np.zeros((n, 9))       # {t, p, normal, -, -} of O.world_hit (u, v: restate's, see uv())
        self.front = np.zeros(n, np.int64)
        self.wid = np.zeros(n, np.int64)
        for k in range(n):
            idk, t, p, nrm, front = O.world_hit(self.sc, self.rays[k, :3], self.rays[k, 3:])
            self.wid[k] = idk
            if idk >= 0:
                self.hits[k, 0], self.hits[k, 1:4], self.hits[k, 4:7], self.front[k] = t, p, nrm, int(front)
        self.mat, self.kind = object_tables(soa)

    @property
    def rehits(self):
        return int(((self.ids >= 0) & (self.ids == self.prev)).sum())

    @property
    def misses(self):
        return int((self.ids < 0).sum())

    def uv(self):
        """restate.World.hit's (u, v) per segment (NaN rows for misses) and, for
        sphere hits, the angles atan2(-n.z, n.x) and acos(n.y) they were divided from."""
        import math
        w = R.World(self.soa)
        out = np.full((len(self.rays), 4), np.nan)
        for k, r in enumerate(self.rays):
            rec = w.hit(tuple(r[:3]), tuple(r[3:]))
            if rec is None:
                continue
            out[k, 0], out[k, 1] = rec.u, rec.v
            if self.kind[self.ids[k]] == 3:
                s = self.soa.spheres[self.ids[k] - (len(self.mat) - len(self.soa.sphere_mat))]
                n = R.divs(R.sub(rec.p, tuple(s[:3])), float(s[3]))
                out[k, 2] = math.atan2(-n[2], n[0])
                out[k, 3] = math.acos(n[1]) if -1.0 <= n[1] <= 1.0 else np.nan
        return out


GRID_SIMPLE = tuple((i, j) for i in range(0, 40, 3) for j in range(0, 24, 3))
GRID_COARSE = tuple((i, j) for i in range(0, 40, 5) for j in range(0, 24, 4))


@functools.lru_cache(maxsize=None)
def segments(name):
    if name == "simple":
        return Segments(name, GRID_SIMPLE, (0, 1))
    if name == "simple63":
        return Segments(name, GRID_FULL, (0, 1))
    if name in ("simple_transform", "simple_light"):
        # small objects in a wide view: every pixel, one sample
        return Segments(name, GRID_FULL, (0,))
    return Segments(name, GRID_COARSE, (0, 1))


GRID_FULL = tuple((i, j) for i in range(0, 40) for j in range(0, 24))


def camera_rays(name, W, H):
    """The primary rays through the pixel centres of the case's camera, [H * W, 6]."""
    _, b = scene(name)
    cam = oracle_cam(b.copy(), W, H, 1, 1)
    c, p00 = np.array(cam.center[:]), np.array(cam.pixel00_loc[:])
    du, dv = np.array(cam.pixel_delta_u[:]), np.array(cam.pixel_delta_v[:])
    jj, ii = np.mgrid[0:H, 0:W]
    tgt = p00 + ii[..., None] * du + jj[..., None] * dv
    rays = np.concatenate([np.broadcast_to(c, tgt.shape), tgt - c], -1).reshape(-1, 6)
    return np.ascontiguousarray(rays)


def lambertian_bounces(seg):
    """(point, direction) pairs of the Lambertian bounces of oracle paths: the
    origin and direction of every segment that follows a hit on a Lambertian
    surface -- the arguments of the integrator's lights.pdf_value."""
    lam = np.asarray(seg.soa.mat_type)[seg.mat] == rtw.RTW_LAMBERTIAN
    keep = (seg.prev >= 0) & lam[np.maximum(seg.prev, 0)]
    return np.ascontiguousarray(seg.rays[keep])
