"""Expected feature buffers (rtw_render_features) for tests/test_features_host.py
and tests/test_gpu_features.py, from the oracle and the independent restatement
alone -- nothing here touches the GPU, and each expectation is computed once
per test run and shared.

For every (pixel, sample): the first row of O.trace_path is the primary ray,
the id and the t the oracle's render meets; O.world_hit gives the point, the
normal and the front face; restate.World.hit the (u, v); O.texture_colour the
colour of a textured material, mat_params the others.  The fold is the
sequential f64 sum in a plain loop."""
import functools
import math

import numpy as np

import query_cases as Q
import ray_tracing_weekend_amd as rtw
from indep import restate as R
from oracle import oracle as O

SEED = 7
W, H, SAMPLES = 40, 24, 4
CHANNELS = 8
# scenes whose expectation another seed serves better would be listed here: {name: seed}
SEED_OF = {}


def scene(name):
    """(SceneSoA, CameraBuilder) of a named case: tests/query_cases.py's, and
      cornell_box        from inside the box, low at the right wall looking up and across:
                         query_cases' camera in front of the box never meets the cuboid with
                         a primary ray (cornell_box_front keeps that camera);
      simple_defocus     `simple` through a wide aperture (the builders above have none)."""
    if name == "cornell_box":
        soa, b = Q.scene("cornell_box")
        return soa, b.copy().with_lookfrom((540.0, 100.0, 100.0)).with_lookat((400.0, 300.0, 300.0)).with_vfov(70.0)
    if name == "cornell_box_front":
        return Q.scene("cornell_box")
    if name == "simple_defocus":
        soa, b = Q.scene("simple")
        return soa, b.copy().with_defocus_angle(2.0).with_focus_dist(10.0)
    return Q.scene(name)


def cameras(name, width, height, spp=SAMPLES, depth=50):
    """(rtw Camera, oracle camera) of the case's builder at this size."""
    _, b = scene(name)
    cam = b.copy().with_image_width(width).with_image_height(height).with_samples_per_pixel(spp) \
           .with_max_depth(depth).build()
    return cam, Q.oracle_cam(b.copy(), width, height, spp, depth)


class Samples:
    """Per (pixel, sample) of a W x H image: the 8 features f[H, W, S, 8], the
    ids {object or -1, material} i[H, W, S, 2], the material kind (-1: a miss)
    and the primitive kind of the hit, and the distance of a checker texture's
    u / v * inv_scale from the nearest integer (inf where none is read)."""

    def __init__(self, name, width=W, height=H, n_samples=SAMPLES, seed=None):
        seed = SEED_OF.get(name, SEED) if seed is None else seed
        soa, _ = scene(name)
        self.name, self.seed, self.soa = name, seed, soa
        self.W, self.H, self.S = width, height, n_samples
        self.cam, self.ocam = cameras(name, width, height, n_samples)
        sc = O.Scene(**soa.__dict__)
        world = R.World(soa)
        mat_of, kind_of = Q.object_tables(soa)
        bg = tuple(float(x) for x in self.cam.background)
        self.f = np.zeros((height, width, n_samples, CHANNELS))
        self.i = np.zeros((height, width, n_samples, 2), np.int32)
        self.mtype = np.full((height, width, n_samples), -1, np.int64)
        self.kind = np.full((height, width, n_samples), -1, np.int64)
        self.checker_margin = np.full((height, width, n_samples), np.inf)
        self.world_hit_agrees = True
        for j in range(height):
            for i in range(width):
                for s in range(n_samples):
                    _, path = O.trace_path(self.ocam, sc, seed, i, j, s, cap=1)
                    row = path[0]
                    o, d = tuple(map(float, row[:3])), tuple(map(float, row[3:6]))
                    oid, t = int(row[6]), float(row[7])
                    if oid < 0:
                        self.f[j, i, s, :3] = bg
                        self.i[j, i, s] = (-1, 0)
                        continue
                    wid, wt, p, nrm, _front = O.world_hit(sc, o, d)
                    if wid != oid or wt != t:
                        self.world_hit_agrees = False
                    m = int(mat_of[oid])
                    mtype = int(soa.mat_type[m])
                    if mtype in (rtw.RTW_LAMBERTIAN, rtw.RTW_DIFFUSE_LIGHT):
                        if soa.mat_tex is not None:
                            rec = world.hit(o, d)
                            albedo = O.texture_colour(sc, int(soa.mat_tex[m]), rec.u, rec.v, p)
                            self.checker_margin[j, i, s] = _checker_margin(world, int(soa.mat_tex[m]), rec.u, rec.v)
                        else:
                            albedo = tuple(map(float, soa.mat_params[m][:3]))
                    elif mtype == rtw.RTW_METAL:
                        albedo = tuple(map(float, soa.mat_params[m][:3]))
                    elif mtype == rtw.RTW_DIELECTRIC:
                        albedo = (1.0, 1.0, 1.0)
                    else:
                        albedo = (0.0, 0.0, 0.0)
                    dist = t * math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                    self.f[j, i, s] = (*albedo, *nrm, dist, 1.0)
                    self.i[j, i, s] = (oid, m)
                    self.mtype[j, i, s], self.kind[j, i, s] = mtype, int(kind_of[oid])

    def fold(self, first=0, n=None, counts=None, onto=None):
        """The sums [H, W, 8] of the samples [first, min(first + n, counts)) of
        every pixel, added in order onto `onto` (zeros)."""
        n = self.S - first if n is None else n
        out = np.zeros((self.H, self.W, CHANNELS)) if onto is None else np.array(onto, np.float64)
        for j in range(self.H):
            for i in range(self.W):
                end = first + n if counts is None else min(first + n, int(counts[j, i]))
                assert end <= self.S, "the expectation holds fewer samples"
                for s in range(first, end):
                    for c in range(CHANNELS):
                        out[j, i, c] = out[j, i, c] + self.f[j, i, s, c]
        return out

    def ids(self, counts=None, onto=None):
        """ids [H, W, 2] a call with first_sample 0 leaves: sample 0's where the
        pixel takes a sample, `onto` (zeros) elsewhere."""
        out = np.zeros((self.H, self.W, 2), np.int32) if onto is None else np.array(onto, np.int32)
        take = np.ones((self.H, self.W), bool) if counts is None else np.asarray(counts) > 0
        out[take] = self.i[:, :, 0][take]
        return out


def _checker_margin(world, tid, u, v):
    """min |x - round(x)| over x = u * inv_scale, v * inv_scale of the checker
    textures Texture::get_colour walks from texture tid (inf: none)."""
    margin = math.inf
    while True:
        kind, tp, refs = world.tex[tid]
        if kind != rtw.RTW_TEX_CHECKER:
            return margin
        for x in (u * tp[3], v * tp[3]):
            margin = min(margin, abs(x - round(x)))
        s = math.floor(u * tp[3]) + math.floor(v * tp[3])
        tid = refs[0] if math.fmod(s, 2.0) == 0.0 else refs[1]


@functools.lru_cache(maxsize=None)
def samples(name, width=W, height=H, n_samples=SAMPLES):
    return Samples(name, width, height, n_samples)


def same(a, b):
    """bit for bit up to the sign of zero, NaN masks equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
