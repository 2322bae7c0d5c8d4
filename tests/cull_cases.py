"""Adversarial cases for the f64 kernels' f32 culling filters (plain numpy,
fixed seeds): ray/sphere records for the primitive probe, ray/box records for
the slab test, and small scenes for the render-level parity tests.

The f64 kernels throw candidates away with f32 filters (the widened slab test,
sphere_may_hit, light_may_hit, the cooperative grid walk) whose error bounds are
relative to the coordinates' size; these cases put the geometry where such a
bound can break: near-zero discriminants, origins on the surface, far origins,
zero direction components, and magnitudes from 2^-130 to 2^130.
tests/test_cull_cases_host.py checks on the CPU oracle that the cases are not
vacuous; tests/test_gpu_cull_probe.py and tests/test_gpu_f64_culls.py run them.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace

import numpy as np

from oracle import oracle as O

FAMILIES = ("tangent", "on_surface", "inside", "far_origin", "axis", "degenerate", "clear_hit", "clear_miss")
CONTROLS = ("clear_hit", "clear_miss")
K_TIER1 = (-40, -20, 0, 10, 20, 30, 40)      # |c| = 2^k
K_TIER2 = (-130, -70, 70, 130)               # f32 squares, or the values themselves, leave f32's range
LOG_RATIO = (-30, -20, -10, -3, 0, 10)       # r / |c| = 2^lr
LOG_DLEN = (-30, -15, 0, 15, 30)             # |d| = 2^ld (the reference never normalises directions)
EPS = 2.0 ** -52


@dataclass
class Records:
    rec: np.ndarray      # (n, 10) o xyz, d xyz, c xyz, r
    family: np.ndarray   # (n,) index into FAMILIES
    k: np.ndarray        # (n,) the sweep's coordinate exponent
    tier: np.ndarray     # (n,) 1: every |coordinate|, r within 2^41 and k from K_TIER1; else 2


def _units(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(w, rng):
    """unit vectors perpendicular to the unit vectors w"""
    a = _units(rng, len(w))
    v = a - (a * w).sum(1, keepdims=True) * w
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rows(o, d, c, r):
    n = len(o)
    out = np.empty((n, 10))
    out[:, 0:3], out[:, 3:6], out[:, 6:9] = o, d, c
    out[:, 9] = np.broadcast_to(r, (n,))
    return out


def _family_rows(fam, rng, c, r, dl):
    """The variants of one family for one sweep point: centre c (3,), radius r, |d| = dl."""
    def rep(n):
        return np.broadcast_to(c, (n, 3)).copy()

    if fam == "tangent":
        # d aimed at the silhouette, displaced across it by +-2^-52 .. +-2^-16 (relative)
        delta = np.array([s * 2.0 ** e for e in (-52, -40, -28, -16) for s in (-1, 1)] * 2)
        dist = np.repeat([1.25, 1024.0], 8) * r
        n = len(delta)
        cc = rep(n)
        o = cc + dist[:, None] * _units(rng, n)
        oc = o - cc
        dd = np.linalg.norm(oc, axis=1)
        w = -oc / dd[:, None]
        v = _perp(w, rng)
        sin = np.minimum(r / dd * (1.0 + delta), 1.0)
        d = dl * (np.sqrt(1.0 - sin * sin)[:, None] * w + sin[:, None] * v)
        return _rows(o, d, cc, r)
    if fam == "on_surface":
        # o on the sphere +- a few ulps along the normal; d leaving, entering, tangential
        js = np.repeat([-4.0, -1.0, 0.0, 1.0, 4.0], 4)
        n = len(js)
        cc = rep(n)
        nrm = _units(rng, n)
        tan = _perp(nrm, rng)
        o = cc + (r * (1.0 + js * EPS))[:, None] * nrm
        kind = np.tile([0, 1, 2, 3], 5)
        d = np.where((kind == 0)[:, None], nrm + 0.3 * tan,
                     np.where((kind == 1)[:, None], -nrm + 0.3 * tan,
                              np.where((kind == 2)[:, None], tan + 2.0 ** -40 * nrm, tan - 2.0 ** -40 * nrm)))
        return _rows(o, dl * d, cc, r)
    if fam == "inside":
        # inside (the centre, deep inside: r >= 2^20 |o - c|, near the surface), any
        # direction; and their twins just outside, leaving
        f = np.array([0.0, 0.0, 2.0 ** -30, 2.0 ** -25, 2.0 ** -25, 0.5, 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -20,
                      1.0 + 2.0 ** -20, 1.0 + 2.0 ** -20, 1.5, 2.0])
        n = len(f)
        cc = rep(n)
        nrm = _units(rng, n)
        o = cc + (f * r)[:, None] * nrm
        d = np.where((f > 1.0)[:, None], nrm + 0.5 * _perp(nrm, rng), _units(rng, n))
        return _rows(o, dl * d, cc, r)
    if fam == "far_origin":
        # |o - c| / r up to 2^30, d aimed through (or just past) the sphere
        D = np.repeat([2.0 ** 5, 2.0 ** 10, 2.0 ** 20, 2.0 ** 30], 5)
        xi = np.tile([0.0, 0.5, 0.999, 1.001, 1.5], 4)
        n = len(D)
        cc = rep(n)
        nrm = _units(rng, n)
        o = cc + (D * r)[:, None] * nrm
        p = cc + (xi * r)[:, None] * _perp(nrm, rng)
        d = p - o
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        return _rows(o, dl * d, cc, r)
    if fam == "axis":
        # one or two components of d exactly +-0, the same components of o exactly 0
        rows = []
        scale = float(np.abs(c).max())
        for two in (True, False):
            for xi in (0.0, 0.5, 0.999, 1.001, 2.0):
                for ahead in (1.0, 1.0, -1.0):
                    ax = rng.permutation(3)
                    z = ax[:2] if two else ax[:1]          # the zero components
                    f = ax[2:] if two else ax[1:]          # the free ones
                    o, d, cc = np.zeros(3), np.zeros(3), np.zeros(3)
                    u = rng.normal(size=len(f))
                    u = u / np.linalg.norm(u)
                    d[f] = dl * u
                    d[z] = rng.choice([0.0, -0.0], size=len(z))
                    o[f] = scale * rng.uniform(-1, 1, size=len(f)) * (rng.random() < 0.7)
                    # the centre: ahead of (or behind) o along d, offset xi r across it
                    across = np.zeros(3)
                    if two:
                        ph = rng.uniform(0, 2 * np.pi)
                        across[z] = np.array([np.cos(ph), np.sin(ph)])
                    else:
                        ph = rng.uniform(0, 2 * np.pi)
                        perp_in = np.array([-u[1], u[0]])
                        across[z] = np.cos(ph)
                        across[f] = np.sin(ph) * perp_in
                    along = d / dl
                    cc = o + ahead * max(scale, 2.0 * r) * along + xi * r * across
                    rows.append(np.concatenate([o, d, cc, [r]]))
        return np.array(rows)
    if fam == "degenerate":
        n = 7
        cc = rep(n)
        nrm = _units(rng, n)
        o = cc + 8.0 * max(r, np.abs(c).max() * 2.0 ** -20) * nrm
        aim = -nrm
        off = _perp(nrm, rng)
        d = aim.copy()
        rr = np.array([0.0, 0.0, -r, -r, r, 0.0, -r])
        d[1] = aim[1] + 0.3 * off[1]          # r = 0, aimed off the centre
        d[2] = aim[2] + 0.03 * off[2]         # negative radius, clear hit
        d[3] = aim[3] + 0.5 * off[3]          # negative radius, clear miss
        o[4:] = cc[4:]                        # o = c exactly, r > 0, = 0, < 0
        d[4:] = _units(rng, 3)
        return _rows(o, dl * d, cc, rr)
    # the controls
    D = np.array([3.0, 100.0, 3.0, 100.0])
    n = len(D)
    cc = rep(n)
    nrm = _units(rng, n)
    o = cc + (D * r)[:, None] * nrm
    xi = 0.3 if fam == "clear_hit" else 3.0
    p = cc + (xi * r) * _perp(nrm, rng)
    d = p - o
    if fam == "clear_miss":
        d[2:] = -d[2:]                        # and pointing away
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return _rows(o, dl * d, cc, r)


@functools.lru_cache(maxsize=None)
def records() -> Records:
    rng = np.random.default_rng(0xC0111)
    recs, fams, ks, t1 = [], [], [], []
    for ks_, first in ((K_TIER1, True), (K_TIER2, False)):
        for k in ks_:
            for lr in LOG_RATIO:
                for ld in LOG_DLEN:
                    for fi, fam in enumerate(FAMILIES):
                        c = 2.0 ** k * rng.uniform(0.5, 1.0) * _units(rng, 1)[0] * np.sqrt(3.0)
                        r = 2.0 ** (k + lr) * rng.uniform(1.0, 2.0)
                        rows = _family_rows(fam, rng, c, r, 2.0 ** ld)
                        recs.append(rows)
                        fams.append(np.full(len(rows), fi))
                        ks.append(np.full(len(rows), k))
                        t1.append(np.full(len(rows), first))
    rec = np.concatenate(recs)
    assert np.isfinite(rec).all()
    big = np.abs(np.delete(rec, [3, 4, 5], axis=1)).max(axis=1)
    tier = np.where(np.concatenate(t1) & (big <= 2.0 ** 41), 1, 2)
    return Records(rec, np.concatenate(fams), np.concatenate(ks), tier)


def f32_sphere(rec):
    """{c, r^2} rounded to f32 exactly as host/stage_scene.cpp fills bsph32: the
    f64 leaf sphere {c, r * r} converted component by component -- and r^2 =
    -inf for a negative radius, as the scene is staged (bounded_hit never passes
    such a sphere's inverted AABB, sphere.rs:42-45).  The probe's f64 columns use
    r * r as Sphere::hit itself does, so for those records the pre-pass is asked
    to keep more than the kernel needs (it does: -inf makes its bound NaN)."""
    with np.errstate(over="ignore"):
        r2 = np.where(rec[:, 9] < 0, -np.inf, rec[:, 9] * rec[:, 9])
        return np.concatenate([rec[:, 6:9], r2[:, None]], axis=1).astype(np.float32)


# ------------------------------------------------------------------ slab records
@functools.lru_cache(maxsize=None)
def box_records():
    """(rec (n, 13) {o, d, box min, box max, tb}, family (n,), k (n,)): boxes with o
    on a face, rays in a face plane with a zero direction component, grazing an
    edge, and plain hits / misses, at the record sweep's scales."""
    rng = np.random.default_rng(0xB0C5)
    rows, fams, ks = [], [], []
    for k in K_TIER1 + K_TIER2:
        for lr in (-20, -3, 0, 10):
            for ld in (-30, 0, 30):
                s = 2.0 ** k
                mid = s * rng.uniform(-1, 1, 3)
                half = 2.0 ** (k + lr) * rng.uniform(0.5, 1.0, 3)
                lo, hi = mid - half, mid + half
                half = (hi - lo) / 2
                for fam in range(4):
                    for _ in range(6):
                        a = int(rng.integers(3))
                        b, c2 = [x for x in range(3) if x != a]
                        o = lo + rng.uniform(0, 1, 3) * (hi - lo)
                        d = rng.normal(size=3)
                        tb = np.inf
                        if fam == 0:       # o on a face, d leaving / entering / along it
                            o[a] = (lo, hi)[int(rng.integers(2))][a]
                            if rng.random() < 0.34:
                                d[a] = 0.0
                        elif fam == 1:     # o outside, in a face's plane, d[a] = +-0
                            o[a] = (lo, hi)[int(rng.integers(2))][a]
                            o[b] = lo[b] - rng.uniform(0.5, 3) * (hi - lo)[b]
                            d[a] = rng.choice([0.0, -0.0])
                            d[b] = abs(d[b])
                            d[c2] *= 0.2
                        elif fam == 2:     # aimed at an edge, displaced across it
                            o = mid + 8 * half * rng.choice([-1, 1], 3) * rng.uniform(1, 2, 3)
                            p = np.where(rng.random(3) < 0.5, lo, hi)
                            p[a] = lo[a] + rng.uniform(0, 1) * (hi - lo)[a]
                            p = p + rng.choice([-1, 1]) * 2.0 ** rng.choice([-52, -30, -20]) * np.abs(p)
                            d = p - o
                            # tb at the box, or inf
                            if rng.random() < 0.5:
                                tb = 1.0 * rng.choice([1 - 2.0 ** -30, 1 + 2.0 ** -30, 2.0])
                        else:              # plain: through the middle, or away
                            o = mid + 8 * half * rng.choice([-1, 1], 3) * rng.uniform(1, 2, 3)
                            d = (mid - o) * rng.choice([1.0, -1.0])
                        ln = np.linalg.norm(d)
                        if fam != 2 or tb == np.inf:
                            d = d / ln * 2.0 ** ld
                        rows.append(np.concatenate([o, d, lo, hi, [tb]]))
                        fams.append(fam)
                        ks.append(k)
    rec = np.array(rows)
    assert np.isfinite(rec[:, :12]).all()
    return rec, np.array(fams), np.array(ks)


def f32_box_outward(lo, hi):
    """the f64 box rounded outward to f32 (as host/bvh.cpp rounds the f32 tree)"""
    with np.errstate(over="ignore"):
        l32, h32 = lo.astype(np.float32), hi.astype(np.float32)
        l32 = np.where(l32.astype(np.float64) > lo, np.nextafter(l32, np.float32(-np.inf)), l32)
        h32 = np.where(h32.astype(np.float64) < hi, np.nextafter(h32, np.float32(np.inf)), h32)
    return l32, h32


# ------------------------------------------------------------------ render scenes
@dataclass
class Case:
    name: str
    scene: O.Scene
    cam: O.Camera
    seed: int
    extra_grids: tuple = ()       # further light_grid resolutions to run
    textured: bool = False        # also once with identity solid textures (the per-lane grid walk)
    axis: bool = False
    far_origin: bool = False


def _scene(spheres, mats, lights, planes=(), plane_mats=()):
    """spheres: [(c, r, mat index)], mats: [(type, (r, g, b), fuzz, ior)], planes: [(p, n)]"""
    sph = np.array([list(c) + [r] for c, r, _ in spheres], np.float64).reshape(-1, 4)
    smat = np.array([m for _, _, m in spheres], np.uint32)
    pl = np.array([list(p) + list(n) for p, n in planes], np.float64).reshape(-1, 6)
    return O.Scene(sph, smat, pl, np.array(plane_mats, np.uint32),
                   np.array([m[0] for m in mats], np.uint32),
                   np.array([list(m[1]) + [m[2], m[3]] for m in mats], np.float64).reshape(-1, 5),
                   np.array(lights, np.float64).reshape(-1, 4))


def _mats():
    return [(O.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, 0.0), (O.LAMBERTIAN, (0.7, 0.3, 0.2), 0.0, 0.0),
            (O.METAL, (0.8, 0.7, 0.6), 0.1, 0.0), (O.DIELECTRIC, (1.0, 1.0, 1.0), 0.0, 1.5),
            (O.DIFFUSE_LIGHT, (4.0, 3.5, 3.0), 0.0, 0.0), (O.METAL, (0.9, 0.9, 0.9), 0.0, 0.0),
            (O.LAMBERTIAN, (0.2, 0.4, 0.8), 0.0, 0.0)]


def _base(n_lights=68):
    """~60 spheres of all three materials on a huge ground sphere, 20 of them
    emitting; the light list: the emitters, then the glass spheres and further
    spheres that emit nothing (a light list entry need not emit), 68 in all."""
    rng = np.random.default_rng(0xBA5E)
    sph = [((0.0, -1000.0, 0.0), 1000.0, 0)]
    glass, emit = [], []
    for i in range(40):
        x, z = (i % 8 - 3.5) * 1.1 + rng.uniform(-0.3, 0.3), (i // 8 - 2.0) * 1.1 + rng.uniform(-0.3, 0.3)
        r = float(rng.uniform(0.15, 0.45))
        y = float(np.sqrt(1000.0 ** 2 - x * x - z * z) - 1000.0 + r)
        m = (1, 2, 3, 6)[i % 4]
        sph.append(((float(x), y, float(z)), r, m))
        if m == 3:
            glass.append([float(x), y, float(z), r])
    for i in range(20):
        c = (float(rng.uniform(-4, 4)), float(rng.uniform(1.2, 3.0)), float(rng.uniform(-3, 3)))
        r = float(rng.uniform(0.05, 0.25))
        sph.append((c, r, 4))
        emit.append(list(c) + [r])
    lights = emit + glass
    while len(lights) < 68:
        lights.append([float(rng.uniform(-5, 5)), float(rng.uniform(0.2, 3.0)), float(rng.uniform(-4, 4)),
                       float(rng.uniform(0.05, 0.3))])
    return sph, lights[:n_lights]


BASE_CAM = dict(lookfrom=(6.0, 2.5, 6.0), lookat=(0.0, 0.3, 0.0), vfov=40.0, focus_dist=8.0,
                background=(0.7, 0.8, 1.0), image_width=32, image_height=24, samples_per_pixel=3, max_depth=10)


def _xform(sph, lights, cam_kw, scale=1.0, shift=(0.0, 0.0, 0.0)):
    sh = np.array(shift)
    sph2 = [(tuple(np.array(c) * scale + sh), r * scale, m) for c, r, m in sph]
    li2 = [list(np.array(L[:3]) * scale + sh) + [L[3] * scale] for L in lights]
    kw = dict(cam_kw)
    kw["lookfrom"] = tuple(np.array(cam_kw["lookfrom"]) * scale + sh)
    kw["lookat"] = tuple(np.array(cam_kw["lookat"]) * scale + sh)
    kw["focus_dist"] = cam_kw["focus_dist"] * scale
    return sph2, li2, kw


def _far_origin():
    """A low camera looking along a down-facing, barely tilted plane (Plane::hit
    accepts only dot(d, n) > eps, and n = -y exactly panics on the UV), a cluster
    of ~100 small lights near the origin: the plane's Lambertian bounces are
    light queries from > 10^4 away."""
    rng = np.random.default_rng(0xFA20)
    n = np.array([1e-9, -1.0, 5e-10])
    n = n / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    sph, lights = [], []
    while len(sph) < 100:
        c = (float(rng.uniform(-3, 3)), float(rng.uniform(0.3, 3.0)), float(rng.uniform(-3, 3)))
        r = float(rng.uniform(0.1, 0.5))
        if np.hypot(c[0], c[1] - 1.0) < r + 0.2:   # the camera's (thin) beam passes at x = 0, y ~ 1
            continue
        sph.append((c, r, 4))
        lights.append(list(c) + [r])
    sc = _scene(sph, _mats(), lights, planes=[((0.0, 0.0, 0.0), tuple(n))], plane_mats=[0])
    cam = O.camera_build(lookfrom=(0.0, 1.0, 40.0), lookat=(0.0, 1.0 - 40 * 6e-5, 0.0), vfov=0.006,
                         focus_dist=10.0, background=(0.7, 0.8, 1.0), image_width=32, image_height=16,
                         samples_per_pixel=4, max_depth=8)
    return sc, cam


def _axis(one_zero, offset=0.0):
    """Every primary ray exactly (0, 0, -1) focus from a centre with zero x and y
    (pixel deltas overwritten with 0), or with a zero x component only; spheres
    on the axis (glass: the ray stays on it; a mirror behind the camera sends it
    back) and touching it.  offset: the camera's x, with d.x still exactly 0 --
    o ix is then infinite, not NaN: the slab planes of a box that straddles
    x = 0 come out as -inf and inf - inf."""
    sph = [((0.0, 0.0, 0.0), 1.0, 3), ((0.0, 0.0, -4.0), 1.5, 1), ((0.0, 0.0, 12.0), 2.0, 5),
           ((1.0, 0.0, 2.5), 1.0, 2), ((0.0, -0.5, 3.5), 0.5, 6), ((-0.75, 0.0, -1.5), 0.75, 0),
           ((0.0, 3.0, -3.0), 0.5, 4), ((2.5, 1.0, -2.0), 0.4, 4), ((-2.0, -1.5, -1.0), 0.3, 4),
           ((0.0, 0.0, -9.0), 0.6, 4), ((1.5, -2.0, 4.0), 0.5, 4)]
    lights = [list(c) + [r] for c, r, m in sph if m == 4]
    sc = _scene(sph, _mats(), lights)
    cam = O.camera_build(lookfrom=(offset, 0.0, 5.0), lookat=(offset, 0.0, 0.0), vfov=30.0, focus_dist=4.0,
                         background=(0.7, 0.8, 1.0), image_width=16, image_height=12, samples_per_pixel=4,
                         max_depth=10)
    if one_zero:
        for q in range(3):
            cam.pixel_delta_u[q] = 0.0
        cam.pixel_delta_v[0] = 0.0
        cam.pixel00_loc[0] = cam.center[0]
    else:
        for q in range(3):
            cam.pixel_delta_u[q] = 0.0
            cam.pixel_delta_v[q] = 0.0
        cam.pixel00_loc[0], cam.pixel00_loc[1], cam.pixel00_loc[2] = 0.0, 0.0, 1.0
    return sc, cam


def _grazing():
    """A few hundred spheres of radius 1e-6 .. 1e-3 at distances 1 .. 100 along the
    primary rays, spheres of radius 1e3 and 1e6 whose horizons cross the image,
    and a light sphere around everything."""
    rng = np.random.default_rng(0x62A2)
    kw = dict(lookfrom=(0.0, 1.0, 0.0), lookat=(0.0, 0.8, -10.0), vfov=40.0, focus_dist=10.0,
              background=(0.7, 0.8, 1.0), image_width=32, image_height=24, samples_per_pixel=3, max_depth=8)
    cam = O.camera_build(**kw)
    sph = [((0.0, -1000.0, 0.0), 1000.0, 0), ((2.0e5, -1.0e6 + 3.0, -4.0e5), 1.0e6, 1)]
    c0 = np.array(cam.center[:])
    p00, du, dv = np.array(cam.pixel00_loc[:]), np.array(cam.pixel_delta_u[:]), np.array(cam.pixel_delta_v[:])
    for k in range(300):
        i, j = rng.uniform(0, 32), rng.uniform(0, 24)
        d = p00 + i * du + j * dv - c0
        d = d / np.linalg.norm(d)
        t = 10.0 ** rng.uniform(0, 2)
        r = 10.0 ** rng.uniform(-6, -3)
        sph.append((tuple(c0 + t * d), float(r), (1, 2, 3, 6)[k % 4]))
    enclosing = [0.0, 0.0, 0.0, 4.0e6]
    sph.append((tuple(enclosing[:3]), enclosing[3], 4))
    lights = [enclosing, [3.0, 5.0, -8.0, 0.5], [-4.0, 2.0, -6.0, 1e-3]]
    sph.append(((3.0, 5.0, -8.0), 0.5, 4))
    return _scene(sph, _mats(), lights), cam


@functools.lru_cache(maxsize=None)
def scenes():
    out = []
    sph, li = _base()
    out.append(Case("base", _scene(sph, _mats(), li), O.camera_build(**BASE_CAM), 101))
    out.append(Case("base_5_lights", _scene(sph, _mats(), li[:5]), O.camera_build(**BASE_CAM), 102))
    for k in (-40, -20, 20, 40):
        s2, l2, kw = _xform(sph, li, BASE_CAM, scale=2.0 ** k)
        out.append(Case(f"scaled_2^{k}", _scene(s2, _mats(), l2), O.camera_build(**kw), 103))
    for k in (12, 18, 22):
        s2, l2, kw = _xform(sph, li, BASE_CAM, shift=(2.0 ** k, -2.0 ** k, 2.0 ** k))
        out.append(Case(f"translated_2^{k}", _scene(s2, _mats(), l2), O.camera_build(**kw), 104))
    sc, cam = _far_origin()
    out.append(Case("far_origin", sc, cam, 105, extra_grids=(1, 256), textured=True, far_origin=True))
    for one_zero in (False, True):
        sc, cam = _axis(one_zero)
        out.append(Case("axis_one_zero" if one_zero else "axis_parallel", sc, cam, 106, axis=True))
    sc, cam = _axis(True, offset=0.3)
    out.append(Case("axis_one_zero_offset", sc, cam, 106, axis=True))
    for e in (-30, 30):
        kw = dict(BASE_CAM, focus_dist=2.0 ** e)
        out.append(Case(f"focus_2^{e}", _scene(sph, _mats(), li), O.camera_build(**kw), 107))
    sc, cam = _grazing()
    out.append(Case("grazing", sc, cam, 108))
    return tuple(out)


def scene_names():
    return [c.name for c in scenes()]


def scene(name) -> Case:
    return next(c for c in scenes() if c.name == name)


def with_identity_textures(sc: O.Scene) -> O.Scene:
    """The same scene with a SolidColour texture of its own albedo on every
    material: the same pixels, through the textured kernels."""
    nm = len(sc.mat_type)
    return replace(sc, mat_tex=np.arange(nm, dtype=np.uint32), tex_type=np.full(nm, O.TEX_SOLID, np.uint32),
                   tex_params=np.array([list(sc.mat_params[m][:3]) + [0.0] for m in range(nm)], np.float64),
                   tex_refs=np.zeros((nm, 2), np.uint32))


def light_sphere_ids(sc: O.Scene):
    """world ids (trace_path's numbering: planes first, then spheres) of the world
    spheres that are also in the light list"""
    li = {tuple(L) for L in np.asarray(sc.lights).reshape(-1, 4).tolist()}
    base = len(sc.plane_mat)
    return {base + k for k, s in enumerate(np.asarray(sc.spheres).reshape(-1, 4).tolist()) if tuple(s) in li}
