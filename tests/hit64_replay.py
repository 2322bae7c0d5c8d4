"""The f32 render's f64 hit-point path (kOptHit64, render_kernel.hpp), replayed
transition by transition -- TEST INFRASTRUCTURE ONLY.

The RTW_TRACE build records, per segment of a traced sample, the f64 ray
(o64, d64), the object the f32 traversal picked, its f64 t, the f32 t and the
sphere the ray starts on.  Given segment k as traced, everything the kernel
derives from it in f64 "with the reference's operation order and no FMA"
 is recomputed here with Python floats -- IEEE binary64, one
rounding per operation, like tests/indep/restate.py, whose Vec3 operations
this file uses -- and compared with segment k + 1 or with the sample's end.  No
error carries from one segment to the next: only the RNG stream does, replayed
draw by draw with each branch's own draw count.

Restated from the kernel (the line numbers are render_kernel.hpp's):
  sphere_t_ref64, plane_t_ref64, ray_at64, sphere_normal64, front64   247-278, 405-413
  mix32, dither64                                                    288-304
  specular_dir64 (Metal / Dielectric on a sphere, f64)               371-404
  the f32 unit ball by inversion (unit_sphere<float>)                rtw_device.hpp
  mixture_direction<double> on the widened f32 light                 rtw_device.hpp, 1285-1298
  the scene's f64 records (sph64, pl64, mat64)                       host/stage_scene.cpp

With f32 = False the same driver takes the reference's forms everywhere (f64
inputs, the UnitSphere rejection loop, f64 uniforms): driven by
restate.World.hit it must reproduce restate.trace_sample bit for bit
(tests/test_hit64_replay_host.py), which proves the driver -- draw counts,
branch order, terminations -- before it judges a kernel.
"""
from __future__ import annotations

import math
import struct

import numpy as np

from indep import restate as RS

EPS = RS.EPS
INF = RS.INF
LAMBERTIAN, METAL, DIELECTRIC, INVISIBLE, DIFFUSE_LIGHT = 0, 1, 2, 3, 4
M32 = 0xFFFFFFFF
NEAR = 1e-5                          # an f32 decision's quantity this close to its threshold is not replayed
LD = np.longdouble


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def same(a, b):
    """equal bit patterns (NaNs of any payload count as equal)"""
    return all((x != x and y != y) or bits(x) == bits(y) for x, y in zip(a, b))


def r32(x):
    """x rounded to f32, held as a Python float"""
    return float(np.float32(x))


def v32(v):
    return (r32(v[0]), r32(v[1]), r32(v[2]))


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


# ------------------------------------------------------------------ dither64
def mix32(h):
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    h ^= h >> 16
    return h


K_SCALE = 2.0 ** -25 / 4294967296.0


def dither64(v):
    """an f32 vector as a generic f64 one: hashed bits below the f32 mantissa"""
    h0 = mix32(f32_bits(v[0]) ^ mix32(f32_bits(v[1]) ^ mix32(f32_bits(v[2]))))
    h1 = mix32((h0 + 0x9E3779B9) & M32)
    h2 = mix32((h1 + 0x9E3779B9) & M32)
    return tuple(x * (1.0 + (float(h) - 2147483648.0) * K_SCALE) for x, h in zip(v, (h0, h1, h2)))


def is_dithered(d):
    """d == dither64(float32(d)) bit for bit"""
    return same(d, dither64(v32(d)))


# ------------------------------------------------------------ the f64 records
def sphere_t_ref64(S, o, d):
    """(hit, t) of Sphere::hit over [EPSILON, inf] on the sphere as given"""
    ocx, ocy, ocz, r = o[0] - S[0], o[1] - S[1], o[2] - S[2], S[3]
    a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    half_b = ocx * d[0] + ocy * d[1] + ocz * d[2]
    c = (ocx * ocx + ocy * ocy + ocz * ocz) - r * r
    disc = half_b * half_b - a * c
    if not disc > 0.0:
        return False, 0.0
    sq = math.sqrt(disc)
    root = RS.fdiv(-half_b - sq, a)
    if not (EPS <= root <= INF):
        root = RS.fdiv(-half_b + sq, a)
        if not (EPS <= root <= INF):
            return False, 0.0
    return True, root


def plane_t_ref64(P, o, d):
    pt, n = P
    denom = d[0] * n[0] + d[1] * n[1] + d[2] * n[2]
    return -RS.fdiv((o[0] - pt[0]) * n[0] + (o[1] - pt[1]) * n[1] + (o[2] - pt[2]) * n[2], denom)


def ray_at64(o, d, t):
    return (o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t)


def sphere_normal64(p, S):
    return RS.divs((p[0] - S[0], p[1] - S[1], p[2] - S[2]), S[3])


def front64(d, n):
    return d[0] * n[0] + d[1] * n[1] + d[2] * n[2] < 0.0


class Scene:
    """The scene as host/stage_scene.cpp stages it for an f32 kernel with f64 hit
    points: sph64 and pl64 as given, spheres, planes, lights and material
    parameters rounded to f32, mat64 with the host's operations.  f32 = False: all
    of it as given."""

    def __init__(self, soa, f32=True):
        rnd = r32 if f32 else float
        self.f32 = f32
        self.sph64 = [tuple(map(float, s)) for s in np.asarray(soa.spheres, np.float64).reshape(-1, 4)]
        self.sph = [tuple(rnd(x) for x in s) for s in self.sph64]
        self._sph = np.array(self.sph64, np.float64).reshape(-1, 4)
        self.sphere_mat = [int(m) for m in soa.sphere_mat]
        pl = np.asarray(soa.planes, np.float64).reshape(-1, 6)
        self.pl64 = [(tuple(map(float, p[:3])), tuple(map(float, p[3:]))) for p in pl]
        self.pl = [(tuple(rnd(x) for x in p), tuple(rnd(x) for x in n)) for p, n in self.pl64]
        self.plane_mat = [int(m) for m in soa.plane_mat]
        self.n_planes = self.sbase = len(self.pl64)
        # Plane::get_aabbox (plane.rs:218-242): the normal's axis pinned at 0 (wherever the plane's
        # point lies), the others infinite -- bounded_hit tests it before the plane
        self.pl_box = [RS.Plane(p, n, 0).aabb for p, n in self.pl64]
        assert not len(soa.quad_mat) and not len(soa.box_mat) and soa.mat_tex is None
        self.lights = [tuple(rnd(x) for x in L) for L in np.asarray(soa.lights, np.float64).reshape(-1, 4)]
        self.mat_type = [int(t) for t in soa.mat_type]
        assert DIFFUSE_LIGHT not in self.mat_type or not f32
        self.mat_params = [tuple(map(float, m)) for m in np.asarray(soa.mat_params, np.float64).reshape(-1, 5)]
        self.albedo = [tuple(rnd(x) for x in m[:3]) for m in self.mat_params]
        self.mat64 = []
        for t, m in zip(self.mat_type, self.mat_params):
            if t == DIELECTRIC:
                ior, rf = m[4], 1.0 / m[4]
                r0f, r0b = (1.0 - rf) / (1.0 + rf), (1.0 - ior) / (1.0 + ior)
                self.mat64.append((rf, r0f * r0f, r0b * r0b, ior))
            else:
                self.mat64.append((0.0, 0.0, 0.0, m[3] if t == METAL else 0.0))

    def material(self, obj):
        return self.plane_mat[obj] if obj < self.sbase else self.sphere_mat[obj - self.sbase]

    def closest64(self, o, d):
        """the f64 brute-force closest hit of the ray over [EPSILON, inf]: [(t, id)]
        of every object hit, in t order (planes first among equals: list order)"""
        out = []
        for k, P in enumerate(self.pl64):
            if d[0] * P[1][0] + d[1] * P[1][1] + d[2] * P[1][2] > EPS and self.pl_box[k].is_hit(o, d, EPS, INF):
                t = plane_t_ref64(P, o, d)
                if EPS <= t <= INF:
                    out.append((t, k))
        # the spheres at once: numpy's elementwise f64 operations round one by one too
        S = self._sph
        with np.errstate(all="ignore"):
            oc = (o[0] - S[:, 0], o[1] - S[:, 1], o[2] - S[:, 2])
            a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            half_b = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2]
            c = (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) - S[:, 3] * S[:, 3]
            disc = half_b * half_b - a * c
            sq = np.sqrt(disc)
            t0, t1 = (-half_b - sq) / a, (-half_b + sq) / a
            t = np.where((t0 >= EPS) & (t0 <= INF), t0, t1)
            hit = (disc > 0.0) & (t >= EPS) & (t <= INF)
        out += [(float(t[k]), self.sbase + int(k)) for k in np.nonzero(hit)[0]]
        out.sort(key=lambda e: e[0])
        return out


# ------------------------------------------------------------------ samplers
def _ld_div(a, b):
    return a / b


def _onb(n, sqrt, div):
    l = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    w = (div(n[0], l), div(n[1], l), div(n[2], l))
    a = (0.0, 1.0, 0.0) if abs(float(w[0])) > 0.9 else (1.0, 0.0, 0.0)
    a = tuple(type(l)(x) for x in a)
    v = RS.cross(w, a)
    l = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    v = (div(v[0], l), div(v[1], l), div(v[2], l))
    return RS.cross(w, v), v, w


def mixture_direction(to_light, n, c, radius, o, r1, r2, ld=False):
    """mixture_direction<double> (rtw_device.hpp): Sphere::random of the light
    (c, radius) seen from o, or the cosine lobe about n, from the uniforms r1, r2.
    Python floats: each operation rounded once, no FMA.  ld: the same expressions
    in np.longdouble with its own sin / cos -- the law the 4 x rule is held to."""
    if ld:
        cv, sqrt, div, one = LD, np.sqrt, _ld_div, LD(1)
        n, c, o = tuple(map(LD, n)), tuple(map(LD, c)), tuple(map(LD, o))
        radius, r1, r2 = LD(radius), LD(r1), LD(r2)
    else:
        cv, sqrt, div, one = float, RS.sqrt, RS.fdiv, 1.0
    with np.errstate(all="ignore"):
        direction = (c[0] - o[0], c[1] - o[1], c[2] - o[2])
        fu, fv, fw = _onb(direction if to_light else n, sqrt, div)
        q = cv(0)
        if to_light:
            distance = sqrt(RS.dot(direction, direction))
            q = div(radius * radius, distance * distance)
        az = r2 if to_light else r1
        if ld:
            x = LD(2) * LD("3.14159265358979323846264338327950288") * az
            s, cph = np.sin(x), np.cos(x)
        else:
            s, cph = RS.sincos_2pi(az)
        t = sqrt(one - (q if to_light else r2))
        z = one + r1 * (t - one) if to_light else t
        sxy = sqrt(one - z * z if to_light else r2)
        x = (cph * sxy, s * sxy, z)
        acc = (cv(0), cv(0), cv(0))
        acc = RS.add(acc, RS.muls(fu, x[0]))
        acc = RS.add(acc, RS.muls(fv, x[1]))
        return RS.add(acc, RS.muls(fw, x[2]))


def _u24(w):
    return (w >> 40) * 2.0 ** -24


def unit_sphere_f32(w0, w1, w2, calib=False):
    """unit_sphere<float> from its three words: radius u^(1/3), z uniform, azimuth
    uniform.  The law: the form in f64 on the 24-bit uniforms; calib: the same in
    f32, each operation and each library call rounded once."""
    z, az, u = _u24(w0), _u24(w1), _u24(w2)
    if calib:
        f = np.float32
        z = f(2) * f(z) - f(1)
        r = f(2.0 ** float(f(f(math.log2(u)) * f(1.0 / 3.0)))) if u > 0 else f(0)
        s, c = f(math.sin(2 * math.pi * az)), f(math.cos(2 * math.pi * az))
        rxy = r * np.sqrt(max(f(1) - z * z, f(0)))
        return (float(rxy * c), float(rxy * s), float(r * z))
    z = 2.0 * z - 1.0
    r = u ** (1.0 / 3.0) if u > 0 else 0.0
    s, c = math.sin(2 * math.pi * az), math.cos(2 * math.pi * az)
    rxy = r * math.sqrt(max(1.0 - z * z, 0.0))
    return (rxy * c, rxy * s, r * z)


def sphere_t_f32(S, o, d, calib):
    """the smaller root the f32 kernels' sphere test stands for, on the f32 ray and
    sphere: in f64 (the law) or with every operation rounded to f32 (calib); NaN
    without a hit -- the calibration of an f32 t's error"""
    f = np.float32 if calib else np.float64
    with np.errstate(all="ignore"):
        o, d, c, r = [f(x) for x in o], [f(x) for x in d], [f(x) for x in S[:3]], f(S[3])
        oc = [o[k] - c[k] for k in range(3)]
        a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        hb = d[0] * oc[0] + d[1] * oc[1] + d[2] * oc[2]
        cc = (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) - r * r
        disc = hb * hb - a * cc
        if not disc > 0:
            return float("nan")
        sq = np.sqrt(disc)
        t = (-hb - sq) / a
        if not t >= f(EPS):
            t = (-hb + sq) / a
        return float(t)


# ------------------------------------------------------------------- the bounce
class Bounce:
    """What the kernel does after a hit, as far as the law knows it.
    kind: the group's name; end: the sample ends here; d: the next direction where
    the law gives it exactly (else None); dithered: the next direction came
    through dither64; approx: (law, calibration) of a direction held under the
    4 x rule; lost: an f32 decision too close to its threshold -- the RNG stream
    past this bounce is not known."""

    def __init__(self, kind, end=False, d=None, dithered=False, approx=None, lost=False, lamb=None, albedo=None):
        self.kind, self.end, self.d, self.dithered = kind, end, d, dithered
        self.approx, self.lost, self.lamb, self.albedo = approx, lost, lamb, albedo


class Replay:
    def __init__(self, soa, cam, seed, f32=True):
        self.sc = Scene(soa, f32)
        self.cam, self.seed, self.f32 = cam, seed, f32
        self.W = cam["image_width"]
        self.scale = RS.uniform_inclusive_scale(-0.5, 0.5)

    # ---- the camera ray: the draws (and in f64 the ray itself, camera.rs:274-293)
    def start(self, i, j, s):
        cam = self.cam
        g = RS.Rng(self.seed, j * self.W + i, s)
        if self.f32:
            g.next_u64()
            g.next_u64()
            assert cam["defocus_angle"] <= EPS, "the f32 replay takes pinhole cameras"
            return g, v32(cam["center"]), None
        ox, oy = g.uniform(-0.5, self.scale), g.uniform(-0.5, self.scale)
        ps = RS.add(RS.add(cam["pixel00_loc"], RS.muls(cam["pixel_delta_u"], float(i) + ox)),
                    RS.muls(cam["pixel_delta_v"], float(j) + oy))
        if cam["defocus_angle"] <= EPS:
            origin = cam["center"]
        else:
            p = RS.unit_disk(g)
            origin = RS.add(RS.add(cam["center"], RS.muls(cam["defocus_disk_u"], p[0])),
                            RS.muls(cam["defocus_disk_v"], p[2]))
        return g, origin, RS.sub(ps, origin)

    # ---- Metal / Dielectric in f64 (specular_dir64)
    def _specular64(self, g, d, n, front, m, metal):
        M = self.sc.mat64[m]
        words = None
        if metal:
            if self.f32:
                words = (g.next_u64(), g.next_u64(), g.next_u64())
                us = None
            else:
                us = RS.unit_sphere(g)
        u = RS.normalize(d)
        vn = RS.dot(u, n)
        r = (u[0] - (n[0] * 2.0) * vn, u[1] - (n[1] * 2.0) * vn, u[2] - (n[2] * 2.0) * vn)
        if metal:
            fuzz = M[3]
            if us is None and fuzz == 0.0:
                us = (0.0, 0.0, 0.0)           # (r + us * 0 = r for every finite us)
            if us is not None:
                out = (r[0] + us[0] * fuzz, r[1] + us[1] * fuzz, r[2] + us[2] * fuzz)
                keep = RS.dot(out, n) > 0.0
                name = "metal fuzz 0" if fuzz == 0.0 else "metal fuzz > 0"
                return Bounce(name if keep else "metal absorbed", end=not keep, d=out if keep else None,
                              albedo=self.sc.albedo[m])
            law, cal = unit_sphere_f32(*words), unit_sphere_f32(*words, calib=True)
            out = (r[0] + law[0] * fuzz, r[1] + law[1] * fuzz, r[2] + law[2] * fuzz)
            k = RS.dot(out, n)
            return Bounce("metal fuzz > 0" if k > 0.0 else "metal absorbed", end=not k > 0.0, lost=abs(k) < NEAR,
                          approx=(r, fuzz, law, cal), albedo=self.sc.albedo[m])
        ratio = M[0] if front else M[3]
        cos_t = RS.fmin(-vn, 1.0)
        sin_t = RS.sqrt(1.0 - cos_t * cos_t)
        face = "front" if front else "back"
        if ratio * sin_t > 1.0:
            return Bounce("dielectric TIR " + face, d=r)
        r0 = M[1] if front else M[2]
        x = 1.0 - cos_t
        x2 = x * x
        if r0 + (1.0 - r0) * (x * (x2 * x2)) > g.open01():
            return Bounce("dielectric Schlick reflect " + face, d=r)
        px, py, pz = (u[0] + n[0] * cos_t) * ratio, (u[1] + n[1] * cos_t) * ratio, (u[2] + n[2] * cos_t) * ratio
        q = -RS.sqrt(1.0 - (px * px + py * py + pz * pz))
        return Bounce("dielectric refract " + face, d=(px + n[0] * q, py + n[1] * q, pz + n[2] * q))

    # ---- Metal / Dielectric on a plane: the f32 kernel's own f32 scatter; the law
    # (the f32 form in f64 on the f32 inputs) decides the draws and the absorption
    def _specular32(self, g, d, n, m, metal):
        d, mp = v32(d), self.sc.mat_params[m]
        unit = RS.normalize(d)
        if metal:
            us = unit_sphere_f32(g.next_u64(), g.next_u64(), g.next_u64())
            out = RS.add(RS.reflect(unit, n), RS.muls(us, r32(mp[3])))
            k = RS.dot(out, n)
            return Bounce("plane metal" if k > 0.0 else "plane metal absorbed", end=not k > 0.0, dithered=True,
                          lost=abs(k) < NEAR, albedo=self.sc.albedo[m])
        ratio = r32(mp[4])                       # a plane is hit from behind only: front is false
        cos_t = RS.fmin(RS.dot(unit, RS.neg(n)), 1.0)
        k = ratio * RS.sqrt(1.0 - cos_t * cos_t)
        if not k > 1.0:
            g.next_u64()
        return Bounce("plane dielectric", dithered=True, lost=abs(k - 1.0) < NEAR)

    def bounce(self, g, d, p, n, front, m, sphere):
        """The scatter of a hit at p with the flipped normal n (f32 replay: the f64
        normal of a sphere, a plane's f32 normal negated) of material m."""
        sc = self.sc
        t = sc.mat_type[m]
        if t in (METAL, DIELECTRIC):
            if sphere or not self.f32:
                return self._specular64(g, d, n, front, m, t == METAL)
            return self._specular32(g, d, n, m, t == METAL)
        if t != LAMBERTIAN:
            return Bounce("invisible", end=True)
        where = "sphere" if sphere else "plane"
        w = g.next_u64()
        to_light = (w >> 63) == 0 if self.f32 else (w >> 11) * (1.0 / 9007199254740992.0) < 0.5
        L, lsel = (0.0, 0.0, 0.0, 0.0), -1
        if to_light:
            assert sc.lights, "the replay takes scenes with a light list"
            lsel = g.gen_index(len(sc.lights))
            L = sc.lights[lsel]
        r1, r2 = g.standard(), g.standard()
        out = mixture_direction(to_light, n, L[:3], L[3], p, r1, r2)
        return Bounce(f"lambertian {'to light' if to_light else 'cosine'} {where}", d=out,
                      lamb=(to_light, n, L, p, r1, r2, lsel), albedo=sc.albedo[m])


def host_sample(rp, world, i, j, s, kinds=None):
    """One sample by the driver in its f64 mode, the hits from restate.World.hit:
    ((r, g, b), segments) as restate.trace_sample returns them."""
    cam = rp.cam
    g, o, d = rp.start(i, j, s)
    mult, res = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    segments = 0
    for depth in range(cam["max_depth"], -1, -1):
        if depth == 0:
            return RS.add((0.0, 0.0, 0.0), res), segments
        rec = world.hit(o, d)
        segments += 1
        if rec is None:
            return RS.add(RS.mulv(mult, cam["background"]), res), segments
        mtype = world.mat_type[rec.mat]
        emitted = world.colour(rec.mat, rec.u, rec.v, rec.p) if mtype == DIFFUSE_LIGHT else (0.0, 0.0, 0.0)
        b = rp.bounce(g, d, rec.p, rec.normal, rec.front, rec.mat, True)   # (f64 mode: one scatter path for planes too)
        if kinds is not None:
            kinds.add(b.kind)
        if b.end:
            return RS.add(RS.mulv(mult, emitted), res), segments
        if b.lamb is not None:
            w = lambert_weight(b.albedo, rec.normal, b.d, world.lights_pdf(rec.p, b.d))
            res = RS.add(res, RS.mulv(mult, emitted))
            mult = RS.mulv(mult, w)
        elif mtype == METAL:
            mult = RS.mulv(mult, b.albedo)
        else:
            mult = RS.mulv(mult, (1.0, 1.0, 1.0))
        o, d = rec.p, b.d
    raise AssertionError("unreachable")


def lambert_weight(att, n, dirn, lpdf):
    """camera.rs:504-521 in the reference's form: att * scattering pdf / mixture pdf"""
    w = RS.normalize(n)
    nd = RS.normalize(dirn)
    cosine_value = RS.fmax(RS.fdiv(RS.dot(nd, w), RS.PI), 0.0)
    pdf = lpdf * 0.5 + cosine_value * 0.5
    spdf = RS.fmax(RS.fdiv(RS.dot(n, nd), RS.PI), 0.0)
    return RS.divs(RS.muls(att, spdf), pdf)


# ------------------------------------------------------- judging a traced render
class Report:
    """Per group: rows checked, rows that failed an exact check, rows left out (with
    the reason), and the (kernel, calibration) errors of the rows under the 4 x rule."""

    def __init__(self):
        self.rows, self.fails, self.out, self.err, self.agreed, self.tag = {}, {}, {}, {}, {}, ""

    def exact(self, group, ok, detail=None):
        self.rows[group] = self.rows.get(group, 0) + 1
        if not ok:
            self.fails.setdefault(group, []).append((self.tag, detail))

    def count(self, group):
        self.rows[group] = self.rows.get(group, 0) + 1

    def leave_out(self, group, why):
        self.out.setdefault(group, []).append(dict(why, tag=self.tag))

    def errors(self, group, kernel, calib):
        self.rows[group] = self.rows.get(group, 0) + 1
        self.err.setdefault(group, []).append((kernel, calib))


def _vabs(a, b):
    return max(abs(float(x) - float(y)) for x, y in zip(a, b))


def judge_sample(rp, rep, i, j, s, seg, colrec, coop=False, path=None):
    """Replay sample s of pixel (i, j) against its traced segments seg [64, 12] and
    its end record colrec [4]; returns the replay's segment count, or None where
    an f32 decision too close to its threshold ended the replay early."""
    sc, cam = rp.sc, rp.cam
    g, origin, _ = rp.start(i, j, s)
    path = [] if path is None else path           # the colour's steps: ("L", ...) / ("M", albedo) / ("end", miss)
    n_traced = int((seg[:, 0] != -2.0).sum())
    max_depth = cam["max_depth"]
    prev_self, dithered, want_o, want_d = -1, True, origin, None
    for k in range(max_depth):
        r = seg[k]
        if r[0] == -2.0:
            rep.exact("segment count", False, (i, j, s, k, "the trace ends before the replay"))
            return k
        obj, t, o, d, tb = int(r[0]), float(r[1]), tuple(map(float, r[2:5])), tuple(map(float, r[5:8])), float(r[8])
        self_s, at = int(r[9]), (i, j, s, k)
        # ---- the ray as the previous transition left it
        rep.exact("ray origin is the f64 hit point", same(o, want_o), at)
        if want_d is not None:
            rep.exact("exact direction", same(d, want_d), at)
        if dithered:
            rep.exact("dither64", is_dithered(d), at)
        rep.exact("own sphere carried", self_s == prev_self and int(r[11]) == max_depth - k, at)
        # ---- the hit: the own sphere's f64 re-hit, the winner's f64 t
        own = self_s >= 0 and obj == sc.sbase + self_s
        if self_s >= 0:
            ok, ts = sphere_t_ref64(sc.sph64[self_s], o, d)
            if own:
                rep.exact("own-sphere re-hit taken", ok and bits(ts) == bits(t) and r32(ts) == tb, at)
            else:
                rep.exact("own-sphere re-hit refused", not ok or (obj >= 0 and tb <= r32(ts)), at)
        if obj >= sc.sbase and not own:
            ok, ts = sphere_t_ref64(sc.sph64[obj - sc.sbase], o, d)
            rep.exact("other sphere", bits(t) == bits(ts if ok else tb), at)
            if not ok:
                rep.count("other sphere: f32 t kept")
        elif 0 <= obj < sc.n_planes:
            rep.exact("plane", bits(t) == bits(plane_t_ref64(sc.pl64[obj], o, d)), at)
        # ---- the object picked, against the f64 brute force
        hits = sc.closest64(o, d)
        group = "picked: " + ("miss" if obj < 0 else "own sphere" if own else "plane" if obj < sc.sbase else "sphere")
        first = hits[0][1] if hits else -1
        if first == obj:
            rep.exact(group, True)
            if obj >= sc.sbase and rep.rows[group] % 16 == 0:      # every 16th: the margin's calibration rows
                rep.agreed.setdefault(group, []).append(dict(obj=obj, o=o, d=d, tag=rep.tag))
        else:
            rep.count(group)
            rep.leave_out(group, dict(at=at, obj=obj, t=t, first=first, hits=hits[:3], o=o, d=d, self_s=self_s))
        if obj < 0:
            rep.exact("termination: miss", n_traced == k + 1 and colrec[3] == max_depth - k, at)
            path.append(("end", True))
            return k + 1
        # ---- the hit point, the normal, the scatter
        p = ray_at64(o, d, t)
        m = sc.material(obj)
        if obj >= sc.sbase:
            n = sphere_normal64(p, sc.sph64[obj - sc.sbase])
            front = front64(d, n)
            if not front:
                n = RS.neg(n)
            prev_self = obj - sc.sbase
        else:
            n, front, prev_self = RS.neg(sc.pl[obj][1]), False, -1
        b = rp.bounce(g, d, p, n, front, m, obj >= sc.sbase)
        if b.lost:
            rep.count(b.kind)
            rep.leave_out(b.kind, dict(at=at, why="an f32 decision within %g of its threshold" % NEAR))
            return None
        if b.end:
            rep.exact("termination: " + b.kind, n_traced == k + 1 and colrec[3] == max_depth - k, at)
            path.append(("end", False))
            return k + 1
        if k + 1 == max_depth:
            rep.exact("termination: depth exhausted", n_traced == max_depth and colrec[3] == 0.0, at)
            path.append(("end", False))
            return max_depth
        nxt = seg[k + 1]
        if nxt[0] == -2.0:
            rep.exact("termination: " + b.kind, False, (at, "the trace ends where the replay goes on"))
            return k + 1
        nd = tuple(map(float, nxt[5:8]))
        want_o, want_d, dithered = p, None, b.dithered
        if b.lamb is not None:
            path.append(("L", obj, p, d, nd, b.lamb[6], m))
        elif b.albedo is not None:
            path.append(("M", b.albedo))
        if b.lamb is not None:
            # bit for bit where the kernel's arithmetic is the no-FMA law's; else under the 4 x rule
            law = mixture_direction(*b.lamb[:2], b.lamb[2][:3], b.lamb[2][3], *b.lamb[3:6], ld=True)
            if any(x != x for x in b.d):
                # (a point inside its light sphere: sqrt of a negative) the NaN pattern is the law's
                rep.exact("lambertian NaN direction", [x != x for x in nd] == [x != x for x in b.d], at)
            else:
                rep.errors(b.kind, (_vabs(nd, law), same(nd, b.d)), _vabs(b.d, law))
            if coop:
                rep.count("stash round trip (" + b.kind.split()[1] + ")")
        elif b.approx is not None:
            refl, fuzz, law, cal = b.approx
            got = tuple((nd[q] - refl[q]) / fuzz for q in range(3))
            rep.errors(b.kind, (_vabs(got, law), False), _vabs(cal, law))
        elif b.d is not None:
            want_d = b.d
            rep.count(b.kind)
        else:
            rep.count(b.kind)
    raise AssertionError("unreachable")


def judge_render(rp, rep, name, pixels, seg, col, base=None, coop=False):
    """Every traced sample of one render.  Samples whose records equal `base`'s (the
    scene's first variant, judged in full) bit for bit are not replayed again.
    Returns (samples, samples equal to base's, samples whose replay ended early)."""
    rep.tag = name
    same_n = lost = 0
    paths = {}
    for k, (i, j) in enumerate(pixels):
        for s in range(seg.shape[1]):
            if base is not None and np.array_equal(seg[k, s], base[0][k, s], equal_nan=True) and \
                    col[k, s, 3] == base[1][k, s, 3]:
                same_n += 1
                if (k, s) in base[2]:
                    paths[k, s] = base[2][k, s]
                continue
            path = []
            n = judge_sample(rp, rep, i, j, s, seg[k, s], col[k, s], coop, path)
            if n is None:
                lost += 1
            else:
                rep.exact("segment count", int((seg[k, s, :, 0] != -2.0).sum()) == n, (i, j, s, n))
                paths[k, s] = path
    return (len(pixels) * seg.shape[1], same_n, lost), paths


def colour_laws(rp, paths, kernel):
    """The samples' colours along their traced paths: the mult recurrence of the render
    (camera.rs:459-522 as render_kernel.hpp computes it in f32: the Lambertian weight
    att * spdf / (lpdf / 2 + cos / 2) with the light pdf of the f32 two-pass test,
    Metal's albedo, the background at a miss, black at every other end) in f64 on
    the f32 inputs (the law) and in f32 (the calibration).
    Returns (keys, law [n, 3], calib [n, 3], margin [n]): margin is the smallest
    decision margin of the sample's Lambertian bounces in the law (a light's hit test,
    the face of the f32 normal)."""
    import f32_forms as FF
    sc = rp.sc
    rows = [(key, st) for key, path in paths.items() for st in path if st[0] == "L"]
    robust = bool(kernel[1] & 1)
    keep_sampled = kernel[0] == 5 and not kernel[1] & 2      # lights_pdf_sum_pk(..., lsel): the sampled light counts
    bg = v32(rp.cam["background"])
    out = {}
    for dtype in (np.float64, np.float32):
        F = FF.Forms(dtype)
        with np.errstate(all="ignore"):
            if rows:
                obj = np.array([st[1] for _, st in rows])
                p = FF.v3(F.arr(np.array([v32(st[2]) for _, st in rows])))
                d_in = FF.v3(F.arr(np.array([v32(st[3]) for _, st in rows])))
                d_out = FF.v3(F.arr(np.array([v32(st[4]) for _, st in rows])))
                lsel = np.array([st[5] for _, st in rows])
                att = FF.v3(F.arr(np.array([sc.albedo[st[6]] for _, st in rows])))
                sph = obj >= sc.sbase
                geo = np.array([sc.sph[o - sc.sbase] if o >= sc.sbase else sc.pl[o][1] + (1.0,) for o in obj])
                g3 = FF.v3(F.arr(geo[:, :3]))
                outward = FF.where3(sph, F.divs(FF.sub(p, g3), F.arr(geo[:, 3])), g3)
                dn = FF.dot(d_in, outward)
                front = np.where(sph, dn < 0, False)
                nrm = FF.where3(front, outward, FF.neg(outward))
                ndir, wn = F.normalize(d_out), F.normalize(nrm)
                cos_w = F.over_pi(FF.dot(ndir, wn))
                spdf = np.fmax(F.over_pi(FF.dot(nrm, ndir)), F.zero)
                acc = np.zeros(len(rows), F.dt)
                margin = np.where(sph, np.abs(dn) / np.sqrt(FF.dot(d_in, d_in) * FF.dot(outward, outward)), np.inf)
                for k, L in enumerate(sc.lights):
                    c, r = FF.v3(F.arr(np.array(L[:3]))), F.dt(L[3])
                    hit, mg = FF.light_hit_f32(F, c, r, p, d_out, robust)
                    if keep_sampled:
                        hit, mg = hit | (lsel == k), np.where(lsel == k, np.inf, mg)
                    acc = np.where(hit, acc + FF.light_pdf_f32(F, c, r, p), acc)
                    margin = np.fmin(margin, mg)
                lpdf = F.div(acc, F.dt(len(sc.lights)))
                pdf = lpdf * F.dt(0.5) + np.fmax(cos_w, F.zero) * F.dt(0.5)
                w = np.stack(F.divs(FF.mulv(att, (spdf, spdf, spdf)), pdf), -1)
            at = {}
            for n, (key, st) in enumerate(rows):
                at[id(st)] = n
            cols, margins = [], []
            for key, path in paths.items():
                mult, mg = np.ones(3, F.dt), np.inf
                for st in path:
                    if st[0] == "L":
                        mult, mg = mult * w[at[id(st)]], min(mg, float(margin[at[id(st)]]))
                    elif st[0] == "M":
                        mult = mult * F.arr(np.array(st[1]))
                    else:
                        mult = mult * (F.arr(np.array(bg)) if st[1] else F.zero) + F.zero
                cols.append(mult)
                margins.append(mg)
        out[dtype] = (np.array(cols, np.float64).reshape(-1, 3), np.array(margins))
    return list(paths), out[np.float64][0], out[np.float32][0], out[np.float64][1]
