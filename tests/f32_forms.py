"""The f32 (speed) mode's arithmetic, restated in numpy and generic over the
dtype -- TEST INFRASTRUCTURE ONLY.

Written from the kernels' device code (csrc/rtw_device.hpp, bvh_traverse.hpp,
light_pdf.hpp, query_kernel.hpp, nee_kernel.hpp, path_kernel.hpp,
render_kernel.hpp) as it reads for R = float, the f32-only branches included:
a * rcp(b) divisions, rsq normalisation, sin / cos in revolutions, the unit
ball by inversion, the cancellation-free x / (1 + sqrt(1 - x)) forms, the
two-pass light test.  Every function takes `dtype`; every intermediate is held
in that dtype; each multiply and each add is its own numpy operation (no fused
form, no np.dot).  Brute force over the primitives: no BVH, no grid.

Two evaluations of this one code serve tests/test_gpu_f32_records.py:

  the law          dtype = float64 on the inputs as the f32 kernel sees them
                   (f32 rays, records and staged scene values upcast exactly,
                   the 24- and 23-bit uniforms): what the f32 form means, free
                   of rounding -- the truth the kernel is compared with
  the calibration  dtype = float32, numpy's correctly rounded operations: what
                   a faultless f32 implementation of the same form loses to
                   rounding and conditioning on these very rows

Transcendentals (sin / cos of an azimuth, atan2, acos, log2 / exp2, sinf) are
evaluated in float64 and rounded once to the dtype: a correctly rounded
library call, not a restatement of an instruction.

With f32_form=False every function takes the reference's form instead (IEEE
division, 1 - sqrt(1 - x), the rejection samplers, the fdlibm sin / cos
kernels of tests/indep/restate.py); on f64 inputs with f64's uniforms
(bits32=False) that evaluation equals tests/indep/restate.py bit for bit
(tests/test_f32_forms_host.py), which ties this file to the independent
restatement.

sphere_uv clamps the argument of acos to [-1, 1] in the f32 form, as the f32
kernel does: at the pole of a large sphere (r = 1000) f32 rounding lifts
(p - c) * rcp(r) an ulp above 1, where acos is NaN -- the law's own point lies
on the sphere to f64 rounding and never needs the clamp, the calibration does.
The reference's form (f32_form=False) is the reference's: unclamped.

Staging (stage()): host/stage_scene.cpp derives a quad's normal, w and area,
a cuboid's six quads, rotation, inverse and boxes and a plane's UV constants
in f64 and rounds them to the kernel's precision; a sphere's r^2 is the
rounded radius squared IN the kernel's precision.  stage(soa, store) rounds
exactly those to `store`, so the law and the kernel start from the same
numbers.  The f64 derivations are tests/indep/restate.py's constructors.
"""
from __future__ import annotations

import math

import numpy as np

from indep import restate as RS

EPS = 2.220446049250313e-16
LAMBERTIAN, METAL, DIELECTRIC, INVISIBLE, DIFFUSE_LIGHT = 0, 1, 2, 3, 4
MISS, ABSORBED, REFLECT, SCATTER = 0, 1, 2, 3
PRIM_PLANE, PRIM_QUAD, PRIM_CUBOID, PRIM_SPHERE = 0, 1, 2, 3
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------ vectors
def v3(a):
    return (a[..., 0], a[..., 1], a[..., 2])


def stack3(a):
    return np.stack(np.broadcast_arrays(*a), -1)


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def neg(a):
    return (-a[0], -a[1], -a[2])


def muls(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def mulv(a, b):
    return (a[0] * b[0], a[1] * b[1], a[2] * b[2])


def dot(a, b):                       # (x x' + y y') + z z'
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def where3(m, a, b):
    return (np.where(m, a[0], b[0]), np.where(m, a[1], b[1]), np.where(m, a[2], b[2]))


class Forms:
    """The precision-specific primitives (rtw_device.hpp P<R>) for one dtype."""

    def __init__(self, dtype, f32_form=True):
        self.dt, self.f32 = np.dtype(dtype).type, bool(f32_form)
        self.one, self.zero, self.two = self.dt(1), self.dt(0), self.dt(2)
        self.pi, self.tau = self.dt(math.pi), self.dt(2 * math.pi)
        self.inv_pi, self.inv_tau = self.dt(1 / math.pi), self.dt(0.159154943091895335769)
        self.inf = self.dt(np.inf)

    def arr(self, x):
        return np.asarray(x).astype(self.dt)

    def lib(self, fn, *x):           # a correctly rounded library call
        with np.errstate(all="ignore"):
            return fn(*[np.asarray(a, np.float64) for a in x]).astype(self.dt)

    def rcp(self, b):
        return self.one / b

    def div(self, a, b):             # P<float>::div_: a * rcp(b)
        return a * self.rcp(b) if self.f32 else a / b

    def over_pi(self, a):
        return a * self.inv_pi if self.f32 else a / self.pi

    def sqrt(self, x):
        return np.sqrt(x)

    def normalize(self, a):
        l2 = dot(a, a)
        if self.f32:                 # k = rsq(a . a)
            return muls(a, self.rcp(np.sqrt(l2)))
        l = np.sqrt(l2)
        return (a[0] / l, a[1] / l, a[2] / l)

    def divs(self, a, s):
        if self.f32:
            return muls(a, self.rcp(s))
        return (a[0] / s, a[1] / s, a[2] / s)

    def sincos_2pi(self, r):
        if self.f32:                 # v_sin / v_cos take revolutions
            x = np.asarray(r, np.float64) * (2 * math.pi)
            return np.sin(x).astype(self.dt), np.cos(x).astype(self.dt)
        return _sincos_2pi_fdlibm(r)

    def reflect(self, v, n):
        d = dot(v, n)
        return sub(v, muls(muls(n, self.two), d))

    def refract(self, v, n, eta):
        cos_theta = np.fmin(dot(v, neg(n)), self.one)
        perp = muls(add(v, muls(n, cos_theta)), eta)
        par = muls(n, -np.sqrt(self.one - dot(perp, perp)))
        return add(perp, par)

    def onb(self, n):                # geometry/src/onb.rs (rtw_device.hpp Onb)
        w = self.normalize(n)
        big = np.abs(w[0]) > 0.9
        a = (np.where(big, self.zero, self.one), np.where(big, self.one, self.zero), np.zeros_like(w[0]))
        v = self.normalize(cross(w, a))
        return cross(w, v), v, w

    def onb_transform(self, f, x):
        acc = (np.zeros_like(x[0]),) * 3
        acc = add(acc, muls(f[0], x[0]))
        acc = add(acc, muls(f[1], x[1]))
        return add(acc, muls(f[2], x[2]))


# fdlibm kernels on arrays (restate.sincos_2pi, operation for operation)
_S, _C = RS._S, RS._C


def _sincos_2pi_fdlibm(r):
    r = np.asarray(r, np.float64)
    q = np.rint(r * 4.0)
    f = r - q * 0.25
    x = f * (2.0 * math.pi)
    z = x * x
    v = z * x
    rr = _S[1] + z * (_S[2] + z * (_S[3] + z * (_S[4] + z * _S[5])))
    ks = x + v * (_S[0] + z * rr)
    rc = z * (_C[0] + z * (_C[1] + z * (_C[2] + z * (_C[3] + z * (_C[4] + z * _C[5])))))
    ax = np.abs(x)
    b = (ax.view(np.uint64) - np.uint64(0x0020000000000000)) & np.uint64(0xFFFFFFFF00000000)
    qx = np.where(ax > 0.78125, 0.28125, b.view(np.float64))
    hz = 0.5 * z - qx
    kc = np.where(ax < 0.3, 1.0 - (0.5 * z - z * rc), (1.0 - qx) - (hz - z * rc))
    k = q.astype(np.int64) & 3
    s = np.select([k == 0, k == 1, k == 2], [ks, kc, -ks], -kc)
    c = np.select([k == 0, k == 1, k == 2], [kc, -ks, -kc], ks)
    return s, c


def _exp_bits(x):
    return (int(np.float64(x).view(np.uint64)) >> 52) & 0x7FF


def _fdlibm_sin(x):
    """f64::sin as the f64 kernels and the oracle compute it (rtw_device.hpp rt_sin): fdlibm's
    medium Cody-Waite reduction by pi / 2 and __kernel_sin / __kernel_cos with the tail"""
    def k_sin(x, y):
        z = x * x
        v = z * x
        r = _S[1] + z * (_S[2] + z * (_S[3] + z * (_S[4] + z * _S[5])))
        return x - ((z * (0.5 * y - v * r) - y) - v * _S[0])

    def k_cos(x, y):
        z = x * x
        r = z * (_C[0] + z * (_C[1] + z * (_C[2] + z * (_C[3] + z * (_C[4] + z * _C[5])))))
        ax = abs(x)
        if ax < 0.3:
            return 1.0 - (0.5 * z - (z * r - x * y))
        if ax > 0.78125:
            qx = 0.28125
        else:
            b = (int(np.float64(ax).view(np.uint64)) - 0x0020000000000000) & 0xFFFFFFFF00000000
            qx = float(np.uint64(b).view(np.float64))
        hz = 0.5 * z - qx
        return (1.0 - qx) - (hz - (z * r - x * y))

    ax = abs(x)
    if ax <= 0.78539816339744828:
        return k_sin(x, 0.0)
    if not ax < 823549.6:
        return math.sin(x)
    n = int(ax * 6.36619772367581382433e-01 + 0.5)
    fn = float(n)
    r = ax - fn * 1.57079632673412561417e+00
    w = fn * 6.07710050650619224932e-11
    y0 = r - w
    j = _exp_bits(ax)
    if j - _exp_bits(y0) > 16:
        t = r
        w = fn * 6.07710050630396597660e-11
        r = t - w
        w = fn * 2.02226624879595063154e-21 - ((t - r) - w)
        y0 = r - w
        if j - _exp_bits(y0) > 49:
            t = r
            w = fn * 2.02226624871116645580e-21
            r = t - w
            w = fn * 8.47842766036889956997e-32 - ((t - r) - w)
            y0 = r - w
    y1 = (r - y0) - w
    q = n
    if x < 0.0:
        y0, y1, q = -y0, -y1, -n
    return (k_sin(y0, y1), k_cos(y0, y1), -k_sin(y0, y1), -k_cos(y0, y1))[q & 3]


# ---------------------------------------------------------------------- RNG
def _u64(x):
    return np.uint64(x & 0xFFFFFFFFFFFFFFFF)


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * _u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * _u64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _rotl(x, k):
    return (x << np.uint64(k)) | (x >> np.uint64(64 - k))


def rng_seed(seed, pixel, sample):
    """xoshiro256++ states [n, 4] of the streams (seed, pixel[k], sample)"""
    with np.errstate(over="ignore"):
        pixel = np.asarray(pixel, np.uint64)
        g = _u64(0x9E3779B97F4A7C15)
        k = _mix64(_u64(seed) + g * (pixel + np.uint64(1)))
        k = _mix64(k ^ (_u64(0xD1B54A32D192ED03) * _u64(sample + 1)))
        s = np.zeros((len(pixel), 4), np.uint64)
        for q in range(4):
            k = k + g
            s[:, q] = _mix64(k)
    return s


def rng_next(s, mask=None):
    """One xoshiro256++ step of the rows in `mask` (all rows without one): the
    64-bit words [n] (0 for rows outside the mask); `s` [n, 4] is advanced in place."""
    with np.errstate(over="ignore"):
        s0, s1, s2, s3 = s[:, 0].copy(), s[:, 1].copy(), s[:, 2].copy(), s[:, 3].copy()
        result = _rotl(s0 + s3, 23) + s0
        t = s1 << np.uint64(17)
        s2 ^= s0
        s3 ^= s1
        s1 ^= s2
        s0 ^= s3
        s2 ^= t
        s3 = _rotl(s3, 45)
    new = np.stack([s0, s1, s2, s3], 1)
    if mask is None:
        s[:] = new
        return result
    s[mask] = new[mask]
    return np.where(mask, result, np.uint64(0))


def rng_index(s, n, mask=None):
    """gen_range(0..n) on u32 (rand 0.8.6): widening multiply and zone"""
    n = int(n)
    zone = ((n << (32 - n.bit_length())) & 0xFFFFFFFF) - 1
    pend = np.ones(len(s), bool) if mask is None else mask.copy()
    out = np.zeros(len(s), np.int64)
    while pend.any():
        v = rng_next(s, pend) >> np.uint64(32)
        m = v * np.uint64(n)
        ok = pend & ((m & np.uint64(0xFFFFFFFF)) <= np.uint64(zone))
        out[ok] = (m >> np.uint64(32))[ok].astype(np.int64)
        pend &= ~ok
    return out


class Uniforms:
    """The uniforms on top of the words: the f32 mode's (bits32: u_std 24 bits,
    u_open01 23 bits + 2^-24, u_incl without scale) or rand 0.8.6's for f64."""

    def __init__(self, F, bits32=True):
        self.F, self.b32 = F, bool(bits32)

    def _unit12(self, v):
        return ((v >> np.uint64(12)) | np.uint64(0x3FF0000000000000)).view(np.float64)

    def std(self, v):
        dt = self.F.dt
        if self.b32:
            return (v >> np.uint64(40)).astype(dt) * dt(2.0 ** -24)
        return (v >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)

    def open01(self, v):
        dt = self.F.dt
        if self.b32:
            return (v >> np.uint64(41)).astype(dt) * dt(2.0 ** -23) + dt(2.0 ** -24)
        return self._unit12(v) - (1.0 - EPS / 2.0)

    def incl(self, v, low, scale):
        dt = self.F.dt
        if self.b32:
            return (v >> np.uint64(40)).astype(dt) * dt(2.0 ** -24) + dt(low)
        return (self._unit12(v) - 1.0) * scale + low


# ------------------------------------------------------------------ staging
def _rnd(x, store):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(store).astype(np.float64)


def _outward(x, store, up):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        r = x.astype(store)
    bad = (r.astype(np.float64) < x) if up else (r.astype(np.float64) > x)
    r = np.where(bad, np.nextafter(r, store(np.inf if up else -np.inf)), r)
    return r.astype(np.float64)


def _quad_fields(qd, store):
    f = dict(q=qd.q, u=qd.u, v=qd.v, w=qd.w, n=qd.n)
    out = {k: _rnd(val, store) for k, val in f.items()}
    out["area"] = float(_rnd(qd.area, store))
    out["lo"], out["hi"] = _outward(qd.aabb.lo, store, False), _outward(qd.aabb.hi, store, True)
    return out


class Staged:
    """The scene as a kernel of precision `store` sees it (values held in float64)."""


def stage(soa, store=np.float32):
    S = Staged()
    store = np.dtype(store).type
    S.store = store
    S.eps = float(store(EPS))
    # planes: {point, normal (as given), box, the UV constants} -- stage_scene.cpp
    S.planes = []
    for p in np.asarray(soa.planes, np.float64).reshape(-1, 6):
        n = tuple(map(float, p[3:6]))
        pin = [abs(n[(k + 1) % 3]) < EPS and abs(n[(k + 2) % 3]) < EPS for k in range(3)]
        c = RS.cross(n, (0.0, 1.0, 0.0))
        clen = RS.length(c)
        theta = math.atan2(clen, RS.dot(n, (0.0, 1.0, 0.0)))
        kv = RS.divs(c, clen)
        kfin = all(math.isfinite(x) for x in kv)
        S.planes.append(dict(p=_rnd(p[:3], store), n=_rnd(n, store),
                             lo=np.array([0.0 if f else -np.inf for f in pin]),
                             hi=np.array([0.0 if f else np.inf for f in pin]),
                             mode=0 if theta <= EPS else (1 if kfin else 2),
                             ct=float(_rnd(math.cos(theta), store)), st=float(_rnd(math.sin(theta), store)),
                             k=_rnd(kv if kfin else (0.0, 0.0, 0.0), store)))
    S.plane_mat = np.asarray(soa.plane_mat, np.int64).reshape(-1)
    S.quads = [_quad_fields(RS.Quad(q[:3], q[3:6], q[6:9], 0), store)
               for q in np.asarray(soa.quads, np.float64).reshape(-1, 9)]
    S.quad_mat = np.asarray(soa.quad_mat, np.int64).reshape(-1)
    S.boxes = []
    for b in np.asarray(soa.boxes, np.float64).reshape(-1, 18):
        tc = RS.TransformedCuboid(b[0:3], b[3:6], (b[6:9], b[9:12], b[12:15]), b[15:18], 0)
        ok = tc.inv is not None
        Ri, Ti = tc.inv if ok else (((0.0,) * 3,) * 3, (0.0,) * 3)
        S.boxes.append(dict(quads=[_quad_fields(qd, store) for qd in tc.quads], rot=_rnd(tc.R, store),
                            t=_rnd(tc.T, store), inv=_rnd(Ri, store), ti=_rnd(Ti, store), ok=ok,
                            lo=_outward(tc.aabb.lo, store, False), hi=_outward(tc.aabb.hi, store, True)))
    S.box_mat = np.asarray(soa.box_mat, np.int64).reshape(-1)
    sp = np.asarray(soa.spheres, np.float64).reshape(-1, 4)
    S.sph_c = _rnd(sp[:, :3], store)
    r = sp[:, 3].astype(store)
    S.sph_r = r.astype(np.float64)
    S.sph_r2 = np.where(sp[:, 3] < 0, -np.inf, (r * r).astype(np.float64))    # r * r in the kernel's precision
    S.sphere_mat = np.asarray(soa.sphere_mat, np.int64).reshape(-1)
    S.n_planes, S.n_quads, S.n_boxes, S.n_sph = len(S.planes), len(S.quads), len(S.boxes), len(sp)
    S.bbase = S.n_planes + S.n_quads
    S.sbase = S.bbase + S.n_boxes
    # the light list
    li = np.asarray(soa.lights, np.float64).reshape(-1, 4)
    S.light_c, S.light_r = _rnd(li[:, :3], store), _rnd(li[:, 3], store)
    lq = np.zeros((0, 9)) if soa.light_quads is None else np.asarray(soa.light_quads, np.float64).reshape(-1, 9)
    S.lquads = [_quad_fields(RS.Quad(q[:3], q[3:6], q[6:9], 0), store) for q in lq]
    kinds = soa.light_kinds
    n_other = int(getattr(soa, "n_light_other", 0) or 0)
    if kinds is None:
        kinds = [0] * len(li) + [1] * len(lq)
    S.lref, ns, nq = [], 0, 0
    for k in map(int, kinds):
        if k == 0:
            S.lref.append(("sphere", ns))
            ns += 1
        elif k == 1:
            S.lref.append(("quad", nq))
            nq += 1
        else:
            S.lref.append(("default", 0))
    S.n_list = len(li) + len(lq) + n_other
    S.mixed = bool(len(lq) or n_other)
    S.leaf = bool(int(soa.light_flags) & 1)
    # materials and textures
    S.mat_type = np.asarray(soa.mat_type, np.int64).reshape(-1)
    mp = np.asarray(soa.mat_params, np.float64).reshape(-1, 5)
    w = np.where(S.mat_type == METAL, mp[:, 3], np.where(S.mat_type == DIELECTRIC, mp[:, 4], 0.0))
    S.mat_p = _rnd(np.concatenate([mp[:, :3], w[:, None]], 1), store)
    S.mat_tex = None if soa.mat_tex is None else np.asarray(soa.mat_tex, np.int64).reshape(-1)
    if S.mat_tex is not None:
        S.tex_type = np.asarray(soa.tex_type, np.int64).reshape(-1)
        S.tex_p = _rnd(np.asarray(soa.tex_params, np.float64).reshape(-1, 4), store)
        S.tex_refs = np.asarray(soa.tex_refs, np.int64).reshape(-1, 2)
        pv = getattr(soa, "perlin_vec", None)
        S.perlin_vec = None if pv is None else _rnd(np.asarray(pv, np.float64).reshape(-1, 3), store)
        pp = getattr(soa, "perlin_perm", None)
        S.perlin_perm = None if pp is None else np.asarray(pp, np.int64).reshape(-1)
    return S


def material_tables(S):
    """(material id, primitive kind) by object id"""
    mats = [S.plane_mat, S.quad_mat, S.box_mat, S.sphere_mat]
    return np.concatenate(mats), np.concatenate([np.full(len(m), k, np.int64) for k, m in enumerate(mats)])


# ------------------------------------------------------------- primitive tests
def aabb_hit(F, lo, hi, o, d, rs):
    """AABBox::hit over [rs, inf] (render_kernel.hpp aabb_hit_ref)"""
    lo, hi = F.arr(lo), F.arr(hi)
    with np.errstate(all="ignore"):
        def slab(k):
            t0, t1 = F.div(lo[k] - o[k], d[k]), F.div(hi[k] - o[k], d[k])
            sw = np.signbit(d[k])
            return np.where(sw, t1, t0), np.where(sw, t0, t1)
        tmin, tmax = slab(0)
        a0, a1 = slab(1)
        ok = ~((tmax < a0) | (tmin > a1))
        tmin, tmax = np.fmax(tmin, a0), np.fmin(tmax, a1)
        a0, a1 = slab(2)
        ok &= ~((tmax < a0) | (tmin > a1))
        tmin, tmax = np.fmax(tmin, a0), np.fmin(tmax, a1)
        return ok & (np.fmax(rs, tmin) <= np.fmin(F.inf, tmax))


def plane_t(F, pl, o, d, tmin, eps):
    n = v3(F.arr(pl["n"]))
    with np.errstate(all="ignore"):
        denom = dot(d, n)
        tt = -F.div(dot(sub(o, v3(F.arr(pl["p"]))), n), denom)
        return (denom > eps) & (tmin <= tt) & (tt <= F.inf), tt


def plane_uv(F, pl, pnt):
    if pl["mode"] == 0:
        return pnt[0], pnt[2]
    if pl["mode"] == 2:
        nan = np.full_like(pnt[0], np.nan)
        return nan, nan
    k = v3(F.arr(pl["k"]))
    vec = sub(pnt, v3(F.arr(pl["p"])))
    ct, st = F.dt(pl["ct"]), F.dt(pl["st"])
    with np.errstate(all="ignore"):
        rot = add(add(muls(vec, ct), muls(cross(k, vec), st)), muls(muls(k, dot(k, vec)), F.one - ct))
        return rot[0] - np.trunc(rot[0]), rot[2] - np.trunc(rot[2])


def quad_uv(F, Q, pq):
    w = v3(F.arr(Q["w"]))
    return dot(cross(pq, v3(F.arr(Q["v"]))), w), dot(cross(v3(F.arr(Q["u"])), pq), w)


def quad_t(F, Q, o, d, tmin, tmax, eps):
    """Quad::hit (rtw_device.hpp quad_t_hit): (hit, t, alpha, beta)"""
    n = v3(F.arr(Q["n"]))
    q = v3(F.arr(Q["q"]))
    with np.errstate(all="ignore"):
        denom = dot(d, n)
        tt = -F.div(dot(sub(o, q), n), denom)
        pq = sub(add(o, muls(d, tt)), q)
        al, be = quad_uv(F, Q, pq)
        hit = (np.abs(denom) > eps) & (tt >= tmin) & (tt <= tmax) & (al >= 0) & (al <= 1) & (be >= 0) & (be <= 1)
    return hit, tt, al, be


def mat3_mul(F, M, p):
    M = F.arr(M)
    return (dot(v3(M[0]), p), dot(v3(M[1]), p), dot(v3(M[2]), p))


def box_t(F, B, o, d, tmin, tmax, eps):
    """Transformed<Cuboid>::hit (render_kernel.hpp box_t_hit): (hit, t, quad, o2, d2, edge):
    the first minimum of the six quads; edge = the chosen quad's distance from its border"""
    ti = v3(F.arr(B["ti"]))
    o2 = add(mat3_mul(F, B["inv"], o), ti)
    d2 = add(mat3_mul(F, B["inv"], d), ti)
    n = len(o[0])
    bt, best, edge = np.full(n, np.inf, F.dt), np.full(n, -1, np.int64), np.full(n, np.inf, F.dt)
    if not B["ok"]:
        return best >= 0, bt, best, o2, d2, edge
    for k, Q in enumerate(B["quads"]):
        hit, tt, al, be = quad_t(F, Q, o2, d2, tmin, tmax, eps)
        upd = hit & ((best < 0) | (tt < bt))
        bt, best = np.where(upd, tt, bt), np.where(upd, k, best)
        with np.errstate(all="ignore"):
            e = np.minimum(np.minimum(np.abs(al), np.abs(F.one - al)), np.minimum(np.abs(be), np.abs(F.one - be)))
        near = np.isfinite(tt) & (tt >= tmin)
        edge = np.where(near, np.fmin(edge, e), edge)
    return best >= 0, bt, best, o2, d2, edge


def sphere_roots(F, c, r2, o, d, tmin, form):
    """The t of one sphere test and its discriminant normalised by the size of its
    terms (the decision's margin): form "t" = sphere_t (the reference's, with
    the dtype's division), "u" = sphere_u's discriminant form, "robust" =
    sphere_u's closest-approach form.  c: 3 arrays broadcastable against the rays'."""
    with np.errstate(all="ignore"):
        f = sub(o, c)
        if form == "t":
            a = dot(d, d)
            hb = dot(d, f)
            cc = dot(f, f) - r2
            disc = hb * hb - a * cc
            rel = disc / (hb * hb + np.abs(a * cc))
            sq = np.sqrt(disc)
            t0, t1 = F.div(-hb - sq, a), F.div(-hb + sq, a)
            pos = disc > 0
        else:
            a = d[2] * d[2] + (d[1] * d[1] + d[0] * d[0])                 # len2_f32
            ia = F.rcp(a)
            hb = d[2] * f[2] + (d[1] * f[1] + d[0] * f[0])
            if form == "robust":
                tc = -hb * ia
                l = add(muls(d, tc), f)
                l2 = l[0] * l[0] + (l[1] * l[1] + l[2] * l[2])
                disc = r2 - l2
                rel = disc / (np.abs(r2) + l2)
                h = np.sqrt(disc * ia)
                t0, t1 = tc - h, tc + h
            else:
                cc = f[0] * f[0] + (f[1] * f[1] + (f[2] * f[2] - r2))
                disc = hb * hb - a * cc
                rel = disc / (hb * hb + np.abs(a * cc))
                sq = np.sqrt(disc)
                nb = -hb * ia
                t0, t1 = nb - sq * ia, nb + sq * ia
            pos = ~np.isnan(t0)
        ok0 = pos & (t0 >= tmin) & (t0 <= F.inf)
        ok1 = pos & (t1 >= tmin) & (t1 <= F.inf)
        t = np.where(ok0, t0, np.where(ok1, t1, F.inf))
        return ok0 | ok1, t, rel


def sphere_uv(F, n):
    """get_sphere_uv; the f32 form clamps acos's argument by compares (a NaN stays NaN): see the
    module docstring"""
    if F.f32:
        y = np.where(n[1] > 1, F.one, np.where(n[1] < -1, -F.one, n[1]))
        return F.lib(np.arctan2, -n[2], n[0]) * F.inv_tau, F.lib(np.arccos, y) * F.inv_pi
    with np.errstate(all="ignore"):
        u = np.array([math.atan2(-z, x) for z, x in zip(n[2], n[0])], np.float64) / (2.0 * math.pi)
        v = np.array([math.acos(y) if -1.0 <= y <= 1.0 else math.nan for y in n[1]], np.float64) / math.pi
    return u, v


def closest_hit(S, rays, dtype, f32_form=True, sphere_form="u", t_min=None, chunk=2048):
    """world.hit(&r, t_min..=inf) and HitRecord::new (query_kernel.hpp
    hit_rays_kernel) for rays [n, 6]: a dict of id (-1: a miss), t, p, normal,
    outward, u, v, mat, front, kind, and the decisions' margins in this dtype:
      gap    (second smallest t - smallest t) / smallest t over all primitives
      rel    the hit sphere's normalised discriminant (inf for other kinds)
      near   the smallest |normalised discriminant| over ALL spheres (a silhouette nearby)
      edge   the smallest distance of a quad's (alpha, beta) from its border, over
             the quads and cuboid faces whose plane the ray meets in range
      facing |d . outward| / |d|"""
    F = Forms(dtype, f32_form)
    rays = F.arr(rays)
    outs = [_closest_hit(S, F, rays[k:k + chunk], sphere_form, t_min) for k in range(0, len(rays), chunk)]
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]} if outs else {}


def _closest_hit(S, F, rays, sphere_form, t_min):
    dt = F.dt
    n = len(rays)
    o, d = v3(rays[:, :3]), v3(rays[:, 3:])
    eps = dt(S.eps)
    tmin = eps if t_min is None else dt(S.store(t_min))
    tb, best = np.full(n, np.inf, dt), np.full(n, -1, np.int64)
    second, edge = np.full(n, np.inf, dt), np.full(n, np.inf, dt)

    def take(hit, t, ident):
        nonlocal tb, best, second
        t = np.where(hit, t, F.inf)
        upd = hit & ((best < 0) | (t < tb))
        second = np.where(upd, tb, np.fmin(second, t))
        tb, best = np.where(upd, t, tb), np.where(upd, ident, best)

    for q, pl in enumerate(S.planes):
        hit, t = plane_t(F, pl, o, d, tmin, eps)
        take(hit & aabb_hit(F, pl["lo"], pl["hi"], o, d, tmin), t, q)
    for q, Q in enumerate(S.quads):
        hit, t, al, be = quad_t(F, Q, o, d, tmin, F.inf, eps)
        with np.errstate(all="ignore"):
            e = np.minimum(np.minimum(np.abs(al), np.abs(F.one - al)), np.minimum(np.abs(be), np.abs(F.one - be)))
        edge = np.where(np.isfinite(t) & (t >= tmin), np.fmin(edge, e), edge)
        take(hit & aabb_hit(F, Q["lo"], Q["hi"], o, d, tmin), t, S.n_planes + q)
    box_rec = {}
    for q, B in enumerate(S.boxes):
        hit, t, qd, o2, d2, e = box_t(F, B, o, d, tmin, F.inf, eps)
        edge = np.fmin(edge, e)
        box_rec[q] = (t, qd, o2, d2)
        take(hit & aabb_hit(F, B["lo"], B["hi"], o, d, tmin), t, S.bbase + q)
    rel_hit, near = np.full(n, np.inf, dt), np.full(n, np.inf, dt)
    if S.n_sph:
        c = v3(F.arr(S.sph_c)[None, :, :])
        r2 = F.arr(S.sph_r2)[None, :]
        oo, dd = tuple(x[:, None] for x in o), tuple(x[:, None] for x in d)
        hit, t, rel = sphere_roots(F, c, r2, oo, dd, tmin, sphere_form)
        t = np.where(hit, t, F.inf)
        k = np.argmin(t, 1)                                # the first minimum: the lowest id on equal t
        rows = np.arange(n)
        ts = t[rows, k]
        t2 = t.copy()
        t2[rows, k] = np.inf
        with np.errstate(all="ignore"):
            near = np.nanmin(np.abs(np.where(np.isfinite(rel), rel, np.inf)), 1).astype(dt)
        shit = hit[rows, k]
        upd = shit & ((best < 0) | (ts < tb))
        second = np.fmin(np.where(upd, tb, np.fmin(second, ts)), t2.min(1))
        tb, best = np.where(upd, ts, tb), np.where(upd, S.sbase + k, best)
        rel_hit = np.where(upd, rel[rows, k], rel_hit)
    # ---- HitRecord::new
    mats, kinds = material_tables(S)
    hitm = best >= 0
    with np.errstate(all="ignore"):
        pnt = add(o, muls(d, tb))
    outward = (np.zeros(n, dt),) * 3
    hu, hv = np.zeros(n, dt), np.zeros(n, dt)
    ddir = d
    with np.errstate(all="ignore"):
        for q, pl in enumerate(S.planes):
            m = best == q
            if m.any():
                outward = where3(m, tuple(np.full(n, x, dt) for x in F.arr(pl["n"])), outward)
                u, v = plane_uv(F, pl, pnt)
                hu, hv = np.where(m, u, hu), np.where(m, v, hv)
        for q, Q in enumerate(S.quads):
            m = best == S.n_planes + q
            if m.any():
                outward = where3(m, tuple(np.full(n, x, dt) for x in F.arr(Q["n"])), outward)
                u, v = quad_uv(F, Q, sub(pnt, v3(F.arr(Q["q"]))))
                hu, hv = np.where(m, u, hu), np.where(m, v, hv)
        for q, B in enumerate(S.boxes):
            m = best == S.bbase + q
            if not m.any():
                continue
            t2, qd, o2, d2 = box_rec[q]
            po = add(o2, muls(d2, t2))
            pw = add(mat3_mul(F, B["rot"], po), v3(F.arr(B["t"])))
            pnt = where3(m, pw, pnt)
            ddir = where3(m, d2, ddir)
            for kq, Q in enumerate(B["quads"]):
                mq = m & (qd == kq)
                if mq.any():
                    outward = where3(mq, tuple(np.full(n, x, dt) for x in F.arr(Q["n"])), outward)
                    u, v = quad_uv(F, Q, sub(po, v3(F.arr(Q["q"]))))
                    hu, hv = np.where(mq, u, hu), np.where(mq, v, hv)
        m = best >= S.sbase
        if m.any():
            s = np.where(m, best - S.sbase, 0)
            cs = v3(F.arr(S.sph_c)[s])
            ow = F.divs(sub(pnt, cs), F.arr(S.sph_r)[s])
            outward = where3(m, ow, outward)
            rows = np.flatnonzero(m)
            u, v = sphere_uv(F, tuple(x[rows] for x in ow))
            hu[rows], hv[rows] = u, v
        dn = dot(ddir, outward)
        front = dn < 0
        nrm = where3(front, outward, neg(outward))
        facing = np.abs(dn) / np.sqrt(dot(ddir, ddir))
        gap = (second - tb) / tb
    z = np.zeros(n, dt)
    res = dict(id=best, t=np.where(hitm, tb, z), p=stack3(where3(hitm, pnt, (z, z, z))),
               normal=stack3(where3(hitm, nrm, (z, z, z))), outward=stack3(where3(hitm, outward, (z, z, z))),
               u=np.where(hitm, hu, z), v=np.where(hitm, hv, z),
               mat=np.where(hitm, mats[np.maximum(best, 0)], 0), front=np.where(hitm, front, False).astype(np.int64),
               kind=np.where(hitm, kinds[np.maximum(best, 0)], 0), gap=np.where(hitm, gap, F.inf), rel=rel_hit,
               near=near, edge=edge, facing=np.where(hitm, facing, F.inf))
    return res


# ------------------------------------------------------------------ light pdf
def one_minus_cos_max(F, x):
    """1 - sqrt(1 - x), x = r^2 / d^2: the f32 form x / (1 + sqrt(1 - x)) or the reference's"""
    with np.errstate(all="ignore"):
        if F.f32:
            return x * F.rcp(F.one + np.sqrt(F.one - x))
        return F.one - np.sqrt(F.one - x)


def sphere_pdf_value(F, c, r, o, d):
    """Sphere::pdf_value (rtw_device.hpp): sphere_t over [0, inf], then the solid angle"""
    with np.errstate(all="ignore"):
        hit, _, rel = sphere_roots(F, c, r * r, o, d, F.zero, "t")
        co = sub(c, o)
        dist2 = dot(co, co)
        if F.f32:
            pdf = F.rcp(F.tau * one_minus_cos_max(F, r * r * F.rcp(dist2)))
        else:
            cos_max = np.sqrt(F.one - r * r / dist2)
            pdf = F.one / ((F.two * F.pi) * (F.one - cos_max))
        return np.where(hit, pdf, F.zero), hit, rel


def light_hit_f32(F, c, r, o, d, robust):
    """light_pdf.hpp light_hit_f32 (pass 1): (hit, the decisions' margins): the normalised
    discriminant, and hb / (|d| |f|) and c / (f.f + r^2) for the side tests"""
    with np.errstate(all="ignore"):
        f = sub(o, c)
        a = d[2] * d[2] + (d[1] * d[1] + d[0] * d[0])
        ia = F.rcp(a)
        hb = d[2] * f[2] + (d[1] * f[1] + d[0] * f[0])
        r2 = r * r
        f2 = f[0] * f[0] + (f[1] * f[1] + f[2] * f[2])
        if robust:
            tc = -hb * ia
            l = add(muls(d, tc), f)
            l2 = l[0] * l[0] + (l[1] * l[1] + l[2] * l[2])
            rel = (r2 - l2) / (r2 + l2)
            inside = f2 <= r2
            hit = (l2 < r2) & ((hb <= 0) | inside)
            side = (r2 - f2) / (r2 + f2)
        else:
            cc = f[0] * f[0] + (f[1] * f[1] + (f[2] * f[2] - r2))
            disc = hb * hb - a * cc
            rel = disc / (hb * hb + np.abs(a * cc))
            hit = (disc > 0) & ((hb <= 0) | (cc <= 0))
            side = -cc / (f2 + r2)
        back = hb / np.sqrt(a * f2)
        # far from a decision: |rel| large, and (behind | inside) decided clearly
        margin = np.minimum(np.abs(rel), np.maximum(np.abs(back), np.abs(side)))
        return hit, margin


def light_pdf_f32(F, c, r, o):
    with np.errstate(all="ignore"):
        co = sub(c, o)
        dist2 = co[0] * co[0] + (co[1] * co[1] + co[2] * co[2])
        x = r * r * F.rcp(dist2)
        return F.rcp(F.tau * one_minus_cos_max(F, x))


def quad_pdf_value(F, Q, o, d, eps):
    with np.errstate(all="ignore"):
        hit, t, al, be = quad_t(F, Q, o, d, F.zero, F.inf, eps)
        n0 = v3(F.arr(Q["n"]))
        front = dot(d, n0) < 0
        n = where3(front, tuple(np.broadcast_to(x, front.shape) for x in n0),
                   tuple(np.broadcast_to(-x, front.shape) for x in n0))
        dist2 = t * t * dot(d, d)
        cosine = np.abs(F.div(dot(d, n), np.sqrt(dot(d, d))))
        pdf = F.div(dist2, cosine * F.dt(Q["area"]))
        e = np.minimum(np.minimum(np.abs(al), np.abs(F.one - al)), np.minimum(np.abs(be), np.abs(F.one - be)))
        return np.where(hit, pdf, F.zero), hit, e


def lights_pdf(S, rays, dtype, f32_form=True, robust=False, two_pass=None):
    """HittableList::pdf_value of the staged light list for rays [n, 6]
    (query_kernel.hpp light_pdf_rays_kernel): dict(pdf, hits [n, n_list] -- which
    entries counted --, margin [n, n_list] -- each entry's decision margin: the hit
    test's, and |1 - r^2 / d^2| for an origin on a light's surface).
    two_pass: the f32 kernels' linear / grid / light-BVH paths (light_hit_f32 then
    light_pdf_f32; default: the f32 form on a list of spheres only); otherwise
    the mixed path and every f64 path: each entry's own pdf_value, summed in list
    order.  The grid and the light BVH add the same terms in their walk's order."""
    F = Forms(dtype, f32_form)
    rays = F.arr(rays)
    n = len(rays)
    o, d = v3(rays[:, :3]), v3(rays[:, 3:])
    if two_pass is None:
        two_pass = f32_form and not S.mixed
    acc = np.zeros(n, F.dt)
    hits, margin = np.zeros((n, len(S.lref)), bool), np.full((n, len(S.lref)), np.inf, F.dt)
    eps = F.dt(S.eps)
    for k, (kind, idx) in enumerate(S.lref):
        if kind == "default":
            acc = acc + F.zero
            continue
        if kind == "quad":
            pdf, hit, e = quad_pdf_value(F, S.lquads[idx], o, d, eps)
            acc = acc + pdf
            hits[:, k], margin[:, k] = hit, e
            continue
        c, r = v3(F.arr(S.light_c[idx])), F.dt(S.light_r[idx])
        if two_pass:
            hit, mg = light_hit_f32(F, c, r, o, d, robust)
            acc = np.where(hit, acc + light_pdf_f32(F, c, r, o), acc)
        else:
            pdf, hit, mg = sphere_pdf_value(F, c, r, o, d)
            acc = acc + pdf
            mg = np.abs(mg)
        with np.errstate(all="ignore"):              # the origin on the light's surface: sqrt(1 - x) at x ~ 1
            co = sub(c, o)
            mg = np.fmin(mg, np.abs(F.one - r * r / dot(co, co)))
        hits[:, k], margin[:, k] = hit, mg
    nl = F.dt(S.n_list)
    with np.errstate(all="ignore"):
        pdf = F.div(acc, nl) * np.ones(n, F.dt)
        if S.leaf:
            pdf = F.div(pdf * nl, nl)
    return dict(pdf=pdf, hits=hits, margin=margin)


# ------------------------------------------------------------------- samplers
def unit_sphere(F, U, s, mask=None):
    """UnitSphere: the f32 form's inversion (three words) or the reference's rejection loop"""
    n = len(s)
    if F.f32:
        z = F.two * U.std(rng_next(s, mask)) - F.one
        az = U.std(rng_next(s, mask))
        u = U.std(rng_next(s, mask))
        # u^(1/3) as exp2(log2(u) / 3); u = 0 gives r = 0
        r = np.where(u > 0, F.lib(np.exp2, F.lib(np.log2, u) * F.dt(1.0 / 3.0)), F.zero)
        sn, cs = F.sincos_2pi(az)
        rxy = r * np.sqrt(np.fmax(F.one - z * z, F.zero))
        return (rxy * cs, rxy * sn, r * z)
    pend = np.ones(n, bool) if mask is None else mask.copy()
    out = [np.zeros(n), np.zeros(n), np.zeros(n)]
    while pend.any():
        p = tuple(2.0 * U.std(rng_next(s, pend)) - 1.0 for _ in range(3))
        ok = pend & (dot(p, p) < 1.0)
        for a in range(3):
            out[a] = np.where(ok, p[a], out[a])
        pend &= ~ok
    return tuple(out)


def unit_disk(F, U, s, mask=None):
    n = len(s)
    pend = np.ones(n, bool) if mask is None else mask.copy()
    ox, oz = np.zeros(n, F.dt), np.zeros(n, F.dt)
    while pend.any():
        x = F.two * U.std(rng_next(s, pend)) - F.one
        z = F.two * U.std(rng_next(s, pend)) - F.one
        ok = pend & (x * x + F.zero * F.zero + z * z < 1)
        ox, oz = np.where(ok, x, ox), np.where(ok, z, oz)
        pend &= ~ok
    return ox, oz


def cone_or_cosine(F, U, s, to_light, frame_n, c, r, o, mask=None):
    """mixture_direction (rtw_device.hpp): Sphere::random of the light {c, r} seen from o for
    the rows of to_light, CosinePdf::generate about frame_n for the others; two words each"""
    with np.errstate(all="ignore"):
        direction = sub(c, o)
        f = F.onb(where3(to_light, direction, frame_n))
        distance = np.sqrt(dot(direction, direction))
        if F.f32:
            q = r * r * F.rcp(distance * distance)
        else:
            q = (r * r) / (distance * distance)
        q = np.where(to_light, q, F.zero)
        r1 = U.std(rng_next(s, mask))
        r2 = U.std(rng_next(s, mask))
        sn, cs = F.sincos_2pi(np.where(to_light, r2, r1))
        t = np.sqrt(F.one - np.where(to_light, q, r2))
        if F.f32:
            w = r1 * (q * F.rcp(F.one + t))
            z = np.where(to_light, F.one - w, t)
            sxy = np.sqrt(np.where(to_light, w * (F.two - w), r2))
        else:
            z = np.where(to_light, F.one + r1 * (t - F.one), t)
            sxy = np.sqrt(np.where(to_light, F.one - z * z, r2))
        return F.onb_transform(f, (cs * sxy, sn * sxy, z))


def quad_random(F, U, Q, o, s, mask=None):
    r1 = U.open01(rng_next(s, mask))
    r2 = U.open01(rng_next(s, mask))
    p = add(add(v3(F.arr(Q["q"])), muls(v3(F.arr(Q["u"])), r1)), muls(v3(F.arr(Q["v"])), r2))
    return sub(p, o)


def lights_random(S, F, U, o, s, mask=None):
    """lights.random(o, rng): (direction, list index); one index draw, then the entry's random()"""
    n = len(s)
    mask = np.ones(n, bool) if mask is None else mask
    idx = rng_index(s, S.n_list, mask)
    out = (np.zeros(n, F.dt), np.zeros(n, F.dt), np.zeros(n, F.dt))
    sph = np.zeros(n, bool)
    for k, (kind, j) in enumerate(S.lref):
        m = mask & (idx == k)
        if not m.any():
            continue
        if kind == "quad":
            out = where3(m, quad_random(F, U, S.lquads[j], o, s, m), out)
        elif kind == "default":
            out = where3(m, (F.one, F.zero, F.zero), out)
        else:
            sph |= m
    if sph.any():
        j = np.array([jj if kind == "sphere" else 0 for kind, jj in S.lref], np.int64)[np.where(sph, idx, 0)]
        c = v3(F.arr(S.light_c)[j])
        r = F.arr(S.light_r)[j]
        dirs = cone_or_cosine(F, U, s, np.ones(n, bool), out, c, r, o, sph)
        out = where3(sph, dirs, out)
    return out, idx


def light_sample(S, origins, seed, first_stream, sample, dtype, f32_form=True, bits32=True, robust=False):
    """nee_kernel.hpp light_sample_kernel: dict(dir [n, 3], index, pdf, hits, margin)"""
    F = Forms(dtype, f32_form)
    U = Uniforms(F, bits32)
    o = v3(F.arr(origins))
    s = rng_seed(seed, np.arange(len(origins), dtype=np.uint64) + np.uint64(first_stream), sample)
    d, idx = lights_random(S, F, U, o, s)
    rays = np.concatenate([stack3(o), stack3(d)], 1)
    lp = lights_pdf(S, rays, dtype, f32_form, robust)
    return dict(dir=stack3(d), index=idx, state=s, **lp)


# ------------------------------------------------------------------- textures
def tex_colour(S, F, tid, u, v, p):
    """Texture::get_colour (render_kernel.hpp tex_colour): (rgb 3 arrays, the smallest distance of
    a checker argument from a cell edge, in cells)"""
    n = len(u)
    tid = tid.copy()
    out = [np.full(n, np.nan, F.dt) for _ in range(3)]
    done = np.zeros(n, bool)
    edge = np.full(n, np.inf, F.dt)
    for _ in range(64):
        kind = S.tex_type[tid]
        tp = F.arr(S.tex_p)[tid]
        solid = ~done & (kind == 0)
        for a in range(3):
            out[a] = np.where(solid, tp[:, a], out[a])
        done |= solid
        noise = ~done & (kind == 2)
        if noise.any():
            rows = np.flatnonzero(noise)
            x = _noise_value(S, F, S.tex_refs[tid[rows], 0], tp[rows, 3], tuple(c[rows] for c in p))
            for a in range(3):
                out[a][rows] = x
            done |= noise
        chk = ~done & (kind == 1)
        if not chk.any():
            break
        with np.errstate(all="ignore"):
            su, sv = u * tp[:, 3], v * tp[:, 3]
            sm = np.floor(su) + np.floor(sv)
            e = np.minimum(np.minimum(su - np.floor(su), np.floor(su) + F.one - su),
                           np.minimum(sv - np.floor(sv), np.floor(sv) + F.one - sv))
            even = np.fmod(sm, F.two) == 0
        edge = np.where(chk, np.fmin(edge, e), edge)
        tid = np.where(chk, np.where(even, S.tex_refs[tid, 0], S.tex_refs[tid, 1]), tid)
    return tuple(out), edge


def _perlin_index(x):
    with np.errstate(all="ignore"):
        return np.where(np.abs(x) < 2147483648.0, x.astype(np.int64) & 255, 0)


def _noise_value(S, F, table, scale, p):
    vec = F.arr(S.perlin_vec)
    perm = S.perlin_perm
    accum, weight = np.zeros(len(scale), F.dt), F.one
    t = p
    with np.errstate(all="ignore"):
        for _ in range(7):
            fl = tuple(np.floor(c) for c in t)
            u, v, w = (c - f for c, f in zip(t, fl))
            acc = np.full(len(scale), -0.0, F.dt)
            for di in range(2):
                px = perm[768 * table + _perlin_index(fl[0] + F.dt(di))]
                for dj in range(2):
                    py = perm[768 * table + 256 + _perlin_index(fl[1] + F.dt(dj))]
                    for dk in range(2):
                        c = vec[256 * table + (px ^ py ^ perm[768 * table + 512 + _perlin_index(fl[2] + F.dt(dk))])]
                        fi, fj, fk = F.dt(di), F.dt(dj), F.dt(dk)
                        wv = (u - fi, v - fj, w - fk)
                        term = (fi * u + (F.one - fi) * (F.one - u)) * (fj * v + (F.one - fj) * (F.one - v)) * \
                               (fk * w + (F.one - fk) * (F.one - w)) * dot(v3(c), wv)
                        acc = acc + term
            accum = accum + weight * acc
            t = muls(t, F.two)
            weight = weight * F.dt(0.5)
        arg = scale * p[2] + accum * F.dt(10)
        if F.f32:
            sn = F.lib(np.sin, arg)
        else:
            sn = np.array([_fdlibm_sin(float(a)) for a in arg], np.float64)
        return F.dt(0.5) * (sn + F.one)


# ----------------------------------------------------------------- the bounce
def shade(S, rays, hits, ids, rng, dtype, f32_form=True, bits32=True, robust=False):
    """One iteration of ray_colour_tail_call after world.hit (path_kernel.hpp
    shade_rays_kernel) on given records: dict(next [n, 6], weight, emitted [n, 3],
    event, pdfs [n, 3], state [n, 4] -- the words after the draws --, what [n],
    margin [n]: the margin of the row's own discrete decision (Metal: dir . n of the
    kept test; Dielectric: |ratio sin - 1| and |reflectance - u|; textures: the
    distance to a checker edge), light_hits / light_margin as lights_pdf)."""
    F = Forms(dtype, f32_form)
    U = Uniforms(F, bits32)
    dt = F.dt
    rays, hits = F.arr(rays), F.arr(hits)
    ids = np.asarray(ids, np.int64)
    n = len(rays)
    s = np.array(rng, np.uint64).reshape(n, 4).copy()
    hit = (ids[:, 0] >= 0) & (ids[:, 1] >= 0) & (ids[:, 1] < len(S.mat_type))
    m = np.where(hit, ids[:, 1], 0)
    zero_state = hit & ((s[:, 0] | s[:, 1] | s[:, 2] | s[:, 3]) == 0)
    if zero_state.any():
        s[zero_state] = rng_seed(0, np.zeros(int(zero_state.sum()), np.uint64), 0)
    front = ids[:, 2] != 0
    d = v3(rays[:, 3:])
    pnt, nrm = v3(hits[:, 1:4]), v3(hits[:, 4:7])
    mtype = np.where(hit, S.mat_type[m], INVISIBLE)
    mp = F.arr(S.mat_p)[m]
    z = np.zeros(n, dt)
    colour = v3(mp)
    margin = np.full(n, np.inf, dt)
    if S.mat_tex is not None:
        tex = hit & ((mtype == DIFFUSE_LIGHT) | (mtype == LAMBERTIAN))
        if tex.any():
            rows = np.flatnonzero(tex)
            col, edge = tex_colour(S, F, S.mat_tex[m[rows]], hits[rows, 7], hits[rows, 8], tuple(c[rows] for c in pnt))
            colour = tuple(c.copy() for c in colour)
            for a in range(3):
                colour[a][rows] = col[a]
            margin[rows] = edge
    emitted = where3(mtype == DIFFUSE_LIGHT, colour, (z, z, z))
    event = np.where(hit, ABSORBED, MISS)
    what = np.where(hit, np.where(mtype == DIFFUSE_LIGHT, "diffuse light", "invisible"), "miss").astype("U32")
    dirn, weight = (z, z, z), (z, z, z)
    pdfs = np.zeros((n, 3), dt)
    with np.errstate(all="ignore"):
        metal = mtype == METAL
        if metal.any():
            refl = F.reflect(F.normalize(d), nrm)
            us = unit_sphere(F, U, s, metal)
            dm = add(refl, muls(us, mp[:, 3]))
            dn = dot(dm, nrm)
            keep = dn > 0
            margin = np.where(metal, np.abs(dn) / np.sqrt(dot(dm, dm)), margin)
            dirn = where3(metal & keep, dm, dirn)
            weight = where3(metal & keep, v3(mp), weight)
            event = np.where(metal & keep, REFLECT, event)
            what = np.where(metal, np.where(keep, "metal", "metal absorbed"), what)
        diel = mtype == DIELECTRIC
        if diel.any():
            ratio = np.where(front, F.div(F.one, mp[:, 3]), mp[:, 3])
            unit = F.normalize(d)
            cos_t = np.fmin(dot(unit, neg(nrm)), F.one)
            sin_t = np.sqrt(F.one - cos_t * cos_t)
            cannot = ratio * sin_t > 1
            r0 = F.div(F.one - ratio, F.one + ratio)
            r0 = r0 * r0
            x = F.one - cos_t
            refl_p = r0 + (F.one - r0) * (x * ((x * x) * (x * x)))
            draw = U.open01(rng_next(s, diel & ~cannot))
            schlick = ~cannot & (refl_p > draw)
            dd = where3(cannot | schlick, F.reflect(unit, nrm), F.refract(unit, nrm, ratio))
            mg = np.where(cannot, np.abs(ratio * sin_t - F.one),
                          np.minimum(np.abs(ratio * sin_t - F.one), np.abs(refl_p - draw)))
            margin = np.where(diel, mg, margin)
            dirn = where3(diel, dd, dirn)
            weight = where3(diel, (F.one + z, F.one + z, F.one + z), weight)
            event = np.where(diel, REFLECT, event)
            what = np.where(diel, np.where(cannot, "total internal reflection",
                                           np.where(schlick, "schlick reflection", "refraction")), what)
        lamb = mtype == LAMBERTIAN
        light_hits = light_margin = None
        if lamb.any():
            to_light = lamb & (U.std(rng_next(s, lamb)) < 0.5)
            idx = rng_index(s, S.n_list, to_light)
            dl = (z, z, z)
            sph = np.zeros(n, bool)
            kind_of = np.array([k for k, _ in S.lref])
            for k, (kind, j) in enumerate(S.lref):
                mk = to_light & (idx == k)
                if not mk.any():
                    continue
                if kind == "quad":
                    dl = where3(mk, quad_random(F, U, S.lquads[j], pnt, s, mk), dl)
                    what = np.where(mk, "light quad", what)
                elif kind == "default":
                    dl = where3(mk, (F.one + z, z, z), dl)
                    what = np.where(mk, "light default", what)
                else:
                    sph |= mk
            rest = lamb & (~to_light | sph)
            jj = np.array([j if kind == "sphere" else 0 for kind, j in S.lref], np.int64)[np.where(sph, idx, 0)]
            if len(S.light_c):
                c, r = v3(F.arr(S.light_c)[jj]), F.arr(S.light_r)[jj]
            else:
                c, r = (z, z, z), z
            c, r = where3(sph, c, (z, z, z)), np.where(sph, r, z)
            dmix = cone_or_cosine(F, U, s, sph, nrm, c, r, pnt, rest)
            dl = where3(rest, dmix, dl)
            what = np.where(sph, "light sphere", np.where(lamb & ~to_light, "cosine lobe", what))
            rows = np.flatnonzero(lamb)
            lr = np.concatenate([stack3(pnt), stack3(dl)], 1)[rows]
            lp = lights_pdf(S, lr, dtype, f32_form, robust)
            lpdf = np.zeros(n, dt)
            lpdf[rows] = lp["pdf"]
            light_hits = np.zeros((n, len(S.lref)), bool)
            light_margin = np.full((n, len(S.lref)), np.inf, dt)
            light_hits[rows], light_margin[rows] = lp["hits"], lp["margin"]
            ndir, wn = F.normalize(dl), F.normalize(nrm)
            cos_w = F.over_pi(dot(ndir, wn))
            pdf = lpdf * dt(0.5) + np.fmax(cos_w, F.zero) * dt(0.5)
            spdf = np.fmax(F.over_pi(dot(nrm, ndir)), F.zero)
            wl = F.divs(muls(colour, spdf), pdf)
            dirn, weight = where3(lamb, dl, dirn), where3(lamb, wl, weight)
            pdfs = np.where(lamb[:, None], np.stack([pdf, lpdf, spdf], 1), pdfs)
            event = np.where(lamb, SCATTER, event)
    goes_on = event >= REFLECT
    nxt = np.concatenate([stack3(where3(goes_on, pnt, (z, z, z))), stack3(dirn)], 1)
    return dict(next=nxt, weight=stack3(weight), emitted=stack3(emitted), event=event.astype(np.int32), pdfs=pdfs,
                state=s, what=what, margin=margin, light_hits=light_hits, light_margin=light_margin)


# --------------------------------------------------------------------- camera
def camera_rays(cam, seed, pixels, sample, dtype, f32_form=True, bits32=True, store=np.float32):
    """Camera::get_ray (path_kernel.hpp camera_rays_kernel): (rays [n, 6], states [n, 4]).
    cam: a dict of the camera's f64 fields (oracle.camera_dict); they reach the kernel
    rounded to `store` (host/camera_params.hpp), and so they do here."""
    F = Forms(dtype, f32_form)
    U = Uniforms(F, bits32)
    g = lambda name: v3(F.arr(_rnd(cam[name], store)))   # noqa: E731
    W = int(cam["image_width"])
    pixels = np.asarray(pixels, np.int64)
    s = rng_seed(seed, pixels.astype(np.uint64), sample)
    scale = RS.uniform_inclusive_scale(-0.5, 0.5)
    ox = U.incl(rng_next(s), -0.5, scale)
    oy = U.incl(rng_next(s), -0.5, scale)
    i, j = (pixels % W).astype(F.dt), (pixels // W).astype(F.dt)
    ps = add(add(g("pixel00_loc"), muls(g("pixel_delta_u"), i + ox)), muls(g("pixel_delta_v"), j + oy))
    origin = tuple(np.broadcast_to(c, i.shape) for c in g("center"))
    if cam["defocus_angle"] > EPS:
        qx, qz = unit_disk(F, U, s)
        origin = add(add(g("center"), muls(g("defocus_disk_u"), qx)), muls(g("defocus_disk_v"), qz))
    return np.concatenate([stack3(origin), stack3(sub(ps, origin))], 1), s
