// render_kernel.hpp -- the gfx950 render kernels, templated on precision R
// and on the world query (brute force over an LDS-staged or a global sphere
// list; BVH).
//
// Restates the reference's per-pixel / per-sample loop:
//   render_internal / render_lambda   shared/src/camera.rs:315-388
//   Camera::get_ray                   shared/src/camera.rs:274-293
//   ray_colour_tail_call              shared/src/camera.rs:459-522
// as ONE iterative loop per lane.  Work is cut into ITEMS = (pixel, chunk of
// `chunk` consecutive samples); a wavefront owns a TASK = one 8x8 tile x a
// group of chunks, i.e. a pool of 64 * group items.  Every lane takes an item,
// traces its samples one segment (one world.hit) per loop trip, folds them in
// sample order into the item's partial sum, and when the item is done takes
// the next free item of the pool (ballot + mbcnt: no atomics).  All lanes thus
// share every trip's closest-hit sweep even though the reference's path
// lengths range from 1 to max_depth segments (its t_min = f64::EPSILON makes
// self-intersecting, depth-long paths common).
//
// Chunk sums land in partial[tile][pixel][chunk]; reduce_chunks_kernel folds
// them in chunk order.  Inside a chunk the samples are folded exactly like
// `(0..spp).map(..).fold(Colour::default(), +)` (camera.rs:323-335), so with
// chunk >= spp the f64 result is the reference's fold order bit for bit.
//
// This file: the primitives of the kernel body (planes, boxes, the brute-force
// sweeps), the f64 hit points of the f32 kernels, textures, and the three
// kernels.  The BVH closest hit is in bvh_traverse.hpp, the light pdf in
// light_pdf.hpp, the host-side launch in render_launch.hpp.
#pragma once

#include <type_traits>

#include "bvh_traverse.hpp"
#include "light_pdf.hpp"
#include "rtw_device.hpp"
#include "rtw_kernels.h"

namespace rtw {

namespace dev {

template <typename R>
__device__ __forceinline__ V3<R> v3of(const R* a) { return mk(a[0], a[1], a[2]); }

// Plane::get_plane_uv, plane.rs:40-54, on the host-computed per-plane
// constants of the record (rtw_kernels.h kPlaneR): the oracle's plane_uv.
template <typename R>
__device__ __forceinline__ void plane_uv(const R* pl, V3<R> pnt, R& u, R& v) {
    const R mode = pl[12];
    if (mode == (R)0) {
        u = pnt.x;
        v = pnt.z;
        return;
    }
    if (mode == (R)2) {
        u = v = (R)NAN;
        return;
    }
    const V3<R> k = q3(pl, 15);
    const V3<R> vec = pnt - q3(pl, 0);
    const R ct = pl[13], st = pl[14];
    const V3<R> rot = ((vec * ct) + cross(k, vec) * st) + (k * dot(k, vec)) * ((R)1 - ct);
    u = rot.x - trunc_(rot.x);
    v = rot.z - trunc_(rot.z);
}

// One plane, plane.rs:61-76 (one-sided: only rays moving along +n hit it).
// Plane::hit computes the UV before its range test and panics on a
// non-finite one (plane.rs:66-69): counted in *panic (a rare event: one
// atomic at the site, no register kept live).  The UV is not formed
// here: it is NaN for every point of a mode-2 plane, (x, z) for mode 0, and a
// rotation of the finite constants for mode 1 -- non-finite exactly when the
// point is (up to overflow inside the rotation itself, |p| ~ 1e308).
template <typename R, typename PP>
__device__ __forceinline__ bool plane_t(PP pl, V3<R> o, V3<R> d, R tmin, R& t,
                                        unsigned long long* panic) {
    V3<R> n = mk(pl[3], pl[4], pl[5]);
    R denom = dot(d, n);
    if (!(denom > P<R>::kEps)) return false;
    V3<R> op = o - mk(pl[0], pl[1], pl[2]);
    R tt = -P<R>::div_(dot(op, n), denom);
    {
        const V3<R> q = o + d * tt;
        const R mode = pl[12];
        const bool fin = mode == (R)0 ? __builtin_isfinite(q.x) && __builtin_isfinite(q.z)
                                      : mode == (R)1 && __builtin_isfinite(q.x + q.y + q.z);
        if (!fin && panic) atomicAdd(panic, 1ull);
    }
    if (!(tmin <= tt && tt <= (R)INFINITY)) return false;
    t = tt;
    return true;
}

// AABBox::hit, hittable.rs:291-339, over [rs, +inf]: the slab test the
// reference runs before every object's own hit (bounded_hit).  Rust's f64
// max/min ignore a NaN operand like fmax/fmin.
template <typename R, typename PP>
__device__ __forceinline__ bool aabb_hit_ref(PP lo, PP hi, V3<R> o, V3<R> d, R rs) {
    R t0 = P<R>::div_(lo[0] - o.x, d.x), t1 = P<R>::div_(hi[0] - o.x, d.x);
    if (__builtin_signbit(d.x)) { R q = t0; t0 = t1; t1 = q; }
    R tmin = t0, tmax = t1;
    R a0 = P<R>::div_(lo[1] - o.y, d.y), a1 = P<R>::div_(hi[1] - o.y, d.y);
    if (__builtin_signbit(d.y)) { R q = a0; a0 = a1; a1 = q; }
    if (tmax < a0 || tmin > a1) return false;
    tmin = P<R>::max_(tmin, a0);
    tmax = P<R>::min_(tmax, a1);
    a0 = P<R>::div_(lo[2] - o.z, d.z);
    a1 = P<R>::div_(hi[2] - o.z, d.z);
    if (__builtin_signbit(d.z)) { R q = a0; a0 = a1; a1 = q; }
    if (tmax < a0 || tmin > a1) return false;
    tmin = P<R>::max_(tmin, a0);
    tmax = P<R>::min_(tmax, a1);
    return P<R>::max_(rs, tmin) <= P<R>::min_((R)INFINITY, tmax);
}

// aabb_hit_ref on a plane's box (Plane::get_aabbox, plane.rs:218-242: every
// axis pinned at [0, 0] or [-inf, inf]) for a finite ray: an infinite axis
// always yields (-inf, +inf) after the sign swap, which no later max_ / min_
// or comparison changes, so the test reduces to the one pinned axis, q = (0 -
// o_a) / d_a, and hits iff !(q < rs) -- the same quotient and the same
// outcome (NaN included) as the six-division reference sequence (f64: IEEE
// division; f32: a * rcp(b), whose infinities for a zero d_a or an infinite
// a follow the same signs).  Anything else (a non-finite ray, other boxes)
// takes aabb_hit_ref itself.
template <typename R, typename PP>
__device__ __forceinline__ bool aabb_hit_plane(PP lo, PP hi, V3<R> o, V3<R> d, R rs) {
    const bool fin = __builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z) &&
                     __builtin_isfinite(d.x) && __builtin_isfinite(d.y) && __builtin_isfinite(d.z);
    int npin = 0, pin = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (lo[a] == (R)0 && hi[a] == (R)0 && !__builtin_signbit(lo[a])) {
            ++npin;
            pin = a;
        } else if (!(lo[a] == (R)-INFINITY && hi[a] == (R)INFINITY)) {
            npin = 4;
        }
    }
    if (!fin || npin > 1) return aabb_hit_ref(lo, hi, o, d, rs);
    if (npin == 0) return true;
    const R oa = pin == 0 ? o.x : (pin == 1 ? o.y : o.z);
    const R da = pin == 0 ? d.x : (pin == 1 ? d.y : d.z);
    const R q = P<R>::div_(lo[pin] - oa, da);
    return !(q < rs);
}

// Transformed<Cuboid>::hit (entities/transformations.rs:14-29, cuboid.rs:50-58)
// on the staged record B (rtw_kernels.h kBoxR), as the oracle's box_hit: the
// ray into object space through the inverse (the direction ALSO gets the
// translation, geometry/src/transformations.rs:112-114 -- the reference's
// behaviour), the closest of the six quads (first minimum wins).
template <typename R>
__device__ __forceinline__ V3<R> mat3_mul(const R* M, V3<R> p) {   // Mul<Vec3> for Matrix3
    return mk(dot(q3(M, 0), p), dot(q3(M, 3), p), dot(q3(M, 6), p));
}
template <typename R>
__device__ __forceinline__ bool box_t_hit(const R* B, V3<R> o, V3<R> d, R tmin, R tmax, R& t, int& quad,
                                          V3<R>& o2, V3<R>& d2) {
    if (B[kBoxOk] == (R)0) return false;
    o2 = mat3_mul(B + kBoxInv, o) + q3(B, kBoxTi);
    d2 = mat3_mul(B + kBoxInv, d) + q3(B, kBoxTi);
    int best = -1;
    R bt = (R)INFINITY;
    for (int k = 0; k < 6; ++k) {
        R tt;
        if (quad_t_hit(B + kQuadR * k, o2, d2, tmin, tmax, tt) && (best < 0 || tt < bt)) {
            bt = tt;
            best = k;
        }
    }
    if (best < 0) return false;
    t = bt;
    quad = best;
    return true;
}

// Closest sphere of a contiguous list [0, n), ids base + k.  Semantics of the
// reference's closest hit: t = near root if it lies in [tmin, inf], else the
// far root (sphere.rs:71-80); the smallest t wins, the lowest id on ties.
//
// f64 (parity mode): the reference's exact arithmetic, divisions included.
template <bool kRobust>
__device__ __forceinline__ void sweep_spheres(const R4<double>* __restrict__ sph, uint32_t n,
                                              int32_t base, V3<double> o, V3<double> d, double tmin,
                                              double& tb, int32_t& best) {
#pragma unroll 2
    for (uint32_t k = 0; k < n; ++k) {
        const R4<double> s = sph[k];
        double t;
        if (sphere_t(mk(s.x, s.y, s.z), s.w, o, d, tmin, t) && (best < 0 || t < tb)) {
            tb = t;
            best = base + (int32_t)k;
        }
    }
}
// f32 (speed mode): the per-sphere test is sphere_u (bvh_traverse.hpp).
// Branch-free body so that the compiler keeps a batch of sphere loads in flight.
template <bool kRobust>
__device__ __forceinline__ void sweep_spheres(const R4<float>* __restrict__ sph, uint32_t n,
                                              int32_t base, V3<float> o, V3<float> d, float tmin,
                                              float& tb, int32_t& best) {
    const float a = len2_f32(d);
    const float ia = __builtin_amdgcn_rcpf(a);
    const uint32_t tminb = __float_as_uint(tmin);
    uint32_t ub = __float_as_uint(tb) - tminb;
#pragma unroll 8
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t u = sphere_u<kRobust>(sph[k], o, d, a, ia, tminb);
        const bool h = u < ub;
        ub = h ? u : ub;
        best = h ? base + (int32_t)k : best;
    }
    tb = __uint_as_float(ub + tminb);
}

// The same with one sphere id excluded (kOptHit64: the sphere the ray starts on)
template <bool kRobust>
__device__ __forceinline__ void sweep_spheres_excl(const R4<float>* __restrict__ sph, uint32_t n, int32_t base,
                                                   V3<float> o, V3<float> d, float tmin, float& tb, int32_t& best,
                                                   int32_t excl) {
    const float a = len2_f32(d);
    const float ia = __builtin_amdgcn_rcpf(a);
    const uint32_t tminb = __float_as_uint(tmin);
    uint32_t ub = __float_as_uint(tb) - tminb;
#pragma unroll 8
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t u = sphere_u<kRobust>(sph[k], o, d, a, ia, tminb);
        const bool h = u < ub && base + (int32_t)k != excl;
        ub = h ? u : ub;
        best = h ? base + (int32_t)k : best;
    }
    tb = __uint_as_float(ub + tminb);
}

// ---------------------------------------------------------------------------
// f64 hit points for the f32 kernels (kOptHit64).  The reference's t_min =
// f64::EPSILON (camera.rs:473) makes the bounce after a hit re-hit its own
// sphere ("acne") exactly when the rounded f64 hit point r.at(t) lies inside
// it -- a coin flip decided by f64 rounding that shapes the image (paths
// trapped inside spheres, NaN samples from Lambertian points inside light
// spheres).  f32 arithmetic flips that coin with other odds, so the f32 image
// drifts from the reference's region by region.  With kOptHit64 the f32
// kernel keeps the ray origin in f64 and computes, in f64 with the
// reference's operation order and no FMA contraction: the re-hit test of the
// sphere the ray starts on, the t of the sphere the f32 traversal picked, and
// the hit point o + d t.  Traversal, shading and sampling stay f32.
// ---------------------------------------------------------------------------
// Sphere::hit's roots, sphere.rs:61-80, with t in [EPSILON, inf] (f64, no FMA)
// on the sphere as given (DevScene::sph64: {c, radius})
__device__ __forceinline__ bool sphere_t_ref64(const R4<double>& S, V3<double> o, V3<double> d, double& t) {
#pragma clang fp contract(off)
    const double ocx = o.x - S.x, ocy = o.y - S.y, ocz = o.z - S.z, r = S.w;
    const double a = d.x * d.x + d.y * d.y + d.z * d.z;
    const double half_b = ocx * d.x + ocy * d.y + ocz * d.z;
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - r * r;
    const double disc = half_b * half_b - a * c;
    if (!(disc > 0.0)) return false;
    const double sq = __builtin_sqrt(disc);
    double root = (-half_b - sq) / a;
    if (!(P<double>::kEps <= root && root <= (double)INFINITY)) {
        root = (-half_b + sq) / a;
        if (!(P<double>::kEps <= root && root <= (double)INFINITY)) return false;
    }
    t = root;
    return true;
}
// Plane::hit's t, plane.rs:64: -((o - p) . n) / (d . n) (f64, no FMA), on the
// plane as given (DevScene::pl64: {point, 0}, {normal, 0})
__device__ __forceinline__ double plane_t_ref64(const R4<double>* P, V3<double> o, V3<double> d) {
#pragma clang fp contract(off)
    const R4<double> pt = P[0], n = P[1];
    const double denom = d.x * n.x + d.y * n.y + d.z * n.z;
    return -(((o.x - pt.x) * n.x + (o.y - pt.y) * n.y + (o.z - pt.z) * n.z) / denom);
}
// Ray::at, o + d t (f64, no FMA)
__device__ __forceinline__ V3<double> ray_at64(V3<double> o, V3<double> d, double t) {
#pragma clang fp contract(off)
    return V3<double>{o.x + d.x * t, o.y + d.y * t, o.z + d.z * t};
}
__device__ __forceinline__ V3<double> to64(V3<float> v) { return V3<double>{v.x, v.y, v.z}; }
__device__ __forceinline__ V3<double> to64(V3<double> v) { return v; }
// An f32 direction as a GENERIC f64 value: the f32 value with pseudo-random
// bits below its 24-bit mantissa (a relative change < 2^-25: the same f32
// value).  The reference's directions are f64 results with rounding noise in
// every bit; a 24-bit value makes d.d exact and the products of d.(o - c)
// nearly so, which changes the odds of the ulp-level decisions above (the
// re-hit of a perfect mirror from inside, measured: tools/trace_paths.py).
// The bits come from a hash of the f32 bits (no RNG draw).
__device__ __forceinline__ uint32_t mix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ V3<double> dither64(V3<float> v) {
    RTW_PROBE_ABL_DITHER(v);
    const uint32_t h0 = mix32(__float_as_uint(v.x) ^ mix32(__float_as_uint(v.y) ^ mix32(__float_as_uint(v.z))));
    const uint32_t h1 = mix32(h0 + 0x9e3779b9u), h2 = mix32(h1 + 0x9e3779b9u);
    constexpr double kScale = 0x1p-25 / 4294967296.0;        // (h - 2^31) * 2^-57: |rel| < 2^-26
    return V3<double>{(double)v.x * (1.0 + ((double)h0 - 2147483648.0) * kScale),
                      (double)v.y * (1.0 + ((double)h1 - 2147483648.0) * kScale),
                      (double)v.z * (1.0 + ((double)h2 - 2147483648.0) * kScale)};
}

__device__ __forceinline__ V3<double> dither64(V3<double> v) { return v; }   // (R = double: unused)
template <typename R>
__device__ __forceinline__ V3<R> from64(V3<double> v) { return mk((R)v.x, (R)v.y, (R)v.z); }

// Vec3::normalize, self / self.length() (vec.rs), in f64, no FMA: the unit
// incoming direction both Metal and Dialectric start from (material.rs:414, 469)
__device__ __forceinline__ V3<double> unit64(V3<double> d) {
#pragma clang fp contract(off)
    const double l = __builtin_sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
    return div3(d.x, d.y, d.z, l);
}
// Metal::scatter's direction (material.rs:407-421) in f64, no FMA, from the
// unit direction u: reflect(u, n) + us * fuzz, with reflect(v, n) = v - (n * 2)
// (v . n) (vec.rs); its dot with n decides absorption (returned in `keep`)
__device__ __forceinline__ V3<double> metal_dir64(V3<double> u, V3<double> n, double fuzz, V3<double> us,
                                                  bool& keep) {
#pragma clang fp contract(off)
    const double ux = u.x, uy = u.y, uz = u.z;
    const double vn = ux * n.x + uy * n.y + uz * n.z;
    const double rx = ux - (n.x * 2.0) * vn, ry = uy - (n.y * 2.0) * vn, rz = uz - (n.z * 2.0) * vn;
    const V3<double> out = {rx + us.x * fuzz, ry + us.y * fuzz, rz + us.z * fuzz};
    keep = out.x * n.x + out.y * n.y + out.z * n.z > 0.0;
    return out;
}
// Dialectric::scatter's direction (material.rs:458-487) in f64, no FMA, from
// the unit direction u and the material's f64 record M = {1/ior, r0 at 1/ior,
// r0 at ior, ior} (DevScene::mat64: the recip() and reflectance's r0 =
// ((1 - ratio) / (1 + ratio))^2 of both faces, computed once on the host with
// the same operations); the Open01 word is drawn only when refraction is
// possible (the || short circuit)
__device__ __forceinline__ V3<double> dielectric_dir64(V3<double> u, V3<double> n, bool front,
                                                       const R4<double>& M, Rng& g) {
#pragma clang fp contract(off)
    const double ratio = front ? M.x : M.w;
    const double ux = u.x, uy = u.y, uz = u.z;
    const double cos_t = __builtin_fmin(ux * -n.x + uy * -n.y + uz * -n.z, 1.0);
    const double sin_t = __builtin_sqrt(1.0 - cos_t * cos_t);
    bool refl = ratio * sin_t > 1.0;
    if (!refl) {
        const double r0 = front ? M.y : M.z;             // Dialectric::reflectance, powi(5) as LLVM expands it
        const double x = 1.0 - cos_t, x2 = x * x;
        refl = r0 + (1.0 - r0) * (x * (x2 * x2)) > P<double>::u_open01(g.next());
    }
    if (refl) {
        const double vn = ux * n.x + uy * n.y + uz * n.z;
        return V3<double>{ux - (n.x * 2.0) * vn, uy - (n.y * 2.0) * vn, uz - (n.z * 2.0) * vn};
    }
    // refract(v, n, eta), vec.rs: perp = (v + n cos) eta, par = n * -sqrt(1 - perp.perp)
    const double c2 = __builtin_fmin(ux * -n.x + uy * -n.y + uz * -n.z, 1.0);
    const double px = (ux + n.x * c2) * ratio, py = (uy + n.y * c2) * ratio, pz = (uz + n.z * c2) * ratio;
    const double q = -__builtin_sqrt(1.0 - (px * px + py * py + pz * pz));
    return V3<double>{px + n.x * q, py + n.y * q, pz + n.z * q};
}
// Metal::scatter and Dialectric::scatter for an f64 sphere hit (kOptHit64)
// in one pass: both start from the unit incoming direction u, its dot with
// the normal and the mirror direction (vec.rs reflect); Metal perturbs it by
// fuzz * UnitSphere (drawn first, as in the separate path), Dialectric keeps
// it on total internal reflection or a Schlick draw and refracts otherwise.
// The lanes of a wave that hit either material run it together.  Per lane
// the draws and operations are metal_dir64's / dielectric_dir64's:
// Dialectric's cos_theta = min(u . -n, 1) is min(-(u . n), 1) bit for bit
// (negation is exact and round-to-nearest symmetric).
// `kRefSphere`: Metal's UnitSphere by the reference's rejection loop in f64
// (the f64 parity kernels), else the f32 kernels' direct sampler carried into
// f64 (dither64).
template <bool kRefSphere = false>
__device__ __forceinline__ V3<double> specular_dir64(bool metal, V3<double> d, V3<double> n, bool front,
                                                     const R4<double>& M, Rng& g, bool& keep) {
#pragma clang fp contract(off)
    V3<double> us = {0.0, 0.0, 0.0};
    if (metal) {
        if constexpr (kRefSphere) us = unit_sphere<double>(g);
        else us = dither64(unit_sphere<float>(g));
    }
    const V3<double> u = unit64(d);
    const double vn = u.x * n.x + u.y * n.y + u.z * n.z;
    const V3<double> r = {u.x - (n.x * 2.0) * vn, u.y - (n.y * 2.0) * vn, u.z - (n.z * 2.0) * vn};
    keep = true;
    if (metal) {
        const double fuzz = M.w;
        const V3<double> out = {r.x + us.x * fuzz, r.y + us.y * fuzz, r.z + us.z * fuzz};
        keep = out.x * n.x + out.y * n.y + out.z * n.z > 0.0;
        return out;
    }
    const double ratio = front ? M.x : M.w;
    const double cos_t = __builtin_fmin(-vn, 1.0);
    const double sin_t = __builtin_sqrt(1.0 - cos_t * cos_t);
    bool refl = ratio * sin_t > 1.0;
    if (!refl) {
        const double r0 = front ? M.y : M.z;   // Dialectric::reflectance, powi(5) as LLVM expands it
        const double x = 1.0 - cos_t, x2 = x * x;
        refl = r0 + (1.0 - r0) * (x * (x2 * x2)) > P<double>::u_open01(g.next());
    }
    if (refl) return r;
    // refract(v, n, eta), vec.rs: perp = (v + n cos) eta, par = n * -sqrt(1 - perp.perp)
    const double px = (u.x + n.x * cos_t) * ratio, py = (u.y + n.y * cos_t) * ratio, pz = (u.z + n.z * cos_t) * ratio;
    const double q = -__builtin_sqrt(1.0 - (px * px + py * py + pz * pz));
    return V3<double>{px + n.x * q, py + n.y * q, pz + n.z * q};
}
// the outward normal (p - c) / radius, sphere.rs:82-83 (f64, no FMA)
__device__ __forceinline__ V3<double> sphere_normal64(V3<double> p, const R4<double>& S) {
#pragma clang fp contract(off)
    return div3(p.x - S.x, p.y - S.y, p.z - S.z, S.w);
}
__device__ __forceinline__ bool front64(V3<double> d, V3<double> n) {
#pragma clang fp contract(off)
    return d.x * n.x + d.y * n.y + d.z * n.z < 0.0;
}

// ---------------------------------------------------------------------------
// Textures (kOptTex kernels): Texture::get_colour, texture.rs:15-102
// ---------------------------------------------------------------------------
__device__ __forceinline__ double fmod_(double a, double b) { return ::fmod(a, b); }
__device__ __forceinline__ float fmod_(float a, float b) { return ::fmodf(a, b); }

// Perlin::noise (perlin.rs:59-82) + perlin_interpolation (:96-108): the
// oracle's rtwo_perlin_noise, term for term (iproduct order, Sum from -0.0)
template <typename R>
__device__ __forceinline__ R perlin_noise(const R4<R>* __restrict__ vec, const uint32_t* __restrict__ perm,
                                          V3<R> p) {
    const R u = p.x - floor_(p.x), v = p.y - floor_(p.y), w = p.z - floor_(p.z);
    const R i = floor_(p.x), j = floor_(p.y), k = floor_(p.z);
    R acc = (R)-0.0;
#pragma unroll
    for (int di = 0; di < 2; ++di) {
        const uint32_t px = perm[perlin_index(i + (R)di)];
#pragma unroll
        for (int dj = 0; dj < 2; ++dj) {
            const uint32_t py = perm[256 + perlin_index(j + (R)dj)];
#pragma unroll
            for (int dk = 0; dk < 2; ++dk) {
                const R4<R> c = vec[px ^ py ^ perm[512 + perlin_index(k + (R)dk)]];
                const R fi = (R)di, fj = (R)dj, fk = (R)dk;
                const V3<R> wv = mk(u - fi, v - fj, w - fk);
                const R term = (fi * u + ((R)1 - fi) * ((R)1 - u)) * (fj * v + ((R)1 - fj) * ((R)1 - v)) *
                               (fk * w + ((R)1 - fk) * ((R)1 - w)) * dot(mk(c.x, c.y, c.z), wv);
                acc = acc + term;
            }
        }
    }
    return acc;
}

// CheckerTexture (nested textures followed iteratively), NoiseTexture
// (0.5 (1 + sin(scale z + 10 turb(p, 7)))), SolidColour
template <typename R>
__device__ V3<R> tex_colour(const DevScene<R>& sc, uint32_t tid, R u, R v, V3<R> p) {
    for (int depth = 0; depth < 64; ++depth) {
        const uint32_t kind = sc.tex_type[tid];
        const R4<R> tp = sc.tex_p[tid];
        if (kind == 1u) {
            const R s = floor_(u * tp.w) + floor_(v * tp.w);
            tid = fmod_(s, (R)2) == (R)0 ? sc.tex_refs[2 * tid] : sc.tex_refs[2 * tid + 1];
            continue;
        }
        if (kind == 2u) {
            const uint32_t q = sc.tex_refs[2 * tid];
            const R4<R>* vec = sc.perlin_vec + 256 * q;
            const uint32_t* perm = sc.perlin_perm + 768 * q;
            R accum = (R)0, weight = (R)1;        // Perlin::turb, perlin.rs:84-94
            V3<R> t = p;
            for (int o = 0; o < 7; ++o) {
                accum = accum + weight * perlin_noise(vec, perm, t);
                t = t * (R)2;
                weight = weight * (R)0.5;
            }
            const R x = rt_sin(tp.w * p.z + accum * (R)10) + (R)1;
            return mk((R)0.5 * x, (R)0.5 * x, (R)0.5 * x);
        }
        return mk(tp.x, tp.y, tp.z);
    }
    return mk((R)NAN, (R)NAN, (R)NAN);
}


// (kOpt: the kOpt* bits of rtw_kernels.h, chosen per render by host/render_plan.cpp)
// the kernels with wide workgroups (rtw_kernels.h kernel_wide)
template <typename R, int kWorld, int kOpt>
constexpr bool kernel_wide() {
    return kernel_wide(sizeof(R), kWorld, kOpt);
}
template <typename R, int kWorld, int kOpt>
constexpr uint32_t kernel_waves() { return block_waves(kernel_wide<R, kWorld, kOpt>()); }
// the waves per SIMD render_kernel asks for (its second __launch_bounds__
// argument; the RTW_WAVES* knobs of rtw_kernels.h).  f64 kernels with quads /
// cuboids / textures keep the compiler's choice.
template <typename R, int kOpt>
constexpr int kernel_occupancy() {
    constexpr bool kLbvh = (kOpt & kOptLightBvh) != 0;
    if (sizeof(R) == 4) return (kOpt & kOptHit64) ? (kLbvh ? RTW_WAVES_H64_LBVH : RTW_WAVES_H64) : RTW_WAVES;
    if (kOpt & (kOptPrims | kOptTex)) return 1;
    return kLbvh ? RTW_WAVES_F64_LBVH : RTW_WAVES_F64;
}
// ray_colour_tail_call's accumulator `res` (camera.rs:459-522): res += mult *
// emitted at every scatter, added to the sample's colour where it ends.
// Kernels for scenes without a DiffuseLight (kEmit false; the host routes a
// scene with one to the kOptPrims kernels) know emitted() = (0, 0, 0) on every
// hit (material.rs:42-44): res starts at +0 and gains mult * (+0), which is
// +0 or -0 -- no change, +0 + -0 = +0 -- while mult is finite and NaN once it
// is not, and then stays NaN.  So res is +0 or NaN per component: three bits
// instead of three registers, and value() is exactly res.
template <typename R, bool kEmit>
struct ResAcc;
template <typename R>
struct ResAcc<R, true> {
    V3<R> v;
    __device__ __forceinline__ void reset() { v = mk<R>(0, 0, 0); }
    __device__ __forceinline__ void add(V3<R> mult, V3<R> emitted) { v = v + mult * emitted; }
    __device__ __forceinline__ V3<R> value() const { return v; }
};
template <typename R>
struct ResAcc<R, false> {
    uint32_t nan;
    __device__ __forceinline__ void reset() { nan = 0; }
    __device__ __forceinline__ void add(V3<R> mult, V3<R>) {   // emitted is (0, 0, 0) here
        nan |= (__builtin_isfinite(mult.x) ? 0u : 1u) | (__builtin_isfinite(mult.y) ? 0u : 2u) |
               (__builtin_isfinite(mult.z) ? 0u : 4u);
    }
    __device__ __forceinline__ V3<R> value() const {
        return mk<R>((nan & 1u) ? (R)NAN : (R)0, (nan & 2u) ? (R)NAN : (R)0, (nan & 4u) ? (R)NAN : (R)0);
    }
};

template <typename R, int kWorld, int kOpt>
__global__ void __launch_bounds__((64 * kernel_waves<R, kWorld, kOpt>()), (kernel_occupancy<R, kOpt>()))
    render_kernel(const KParams<R> p) {
    using PR = P<R>;
    constexpr uint32_t kWB = kernel_waves<R, kWorld, kOpt>();   // waves per workgroup
    constexpr uint32_t kBlk = 64 * kWB;
    constexpr bool kRobust = (kOpt & kOptRobust) != 0;
    constexpr bool kLightBvh = (kOpt & kOptLightBvh) != 0 && kWorld >= kWorldBvh;
    constexpr bool kTex = (kOpt & kOptTex) != 0;
    constexpr bool kPrims = (kOpt & kOptPrims) != 0;
    constexpr bool kHit64 = (kOpt & kOptHit64) != 0 && sizeof(R) == 4 && !kTex && !kPrims;
    // DiffuseLight materials only in the kOptPrims / kOptTex kernels (the host
    // routes scenes with one there): the others know emitted() is black
    constexpr bool kEmit = kPrims || kTex;
    extern __shared__ __attribute__((aligned(32))) unsigned char smem[];
    R4<R>* s_sph = reinterpret_cast<R4<R>*>(smem);
    R4<R>* s_li = s_sph + p.sc.n_sph;
    if constexpr (kWorld == kWorldLds) {
        // Stage the sphere list {c, r^2} and the light list into LDS once per
        // workgroup: every lane of every wave then reads sphere k at the same
        // LDS address (a broadcast read) during its closest-hit sweep.
        for (uint32_t k = threadIdx.x; k < p.sc.n_sph; k += kBlk) s_sph[k] = p.sc.sph[k];
        for (uint32_t k = threadIdx.x; k < p.sc.n_lights; k += kBlk) s_li[k] = p.sc.lights[k];
        __syncthreads();
    }
    const R4<R>* __restrict__ sph = kWorld == kWorldLds ? s_sph : p.sc.sph;
    const R4<R>* __restrict__ li = kWorld == kWorldLds ? s_li : p.sc.lights;
    R4<R>* l_li = nullptr;   // kWorldBvhLds: the light list in LDS
    R4<R>* l_lp = nullptr;   // kWorldBvhLds, f32: the light list as pairs in LDS
    R4<float>* l_li32 = nullptr;   // kWorldBvhLds, f64: the lights rounded to f32 (light pre-pass)
    R4<R>* l_bsph64 = nullptr;     // kWorldBvhLds, f64, wide workgroups: the f64 leaf spheres
    R4<R>* l_sph64 = nullptr;      // ... and the f64 spheres in id order
    // World view of the closest-hit query.  kWorldBvhLds: the BVH nodes and
    // the leaf-ordered spheres + ids are copied into LDS once per workgroup
    // (after the traversal stacks), so traversal fetches go to the LDS
    // instead of the vector-memory (TA/L1) path the shading loads use.
    DevScene<R> scw = p.sc;
    if constexpr (kWorld == kWorldBvhLds) {
        unsigned char* base = smem + traversal_lds<R>(p.stack, kLightBvh, kWB);
        // the f32 tree (bvh32) in both precisions: the while-while traversal culls on it
        BvhNode<float>* l_nodes = reinterpret_cast<BvhNode<float>*>(base);
        // the leaf spheres {c, r^2} in f32 (f64: the pre-pass copy bsph32; the
        // f64 candidates are read from the global leaf array)
        R4<float>* l_bsph = reinterpret_cast<R4<float>*>(l_nodes + p.sc.n_nodes);
        uint32_t* l_bid = reinterpret_cast<uint32_t*>(l_bsph + p.sc.n_sph);
        static_assert(sizeof(BvhNode<float>) % 16 == 0, "nodes are copied in 16-B units");
        const uint4* g_nodes = reinterpret_cast<const uint4*>(cull_nodes(p.sc));
        constexpr uint32_t kNode16 = sizeof(BvhNode<float>) / 16;
        for (uint32_t k = threadIdx.x; k < p.sc.n_nodes * kNode16; k += kBlk)
            reinterpret_cast<uint4*>(l_nodes)[k] = g_nodes[k];
        const R4<float>* g_bsph32;
        if constexpr (sizeof(R) == 4) g_bsph32 = p.sc.bsph;
        else g_bsph32 = p.sc.bsph32;
        for (uint32_t k = threadIdx.x; k < p.sc.n_sph; k += kBlk) {
            l_bsph[k] = g_bsph32[k];
            l_bid[k] = p.sc.bid[k];
        }
        // the light list follows, aligned to its element (read by the light pdf / sampling)
        // (offsets from smem, not integer casts of pointers: a pointer rebuilt from an
        // integer loses its LDS address space, and every access through it became a
        // flat instruction -- which waits on the vector-memory counter as well)
        auto lds_after = [&](const void* end, size_t align) {
            const size_t off = (size_t)(reinterpret_cast<const unsigned char*>(end) - smem);
            return smem + ((off + align - 1) & ~(align - 1));
        };
        l_li = reinterpret_cast<R4<R>*>(lds_after(l_bid + ((p.sc.n_sph + 7u) & ~7u), sizeof(R4<R>)));
        for (uint32_t k = threadIdx.x; k < p.sc.n_lights; k += kBlk) l_li[k] = p.sc.lights[k];
        if constexpr (sizeof(R) == 4) {
            // and again as pairs for the packed light test (lights_pdf_sum_pk)
            l_lp = l_li + p.sc.n_lights;
            const uint32_t n = p.sc.n_lights;
            for (uint32_t q = threadIdx.x; 2 * q < n; q += kBlk) {
                const R4<R> A = p.sc.lights[2 * q];
                const bool odd = 2 * q + 1 < n;
                const R4<R> B = odd ? p.sc.lights[2 * q + 1] : R4<R>{0, 0, 0, 0};
                l_lp[2 * q] = R4<R>{A.x, B.x, A.y, B.y};
                l_lp[2 * q + 1] = R4<R>{A.z, B.z, A.w * A.w, odd ? B.w * B.w : (R)-INFINITY};
            }
        } else {
            // the lights rounded to f32 with |radius| (the f32 pre-pass of lights_pdf_sum;
            // a packed-FP32 pre-pass over light pairs measured 1.4 ms slower: r04)
            l_li32 = reinterpret_cast<R4<float>*>(l_li + p.sc.n_lights);
            for (uint32_t k = threadIdx.x; k < p.sc.n_lights; k += kBlk) {
                const R4<R> L = p.sc.lights[k];
                l_li32[k] = R4<float>{(float)L.x, (float)L.y, (float)L.z, fabsf((float)L.w)};
            }
            if constexpr (kernel_wide<R, kWorld, kOpt>()) {
                // wide workgroups: the f64 leaf spheres too, 32-B aligned (the leaf
                // loop's candidates, test_leaf: an LDS read instead of L1 / L2)
                l_bsph64 = reinterpret_cast<R4<R>*>(lds_after(l_li32 + p.sc.n_lights, 32));
                for (uint32_t k = threadIdx.x; k < p.sc.n_sph; k += kBlk) l_bsph64[k] = p.sc.bsph[k];
                // and in id order (the own-sphere test at the traversal's start)
                l_sph64 = l_bsph64 + p.sc.n_sph;
                for (uint32_t k = threadIdx.x; k < p.sc.n_sph; k += kBlk) l_sph64[k] = p.sc.sph[k];
            }
        }
        __syncthreads();
        if constexpr (sizeof(R) == 4) {
            scw.bvh = l_nodes;
            scw.bsph = l_bsph;
        } else {
            scw.bvh32 = l_nodes;
            scw.bsph32 = l_bsph;
            if constexpr (kernel_wide<R, kWorld, kOpt>()) {
                scw.bsph = l_bsph64;
                scw.sph = l_sph64;
            }
        }
        scw.bid = l_bid;
    }
    if constexpr (kWorld == kWorldBvhLds) li = l_li;

    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // subtree stealing (while-while kernels): this wave's result slots and
    // rendezvous bytes, after the workgroup's traversal stacks.
    // Only for trees held in LDS: on large trees (C3, C5 from L2 / MALL) the
    // subtrees idle lanes take early are mostly culled later by the owner's
    // closest hit (C5: 9.6 -> 18.4 node visits per segment), and the steady
    // state loses more than the lanes gain (C3 852 -> 875 ms, C5 1536 -> 1751)
    constexpr bool kSteal = kWorld == kWorldBvhLds;
    unsigned char* const steal_area =
        smem + (size_t)kWB * p.stack * 64 * sizeof(int32_t) + wave * kStealLdsPerWave<R>;
    // the light BVH / grid kernels: the wave's light-work counters (u64 light
    // tests, grid cells), right after the traversal area
    unsigned long long* const wcnt =
        reinterpret_cast<unsigned long long*>(smem + traversal_lds<R>(p.stack, false, kWB) + wave * kLightWorkBytes);
    if constexpr (kLightBvh) {
        if (lane < 2) wcnt[lane] = 0ull;
    }
    // the wave's current task (wave-uniform): local tile lt = global 8x8 tile
    // T = lt * nranks + rank at (tx, ty) -- the ranks take the image's tiles
    // round-robin (rtw_tiles_for_rank) -- and chunks [c_begin, c_begin +
    // glen): a pool of 64 glen (pixel, chunk) items.  Chunk indices are absolute:
    // a sample window's start at c_base (KParams::c_base, added once per task), so
    // a lane's c and s = c * chunk + ... are the render's own chunk and sample
    // indices and a sample's start costs a window nothing
    uint32_t lt = 0, tx = 0, ty = 0, c_begin = 0, glen = 0;
    uint32_t glen_m = 0;          // glen > 1: ceil(2^32 / glen), q / glen = umulhi(q, glen_m) for q < 64 glen
                                  // (2^32 does not fit: glen == 1 is special-cased)
    // The camera, the background and the task parameters are read where they
    // are used (once per sample, miss or task), from the kernarg segment
    // through an opaque pointer: held in SGPRs across the loop they overflow
    // the SGPR file, and the compiler parks them in VGPR lanes and reads them
    // back with v_readlane -- a VALU instruction each, every segment.
    typedef const KParams<R> __attribute__((address_space(4))) KArgs;
    auto kargs = []() {
        const KArgs* k = (const KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(k));   // not loop-invariant for the compiler: loaded at each use
        return k;
    };
    // The scene record for a callee, read from the kernel arguments at the call
    // (the fields it uses, by scalar loads) instead of from `p`, whose fields the
    // compiler hoists into SGPRs held across the whole loop -- the light pdf's
    // walks overflow the SGPR file into VGPR lanes and scratch.  (The host pass
    // only type-checks the kernel body: there it is a reference to `p.sc`.)
#if defined(__HIP_DEVICE_COMPILE__)
#define RTW_KARG_SCENE(name) const DevScene<R> name = kargs()->sc
#else
#define RTW_KARG_SCENE(name) const DevScene<R>& name = p.sc
#endif

    auto set_task = [&](uint32_t t) {
        const KArgs* k = kargs();
        if (k->task_table) {   // longest tiles first, cut by cost
            lt = k->task_table[2 * t];
            const uint32_t e = k->task_table[2 * t + 1];
            c_begin = (e & 0xFFFFFu) + k->c_base;
            glen = e >> 20;
        } else {
            lt = t / k->n_groups;
            const uint32_t cg = t - lt * k->n_groups;
            c_begin = cg * k->group;
            glen = min(c_begin + k->group, k->n_chunks) - c_begin;
            c_begin += k->c_base;
        }
        const uint32_t T = k->tile_map ? k->tile_map[lt] : lt * k->nranks + k->rank;   // (global_tile)
        ty = T / k->tiles_x;
        tx = T - ty * k->tiles_x;
        glen_m = glen > 1 ? (uint32_t)((0xFFFFFFFFull + glen) / glen) : 0u;
    };
    // p.persist: every wave takes tasks from a global counter until none are
    // left, and its lanes move on to the next task's items while others still
    // finish the last one -- no per-task drain, one workgroup setup (LDS
    // staging) per resident workgroup.  Else one task per wave (static map).
    bool more = p.persist != 0;       // wave-uniform: the counter may hold tasks
    if (!p.persist) {
        const uint32_t task = blockIdx.x * kWB + wave;
        if (task >= p.n_tasks) return;
        set_task(task);
    }
    // item q -> (pixel px, chunk c): pixel-major (p.item_order 0: q = chunk
    // offset * 64 + px -- the 64 lanes start on the tile's 64 pixels) or
    // sample-major (1: q = px * glen + chunk offset -- the lanes start on a
    // few pixels' consecutive samples: coherent primary rays and first hits).
    // Every item is still one (pixel, chunk) folded in order by the reduce
    // kernel, so the image does not depend on it.
    auto decode = [&](uint32_t qq, uint32_t& px_out, uint32_t& c_out) {
        if (p.item_order) {
            px_out = glen > 1 ? __umulhi(qq, glen_m) : qq;   // qq / glen: exact, qq < 64 glen <= 2^18
            c_out = c_begin + (qq - px_out * glen);
        } else {
            px_out = qq & 63u;
            c_out = c_begin + (qq >> 6);
        }
    };

    const V3<R> zero = mk<R>(0, 0, 0);
    const R tmin = PR::kEps;
    const int32_t nplanes = (int32_t)p.sc.n_planes;
    const int32_t nquads = (int32_t)p.sc.n_quads;
    const int32_t bbase = nplanes + nquads;                  // object ids: planes, quads,
    const int32_t sbase = bbase + (int32_t)p.sc.n_boxes;     // boxes, spheres

    // per-lane item state
    uint32_t q = lane;            // item index in the task's pool
    uint32_t next_q = 0;          // wave-uniform: first unassigned item
    // (kept small: it is live across the whole segment loop) the pixel (i, j)
    // as i | j << 16 (W, H < 2^16, checked by the host), the item's chunk-sum
    // slot lt * 64 + px (its local tile lt = slot >> 6), its chunk c and the
    // current sample s; the chunk's samples end at min((c + 1) chunk, spp)
    uint32_t ij = 0, slot = 0, c = 0, s = 0;
    auto pix_now = [&]() { return (uint64_t)(ij >> 16) * p.W + (ij & 0xffffu); };   // pixel index
    (void)pix_now;                // (probe builds)
    Rng g;
    V3<R> o = zero, d = zero, mult = zero;
    ResAcc<R, kEmit> res;
    res.reset();
    uint32_t depth = 0;
    int32_t self_s = -1;          // isolated sphere the current ray starts on (else -1); kHit64:
                                  // the sphere it starts on, isolated or not
    bool self_iso = false;        // kHit64: self_s is isolated
    V3<double> o64 = {0.0, 0.0, 0.0};   // kHit64: the ray origin in f64
    V3<double> d64 = {0.0, 0.0, 0.0};   // kHit64: the ray direction in f64 (a Metal / Dielectric
                                        // scatter's own f64 result, else dither64 of the f32 one)
    // segments and Lambertian bounces are counted per wave (scalar: a ballot's
    // popcount per trip), node visits and sphere tests per lane (the tile costs)
    uint32_t segs = 0, lambs = 0, nvis = 0, ntest = 0;
    // (counting renders with KParams::cost_time) the clock at the last trip's
    // start and its lanes
    uint64_t trip_clk = 0;
    uint32_t trip_lanes = 0;
    bool active = false, need = true;
    // kCoopGrid (f32 kernels with the light grid, KParams::grid_piece > 0): a
    // Lambertian bounce's light pdf is left pending (`pend`) for the wave's
    // cooperative grid walk at the end of the trip (lights_pdf_grid_coop); the
    // bounce's att * scattering pdf and half its cosine pdf wait with it
    constexpr bool kCoopGrid = kLightBvh && !kPrims;
    RTW_PROBE_WAVE_BEGIN();
    RTW_PROBE_CLK_INIT();
    RTW_PROBE_HIT_INIT();

    auto start_sample = [&]() {
        const KArgs* k = kargs();
        // tile costs (KParams::tile_cost): the sample's work is the lane's counters at
        // its end minus at its start -- subtracted here, added at the end (a
        // u32 sum: exact modulo 2^32, no register kept)
        if (k->tile_cost) {
            if (s < k->cost_spp && !k->cost_time) atomicSub(k->tile_cost + (slot >> 6), nvis + ntest);
        }
        // Camera::get_ray, camera.rs:274-293 + ray_colour_call, camera.rs:439-457
        const uint32_t i = ij & 0xffffu, j = ij >> 16;
        g.seed(k->seed, (uint64_t)j * k->W + i, s);
        R ox = PR::u_incl(g.next(), (R)-0.5, k->u_scale);
        R oy = PR::u_incl(g.next(), (R)-0.5, k->u_scale);
        V3<R> ps = (mk(k->p00[0], k->p00[1], k->p00[2]) + mk(k->du[0], k->du[1], k->du[2]) * ((R)i + ox)) +
                   mk(k->dv[0], k->dv[1], k->dv[2]) * ((R)j + oy);
        const V3<R> center = mk(k->center[0], k->center[1], k->center[2]);
        V3<R> origin = center;
        if (k->defocus) {
            V3<R> qd = unit_disk<R>(g);
            origin = (center + mk(k->disk_u[0], k->disk_u[1], k->disk_u[2]) * qd.x) +
                     mk(k->disk_v[0], k->disk_v[1], k->disk_v[2]) * qd.z;
        }
        o = origin;
        d = ps - origin;
        if constexpr (kHit64) {
            o64 = to64(origin);
            d64 = dither64(d);
        }
        mult = mk<R>(1, 1, 1);
        res.reset();
        RTW_PROBE_HIT_RESET();
        depth = k->max_depth;
        self_s = -1;
        self_iso = false;
    };
    // (wave-uniform) the end of the items this wave may hand out: its task's 64 glen
    uint32_t claim_end = p.persist ? 0u : 64u * glen;
    // Give every lane that needs one a valid item: from the current pool, then
    // (p.persist) from the next task's; none once no task is left.
    auto acquire = [&]() {
        const KArgs* k = kargs();
        for (;;) {
            const uint64_t want = __ballot(need);
            if (want == 0) break;
            if (next_q >= claim_end) {
                uint32_t t = 0xffffffffu;
                if (more) {
                    const uint64_t live = __ballot(true);
                    const uint32_t leader = (uint32_t)__builtin_ctzll(live);
                    if (lane == leader) t = (uint32_t)atomicAdd(k->counters + 6, 1ull);
                    t = (uint32_t)__shfl((int)t, (int)leader);
                }
                if (t >= k->n_tasks) {   // every task is taken: these lanes are done
                    RTW_PROBE_WAVE_DRY();
                    more = false;
                    need = false;
                    break;
                }
                set_task(t);
                RTW_PROBE_WAVE_TASK();
                next_q = 0;
                claim_end = 64u * glen;
                continue;
            }
            if (need) {
                const uint32_t below = __builtin_amdgcn_mbcnt_hi(
                    (uint32_t)(want >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)want, 0u));
                q = next_q + below;
                if (q < claim_end) {
                    uint32_t px;
                    decode(q, px, c);
                    const uint32_t i = tx * kTile + (px & 7u), j = ty * kTile + (px >> 3);
                    if (i < k->W && j < k->H) {
                        ij = i | (j << 16);
                        slot = lt * 64u + px;
                        s = c * k->chunk;
                        active = true;
                        need = false;
                        start_sample();
                    }
                }
            }
            next_q += (uint32_t)__popcll(want);
        }
    };
    // the first 64 items of the first task go to lanes 0..63 in order
    acquire();
    RTW_PROBE_CLK(0);
    // Issue priority in rotation.  A SIMD's arbiter favours its oldest wave:
    // with persistent waves, whose ages never change, the wave in slot 0 ran
    // at 1.46x and the one in slot 3 at 0.53x the mean rate (lane-segments per
    // us, profiles/r06c_timeline.jsonl), and the launch ended on slot-3 waves
    // finishing a task taken long before (an 8-rank C2 share: 1 ms after the
    // median wave).  Each wave takes priority (clock / 2^RTW_PRIO_SHIFT + its
    // slot) mod 4 at every trip, so at any time the waves of a SIMD hold
    // different priorities and each holds the highest a quarter of the time.
    uint32_t prio_slot;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(prio_slot));
    prio_slot &= 3u;

    for (;;) {
        const uint64_t live = __ballot(active);
        if (live == 0) break;
        if (kargs()->cost_time) {
            // wave-time tile costs (counting renders): the last trip's clock cycles,
            // shared by its lanes, added for each lane running a counted sample now
            // (a trip lasts about as long as the one before it)
            const KArgs* k = kargs();
            const uint64_t now = clock64();
            if (trip_lanes && active && s < k->cost_spp)
                atomicAdd(k->tile_cost + (slot >> 6), (uint32_t)(now - trip_clk) / trip_lanes);
            trip_clk = now;
            trip_lanes = (uint32_t)__popcll(live);
        }
        {
            const uint32_t pr = ((uint32_t)(wall_clock64() >> RTW_PRIO_SHIFT) + prio_slot) & 3u;
            if (pr == 0) __builtin_amdgcn_s_setprio(0);
            else if (pr == 1) __builtin_amdgcn_s_setprio(1);
            else if (pr == 2) __builtin_amdgcn_s_setprio(2);
            else __builtin_amdgcn_s_setprio(3);
        }
        segs += (uint32_t)__popcll(live);   // every active lane runs one segment of this trip
        RTW_PROBE_WAVE_TRIP();
        bool lamb = false;                  // the lane's segment ended in a Lambertian scatter
        // (kCoopGrid) this trip's pending light pdf and the bounce's weights: set by
        // the Lambertian branch, consumed by the walk at the end of the same trip --
        // declared per trip, so the compiler does not carry them across trips
        bool pend = false;
        V3<R> pend_aw = zero;
        R pend_ch = (R)0;
        RTW_PROBE_CLK(12);
        RTW_PROBE_LANES(3);
        if (active) {
            RTW_PROBE_LANES(4);
            if constexpr (kHit64) {
                // the f32 ray is the f64 one rounded (dither64 stays within half an
                // f32 ulp): o, d are not kept live across segments
                o = from64<R>(o64);
                d = from64<R>(d64);
            }
            // ---- world.hit(&r, EPSILON..=INFINITY): closest over all primitives
            R tb = (R)INFINITY;
            int32_t best = -1;
            double tb64 = 0.0;            // kHit64: the closest hit's t in f64
            RTW_PROBE_PLANES();
            for (int32_t k = 0; k < nplanes; ++k) {
                R t;
                // f32 kernels: the plane record through a constant-address-space
                // pointer -- its address is wave-uniform, so these are scalar loads
                // (SGPR operands, the scalar cache) instead of a vector load per field
                // whose latency started every segment (hit64 86.2 -> 85.7 ms, plain
                // 58.0 -> 57.5, C3 f32 -1 %; profiles/r06pl_ab.jsonl).  The f64 kernels
                // keep vector loads: the f64 record's SGPRs spilled (C2 f64 +0.3 %).
                typedef const R __attribute__((address_space(4))) KR;
                using PlanePtr = typename std::conditional<sizeof(R) == 4, KR*, const R*>::type;
                PlanePtr pl = (PlanePtr)kargs()->sc.planes + kPlaneR * k;
                // plane_t's one-sided test (plane.rs:62-63) first: it fails for every
                // ray that leaves the Book-1 ground downwards, and then the box test
                // (side-effect free, bounded_hit's first half) cannot change the outcome
                if (!(dot(d, mk(pl[3], pl[4], pl[5])) > PR::kEps)) continue;
                const bool box_hit = aabb_hit_plane(pl + 6, pl + 9, o, d, tmin);
                if (box_hit && plane_t(pl, o, d, tmin, t, p.counters + 4) &&
                    (best < 0 || t < tb)) {
                    tb = t;
                    best = k;
                }
            }
            // quads, each behind its own AABB (bounded_hit, hittable.rs:190-196)
            for (int32_t k = 0; kPrims && k < nquads; ++k) {
                R t;
                const R* Q = kargs()->sc.quads + kQuadR * k;
                if (aabb_hit_ref(Q + 16, Q + 19, o, d, tmin) && quad_t_hit(Q, o, d, tmin, (R)INFINITY, t) &&
                    (best < 0 || t < tb)) {
                    tb = t;
                    best = nplanes + k;
                }
            }
            // transformed cuboids, each behind its world AABB
            for (int32_t k = 0; kPrims && k < (int32_t)kargs()->sc.n_boxes; ++k) {
                R t;
                int qd;
                V3<R> o2, d2;
                const R* B = kargs()->sc.boxes + kBoxR * k;
                if (aabb_hit_ref(B + kBoxLo, B + kBoxHi, o, d, tmin) &&
                    box_t_hit(B, o, d, tmin, (R)INFINITY, t, qd, o2, d2) && (best < 0 || t < tb)) {
                    tb = t;
                    best = bbase + k;
                }
            }
            RTW_PROBE_CLK(1);
            if constexpr (kHit64) {
                // the own sphere's re-hit in f64, the others in f32 (it excluded), the
                // winner's t again in f64
                tb64 = best >= 0 ? (double)tb : (double)INFINITY;
                bool skip = false;
                if (self_s >= 0) {
                    RTW_PROBE_LANES(5);
                    ++ntest;
                    double ts;
                    bool self_hit = sphere_t_ref64(kargs()->sc.sph64[self_s], o64, d64, ts) && ts < tb64;
                    RTW_PROBE_ABL_SELF(self_hit, ts);
                    if (self_hit) {
                        tb64 = ts;
                        tb = (float)ts;
                        best = sbase + self_s;
                        skip = self_iso;          // isolated: provably the closest sphere hit
                    }
                }
                if constexpr (kSteal) {
                    // every active lane calls the traversal: the skipped ones steal work
                    RTW_PROBE_LANES(6);
                    const int32_t prev = best, excl = self_s >= 0 ? sbase + self_s : -1;
                    int32_t* stk_wave = reinterpret_cast<int32_t*>(smem) + wave * p.stack * 64;
                    bvh_closest_excl_steal<kRobust>(scw, sbase, o, d, tmin, tb, best, stk_wave, lane, steal_area,
                                                    nvis, ntest, excl, skip);
                    if (!skip && best != prev && best >= sbase) {
                        if (!sphere_t_ref64(kargs()->sc.sph64[best - sbase], o64, d64, tb64)) tb64 = (double)tb;
                        RTW_PROBE_ABL_WINNER();
                    }
                } else if (!skip) {   // (kernels without stealing)
                    RTW_PROBE_LANES(6);
                    const int32_t prev = best, excl = self_s >= 0 ? sbase + self_s : -1;
                    if constexpr (kWorld >= kWorldBvh) {
                        int32_t* stk = reinterpret_cast<int32_t*>(smem) + wave * p.stack * 64 + lane;
                        constexpr int kKind = kWorld == kWorldBvhLds ? kWorldBvhWW : kWorld;
                        bvh_closest_excl<kKind, kRobust>(scw, sbase, o, d, tmin, tb, best, stk, nvis, ntest, excl);
                    } else {
                        sweep_spheres_excl<kRobust>(sph, kargs()->sc.n_sph, sbase, o, d, tmin, tb, best, excl);
                    }
                    if (best != prev && best >= sbase) {
                        if (!sphere_t_ref64(kargs()->sc.sph64[best - sbase], o64, d64, tb64)) tb64 = (double)tb;
                        RTW_PROBE_ABL_WINNER();
                    }
                }
                // a plane's t in f64 too, so that its hit points lie within f64 rounding
                // of the plane (the one-sided Book-1 ground is never hit from above)
                if (best >= 0 && best < nplanes) tb64 = plane_t_ref64(kargs()->sc.pl64 + 2 * best, o64, d64);
                RTW_PROBE_H64();
            } else if constexpr (kWorld >= kWorldBvh) {
                RTW_PROBE_CLOSEST();
                int32_t* stk = reinterpret_cast<int32_t*>(smem) + wave * p.stack * 64 + lane;
                constexpr int kKind = kWorld == kWorldBvhLds ? kWorldBvhWW : kWorld;
                if constexpr (kSteal) {
                    bvh_closest_steal<kRobust>(scw, sbase, o, d, tmin, tb, best, stk - lane, lane, steal_area,
                                               nvis, ntest, self_s);
                } else {
                    bvh_closest<kKind, kRobust>(scw, sbase, o, d, tmin, tb, best, stk, nvis, ntest, self_s);
                }
            } else {
                sweep_spheres<kRobust>(sph, kargs()->sc.n_sph, sbase, o, d, tmin, tb, best);
            }
            RTW_PROBE_CLK(2);
            RTW_PROBE_SEGMENT();
            RTW_PROBE_HIT(best);

            bool done = false;
            V3<R> col = zero;
            if (best < 0) {
                const KArgs* k = kargs();
                col = mult * mk(k->bg[0], k->bg[1], k->bg[2]) + res.value();   // camera.rs:473-475
                done = true;
            } else {
                // HitRecord::new, hittable.rs:101-129
                V3<R> pnt = o + d * tb;
                V3<double> pnt64 = {0.0, 0.0, 0.0};
                if constexpr (kHit64) {
                    pnt64 = ray_at64(o64, d64, tb64);
                    pnt = mk((float)pnt64.x, (float)pnt64.y, (float)pnt64.z);
                }
                V3<R> outward;
                uint32_t m, mtype;
                R4<R> mp;
                int32_t next_self = -1;
                bool next_iso = false;
                V3<double> n64 = {0.0, 0.0, 0.0};   // kHit64, sphere hits: the f64 outward normal
                bool sph_hit = false;
                bool box_hit = false;
                bool box_front = false;
                R hu = (R)0, hv = (R)0;                            // HitRecord u, v (kTex)
                if (kPrims && best >= bbase && best < sbase) {
                    // Transformed<Cuboid>: the record of the object-space hit,
                    // its point mapped back (transform_point3d); the normal and
                    // front face stay in object space (transformations.rs:14-29)
                    const R* B = kargs()->sc.boxes + kBoxR * (best - bbase);
                    R t2;
                    int qd = 0;
                    V3<R> o2, d2;
                    box_t_hit(B, o, d, tmin, (R)INFINITY, t2, qd, o2, d2);
                    const V3<R> n = q3(B + kQuadR * qd, 12);
                    box_front = dot(d2, n) < (R)0;
                    outward = n;
                    const V3<R> po = o2 + d2 * t2;
                    pnt = mat3_mul(B + kBoxRot, po) + q3(B, kBoxT);
                    m = kargs()->sc.box_mat[best - bbase];
                    mtype = kargs()->sc.mat_type[m];
                    mp = kargs()->sc.mat_p[m];
                    box_hit = true;
                    if constexpr (kTex) {                          // get_quad_uv, object space
                        const R* Q = B + kQuadR * qd;
                        const V3<R> pq = po - q3(Q, 0);
                        hu = dot(cross(pq, q3(Q, 6)), q3(Q, 9));
                        hv = dot(cross(q3(Q, 3), pq), q3(Q, 9));
                    }
                } else if (best < nplanes) {
                    const R* pl = kargs()->sc.planes + kPlaneR * best;
                    outward = mk(pl[3], pl[4], pl[5]);
                    m = kargs()->sc.plane_mat[best];
                    mtype = kargs()->sc.mat_type[m];
                    mp = kargs()->sc.mat_p[m];
                    if constexpr (kTex) plane_uv(pl, pnt, hu, hv);
                } else if (kPrims && best < bbase) {
                    const R* Q = kargs()->sc.quads + kQuadR * (best - nplanes);
                    outward = q3(Q, 12);                           // quadrilateral.rs:97
                    m = kargs()->sc.quad_mat[best - nplanes];
                    mtype = kargs()->sc.mat_type[m];
                    mp = kargs()->sc.mat_p[m];
                    if constexpr (kTex) {                          // get_quad_uv, quadrilateral.rs:58-63
                        const V3<R> pq = pnt - q3(Q, 0);
                        hu = dot(cross(pq, q3(Q, 6)), q3(Q, 9));
                        hv = dot(cross(q3(Q, 3), pq), q3(Q, 9));
                    }
                } else {
                    const uint32_t k = (uint32_t)(best - sbase);
                    const R4<R> sk = kargs()->sc.sph[k];
                    outward = PR::divs(pnt - mk(sk.x, sk.y, sk.z), kargs()->sc.sph_r[k]);  // sphere.rs:82-83
                    // one level of loads: the sphere's material kind and
                    // parameters are copied per sphere (sph_mat word: id,
                    // kind, isolated flag; sph_shade: albedo + fuzz | ior)
                    const uint32_t mw = kargs()->sc.sph_mat[k];
                    m = mw & 0xffffffu;
                    mtype = (mw >> 24) & 0x7fu;
                    mp = kargs()->sc.sph_shade[k];
                    next_self = (mw >> 31) ? (int32_t)k : -1;   // bit 31: isolated sphere
                    if constexpr (kHit64) {
                        next_self = (int32_t)k;
                        next_iso = (mw >> 31) != 0;
                        // Metal / Dielectric scatter in f64 from the f64 normal: their
                        // directions decide the next re-hit at the ulp level
                        bool scatter64 = mtype == kMatMetal || mtype == kMatDielectric;
                        RTW_PROBE_ABL_SCATTER(scatter64);
                        if (scatter64) {
                            n64 = sphere_normal64(pnt64, kargs()->sc.sph64[k]);
                            outward = mk((float)n64.x, (float)n64.y, (float)n64.z);
                            sph_hit = true;
                        }
                    }
                    if constexpr (kTex) sphere_uv(outward, hu, hv);
                }
                bool front = box_hit ? box_front : dot(d, outward) < (R)0;
                if constexpr (kHit64) {
                    if (sph_hit) {                                 // the f64 front face and normal
                        front = front64(d64, n64);
                        if (!front) n64 = -n64;
                    }
                }
                const V3<R> nrm = front ? outward : -outward;
                // Material::emitted: DiffuseLight's colour (material.rs:508-514),
                // black for every other material (material.rs:42-44)
                // the material's colour: its texture at (u, v, p) (kTex) or its SolidColour
                V3<R> colour = mk(mp.x, mp.y, mp.z);
                if constexpr (kTex) {
                    if (mtype == kMatDiffuseLight || mtype == kMatLambertian)
                        colour = tex_colour(p.sc, kargs()->sc.mat_tex[m], hu, hv, pnt);
                }
                const V3<R> emitted = kEmit && mtype == kMatDiffuseLight ? colour : zero;
                RTW_PROBE_CLK(3);
                if (kHit64 && sph_hit) {
                    // Metal / Dielectric sphere: the f64 scatter of both in one pass
                    RTW_PROBE_LANES(7);
                    const bool metal = mtype == kMatMetal;
                    bool keep;
                    RTW_PROBE_SCATTER64(specular_dir64(metal, d64, n64, front, kargs()->sc.mat64[m], g2, keep2).y);
                    d64 = specular_dir64(metal, d64, n64, front, kargs()->sc.mat64[m], g, keep);
                    if (!keep) {
                        col = mult * emitted + res.value();
                        done = true;
                    } else {
                        if (metal) mult = mult * mk(mp.x, mp.y, mp.z);   // Reflect, camera.rs:488-500
                        o = pnt;                          // (Dielectric: mult * (1, 1, 1) = mult)
                        self_s = next_self;
                        self_iso = next_iso;
                        o64 = pnt64;
                        d = from64<R>(d64);
                    }
                    RTW_PROBE_CLK(6);
                } else if (sizeof(R) == 8 && (mtype == kMatMetal || mtype == kMatDielectric)) {
                    // f64: Metal::scatter and Dialectric::scatter (material.rs:407-421,
                    // 458-487) in one pass (specular_dir64 with the reference's
                    // UnitSphere loop and the material's f64 record: 1 / ior and both
                    // faces' Schlick r0 computed on the host with the reference's
                    // operations), so a wave whose lanes hit both runs it once
                    RTW_PROBE_LANES(7);
                    const bool metal = mtype == kMatMetal;
                    bool keep;
                    const V3<double> dir = specular_dir64<true>(metal, to64(d), to64(nrm), front,
                                                                kargs()->sc.mat64[m], g, keep);
                    if (!keep) {
                        col = mult * emitted + res.value();
                        done = true;
                    } else {
                        if (metal) mult = mult * mk(mp.x, mp.y, mp.z);   // Reflect, camera.rs:488-500
                        o = pnt;                                          // (Dielectric: mult * (1, 1, 1) = mult)
                        self_s = next_self;
                        self_iso = next_iso;
                        d = from64<R>(dir);
                    }
                    RTW_PROBE_CLK(6);
                } else if (mtype == kMatMetal) {
                    RTW_PROBE_LANES(7);
                    // Metal::scatter, material.rs:407-421
                    V3<R> refl = reflect(PR::normalize(d), nrm);
                    const V3<R> dir = refl + unit_sphere<R>(g) * mp.w;
                    if (!(dot(dir, nrm) > (R)0)) {
                        col = mult * emitted + res.value();
                        done = true;
                    } else {
                        mult = mult * mk(mp.x, mp.y, mp.z);            // Reflect, camera.rs:488-500
                        o = pnt;
                        self_s = next_self;
                        self_iso = next_iso;
                        if constexpr (kHit64) {
                            o64 = pnt64;
                            d64 = dither64(dir);
                        }
                        d = dir;
                    }
                    RTW_PROBE_CLK(7);
                } else if (mtype == kMatDielectric) {
                    RTW_PROBE_LANES(8);
                    // Dialectric::scatter, material.rs:458-487
                    V3<R> dir;
                    R ratio = front ? PR::div_((R)1, mp.w) : mp.w;
                    V3<R> unit = PR::normalize(d);
                    R cos_t = PR::min_(dot(unit, -nrm), (R)1);
                    R sin_t = PR::sqrt_((R)1 - cos_t * cos_t);
                    bool cannot = ratio * sin_t > (R)1;
                    if (cannot || reflectance(cos_t, ratio) > PR::u_open01(g.next()))
                        dir = reflect(unit, nrm);
                    else
                        dir = refract(unit, nrm, ratio);
                    if constexpr (kHit64) d64 = dither64(dir);
                    // mult * Colour(1, 1, 1) is the identity on every value
                    o = pnt;
                    self_s = next_self;
                    self_iso = next_iso;
                    if constexpr (kHit64) o64 = pnt64;
                    d = dir;
                    RTW_PROBE_CLK(8);
                } else if (mtype == kMatLambertian) {
                    RTW_PROBE_LANES(9);
                    // Lambertian + MixturePdf(HittablePdf(lights), CosinePdf):
                    // material.rs:357-376, pdf.rs:33-101, camera.rs:504-521
                    lamb = true;
                    const V3<R> att = colour;
                    // the normal's Onb (onb.rs:8-35) is built by mixture_direction
                    // for the cosine lanes only; the pdf needs its w = normalize(n)
                    // (computed after the direction: not held across the sampling)
                    V3<R> dir;
                    const bool to_light = PR::u_std(g.next()) < (R)0.5;
                    bool sampled = false;
                    bool nan_dir = false;   // (light kernels) an empty light list: a NaN direction
                    if (to_light && (kargs()->sc.n_list == 0 || (kPrims && kargs()->sc.lref))) {
                        // HittableList::random (hittable_list.rs:414-419): a
                        // uniform light (one gen_index draw), then its random()
                        // (no lref list without kPrims: the light kernels drop that code
                        // and take an empty list's NaN direction below, as a select after
                        // the cosine lobe's draws -- a direction assigned on two paths was
                        // spilled at every Lambertian bounce; the Book-1 kernels keep this
                        // code -- dropped there, the f64 kernel's registers were allocated
                        // worse: +0.5 %)
                        if constexpr (kLightBvh && !kPrims) {
                            nan_dir = true;
                            atomicAdd(p.counters + 5, 1ull);
                        } else if (kargs()->sc.n_list == 0) {
                            // an empty list panics there (:417): counted; the
                            // sample goes on along a NaN direction and ends NaN
                            // at its next world query, as in the oracle
                            sampled = true;
                            atomicAdd(p.counters + 5, 1ull);
                            dir = mk((R)NAN, (R)NAN, (R)NAN);
                        } else {
                            sampled = true;
                            const uint32_t ref = kargs()->sc.lref[g.index(kargs()->sc.n_list)];
                            if (ref & kLrefQuad) {
                                dir = quad_random(kargs()->sc.lquads + kQuadR * (ref & 0x3fffffffu), pnt, g);
                            } else if (ref & kLrefDefault) {
                                dir = mk<R>(1, 0, 0);              // Hittable::random default
                            } else {
                                const R4<R> L = li[ref];
                                dir = sphere_random(mk(L.x, L.y, L.z), L.w, pnt, g);
                            }
                        }
                    }
                    int32_t lsel = -1;   // the sampled light (f32: always counted in the pdf)
                    V3<double> dir64l = {0.0, 0.0, 0.0};   // kHit64: the f64 direction
                    bool have64 = false;
                    if (!sampled) {
                        // a sphere light (one gen_index draw, then Sphere::random)
                        // or the cosine lobe, in one pass (mixture_direction)
                        R4<R> L = R4<R>{0, 0, 0, 0};
                        const bool tl = to_light && !nan_dir;
                        if (tl) {
                            lsel = (int32_t)g.index(kargs()->sc.n_lights);
                            L = li[lsel];
                        }
                        if constexpr (kHit64) {
                            // the Lambertian direction in f64 from the f64 normal (same
                            // words, the f64 kernels' forms -- FMA-contracted in this unit, DESIGN.md
                            // §2b: within rounding of them, not their bits; with the azimuth's sin /
                            // cos in f32 it was 1.9 % faster, but the paths' statistics fell
                            // back to the f32 direction's: profiles/r05_hit64_trig32_ab.jsonl)
                            V3<double> nl = to64(nrm);
                            if (best >= sbase) {
                                nl = sphere_normal64(pnt64, kargs()->sc.sph64[best - sbase]);
                                if (!front64(d64, nl)) nl = -nl;
                            }
                            dir64l = mixture_direction(tl, nl, V3<double>{(double)L.x, (double)L.y, (double)L.z},
                                                       (double)L.w, pnt64, g);
                            dir = from64<R>(dir64l);
                            have64 = true;
                        } else {
                            dir = mixture_direction(tl, nrm, mk(L.x, L.y, L.z), L.w, pnt, g);
                        }
                    }
                    if constexpr (kLightBvh && !kPrims) {
                        dir = nan_dir ? mk((R)NAN, (R)NAN, (R)NAN) : dir;
                        dir64l = nan_dir ? V3<double>{(double)NAN, (double)NAN, (double)NAN} : dir64l;
                    }
                    RTW_PROBE_LAMBERT_DIR();
                    RTW_PROBE_CLK(4);
                    const V3<R> ndir = PR::normalize(dir);
                    const V3<R> wn = PR::normalize(nrm);
                    const R cos_w = PR::over_pi(dot(ndir, wn));
                    R acc;                                                // hittable_list.rs:408-412
                    // the light walks of the light BVH / grid kernels: deferred to the end
                    // of the trip (the grid's by the whole wave, the others per lane)
                    if constexpr (kCoopGrid) {
                        const R spdf = PR::max_(PR::over_pi(dot(nrm, ndir)), (R)0);
                        pend = true;
                        pend_aw = att * spdf;
                        pend_ch = PR::max_(cos_w, (R)0) * (R)0.5;
                        res.add(mult, emitted);
                        o = pnt;
                        self_s = next_self;
                        self_iso = next_iso;
                        if constexpr (kHit64) {
                            o64 = pnt64;
                            d64 = have64 ? dir64l : dither64(dir);
                        }
                        d = dir;
                    } else {
                    if (kPrims && kargs()->sc.lref)
                        acc = lights_pdf_mixed(p.sc, li, pnt, dir);
                    else if constexpr (kLightBvh) {
                        LightWork lw;
                        RTW_KARG_SCENE(wsc);
                        acc = kargs()->light_bvh == 2
                                  ? lights_pdf_grid<kRobust>(wsc, pnt, dir, lw)
                                  : lights_pdf_bvh<kRobust>(wsc, pnt, dir,
                                                            reinterpret_cast<int32_t*>(smem) + wave * p.stack * 64 + lane,
                                                            lw);
                        light_work_lane(wcnt, lw);
                    } else if constexpr (kWorld == kWorldBvhLds && sizeof(R) == 4)
                        acc = lights_pdf_sum_pk<kRobust>(li, l_lp, kargs()->sc.n_lights, pnt, dir, lsel);
                    else if constexpr (kWorld == kWorldBvhLds && sizeof(R) == 8)
                        acc = lights_pdf_sum<kRobust>(li, kargs()->sc.n_lights, pnt, dir, l_li32);
                    else
                        acc = lights_pdf_sum<kRobust>(li, kargs()->sc.n_lights, pnt, dir);
                    RTW_PROBE_LIGHT_PDF();
                    RTW_PROBE_CLK(5);
                    // / len; a BVH leaf list multiplies by len and divides again (bvh.rs:67-76, 191-194)
                    R lpdf = PR::div_(acc, (R)p.sc.n_list);
                    if (p.sc.light_flags & 1u) lpdf = PR::div_(lpdf * (R)p.sc.n_list, (R)p.sc.n_list);
                    const R pdf = lpdf * (R)0.5 + PR::max_(cos_w, (R)0) * (R)0.5;
                    const R spdf = PR::max_(PR::over_pi(dot(nrm, ndir)), (R)0);
                    const V3<R> w = PR::divs(att * spdf, pdf);
                    const V3<R> new_mult = mult * w;
                    RTW_PROBE_NAN_LAMBERT(__builtin_isnan(mult.x + mult.y + mult.z),
                                          __builtin_isnan(new_mult.x + new_mult.y + new_mult.z), best);
                    res.add(mult, emitted);
                    mult = new_mult;
                    o = pnt;
                    self_s = next_self;
                    self_iso = next_iso;
                    if constexpr (kHit64) {
                        o64 = pnt64;
                        d64 = have64 ? dir64l : dither64(dir);
                    }
                    d = dir;
                    }
                    RTW_PROBE_CLK(4);
                } else {
                    // Invisible (material.rs:321-325): scatter() == None
                    col = mult * emitted + res.value();
                    done = true;
                }
                if (!done) {
                    depth -= 1;
                    if (depth == 0) {                                  // camera.rs:470-472
                        col = zero + res.value();
                        done = true;
                        if constexpr (kCoopGrid) pend = false;         // its pdf is not needed
                    }
                }
            }
            if (done) {
                RTW_PROBE_SAMPLE_END();
                // the item's running sum lives in its chunk-sum slot, not in
                // registers: (0 + s_first) on the first sample, then slot + s
                // -- the fold of camera.rs:323-335 in the same order
                const KArgs* k = kargs();
                R* dst = k->partial + ((size_t)slot * k->n_chunks + c) * 3;
                V3<R> prev = zero;
                if (k->chunk > 1) {   // (wave-uniform: one sample per item never reads the slot)
                    if (s != c * k->chunk) prev = mk(dst[0], dst[1], dst[2]);
                }
                const V3<R> part = prev + col;
                dst[0] = part.x;
                dst[1] = part.y;
                dst[2] = part.z;
                if (k->tile_cost) {   // tile costs for the task order: this sample's work
                    if (s < k->cost_spp && !k->cost_time)
                        atomicAdd(k->tile_cost + (slot >> 6), nvis + ntest + kCostPerSegment * (k->max_depth - depth + 1u));
                }
                ++s;
                if (s < min((c + 1u) * k->chunk, k->spp)) {
                    RTW_PROBE_SEED();
                    start_sample();
                RTW_PROBE_LANES(10);
                } else {
                    active = false;
                    need = true;
                }
            }
        }
        RTW_PROBE_CLK(9);
        lambs += (uint32_t)__popcll(__ballot(lamb));
        if constexpr (kCoopGrid) {
            // the deferred Lambertian light pdfs of this trip, by the whole wave;
            // then the path throughput as in the Lambertian branch
            // (wave-uniform) the grid's walk by the whole wave; else -- the light
            // BVH, or the grid with grid_piece 0 -- each lane walks for its own
            // ray here, where less of the path state is live than at the bounce
            const bool coop_walk = kargs()->light_bvh == 2 && kargs()->grid_piece != 0;
            if (!coop_walk && __any(pend)) {
                const V3<R> po = kHit64 ? from64<R>(o64) : o, pd = kHit64 ? from64<R>(d64) : d;
                R acc = (R)0;
                if (pend) {
                    LightWork lw;
                    RTW_KARG_SCENE(wsc);
                    acc = kargs()->light_bvh == 2
                              ? lights_pdf_grid<kRobust>(wsc, po, pd, lw)
                              : lights_pdf_bvh<kRobust>(wsc, po, pd,
                                                        reinterpret_cast<int32_t*>(smem) + wave * p.stack * 64 + lane, lw);
                    light_work_lane(wcnt, lw);
                    R lpdf = PR::div_(acc, (R)p.sc.n_list);
                    if (p.sc.light_flags & 1u) lpdf = PR::div_(lpdf * (R)p.sc.n_list, (R)p.sc.n_list);
                    const R pdf = lpdf * (R)0.5 + pend_ch;
                    mult = mult * PR::divs(pend_aw, pdf);
                    pend = false;
                }
            }
            if (coop_walk && __any(pend)) {
                // The walk's registers come on top of the whole path state: the RNG
                // state and (hit64) the f64 ray wait in the wave's LDS stack area
                // ([word][lane]; the host sizes p.stack >= kCoopStash + 1) instead of
                // being spilled to scratch by the compiler; the pieces' slots follow.
                // (f64: the RNG state, the pending ray (o, d) itself, and the
                // throughput and the pending bounce's weights -- without those the
                // compiler spilled ~28 dwords per lane around every walk)
                constexpr uint32_t kStash = sizeof(R) == 8 ? kCoopStash64 : (kHit64 ? 20u : 8u);
                static_assert(kStash < (sizeof(R) == 8 ? kCoopStash64 : kCoopStash) + 1,
                              "the host's stack minimum covers the stash");
                uint32_t* area = reinterpret_cast<uint32_t*>(smem) + wave * p.stack * 64;
                // hit64: the pending ray is (o64, d64) rounded (o = pnt, d = dir), so o and d
                // need not stay live to here
                const V3<R> po = kHit64 ? from64<R>(o64) : o, pd = kHit64 ? from64<R>(d64) : d;
                auto put = [&](uint32_t k, uint64_t v) {
                    area[(2 * k) * 64 + lane] = (uint32_t)v;
                    area[(2 * k + 1) * 64 + lane] = (uint32_t)(v >> 32);
                };
                auto get = [&](uint32_t k) {
                    return (uint64_t)area[(2 * k) * 64 + lane] | ((uint64_t)area[(2 * k + 1) * 64 + lane] << 32);
                };
                auto dbits = [](double x) { return (uint64_t)__double_as_longlong(x); };
                auto bitsd = [](uint64_t x) { return __longlong_as_double((long long)x); };
                put(0, g.s0);
                put(1, g.s1);
                put(2, g.s2);
                put(3, g.s3);
                if constexpr (kHit64) {
                    put(4, dbits(o64.x)); put(5, dbits(o64.y)); put(6, dbits(o64.z));
                    put(7, dbits(d64.x)); put(8, dbits(d64.y)); put(9, dbits(d64.z));
                } else if constexpr (sizeof(R) == 8) {
                    put(4, dbits(o.x)); put(5, dbits(o.y)); put(6, dbits(o.z));
                    put(7, dbits(d.x)); put(8, dbits(d.y)); put(9, dbits(d.z));
                    put(10, dbits(mult.x)); put(11, dbits(mult.y)); put(12, dbits(mult.z));
                    put(13, dbits(pend_aw.x)); put(14, dbits(pend_aw.y)); put(15, dbits(pend_aw.z));
                    put(16, dbits(pend_ch));
                }
                R acc;
                LightWork lw;
                // the walk's sections for the clock probes (RTW_CLOCK): 13 setup, 14 the
                // pieces' walks, 15 the owners' sums
                auto walk_mark = [&](int id) { (void)id; RTW_PROBE_CLK(id); };
                RTW_PROBE_CLK(11);
                if constexpr (sizeof(R) == 8) {
                    // (the pending ray: stash words 4..9, put above)
                    // the grid's fields read from the kernel arguments here (RTW_KARG_SCENE)
                    RTW_KARG_SCENE(wsc);
                    Grid64 gr;
                    gr.lg_start = wsc.lg_start;
                    gr.lg_rec = wsc.lg_rec;
                    gr.lg_sph32 = wsc.lg_sph32;
                    gr.lg_id = wsc.lg_id;
                    gr.lights = wsc.lights;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        gr.lo[a] = (float)wsc.lg_lo[a];
                        gr.hi[a] = (float)wsc.lg_hi[a];
                        gr.cell[a] = (float)wsc.lg_cell[a];
                        gr.inv[a] = (float)wsc.lg_inv[a];
                        gr.n[a] = wsc.lg_n[a];
                    }
                    gr.big = wsc.lg_big;
                    acc = lights_pdf_grid_coop64(gr, pend, area + 8 * 64, kargs()->grid_piece, area + kStash * 64,
                                                 (kargs()->stack - kStash) * 64, lane, lw, walk_mark);
                } else {
                    float* slots = reinterpret_cast<float*>(area + kStash * 64);
                    RTW_KARG_SCENE(wsc);
                    acc = lights_pdf_grid_coop<kRobust>(wsc, pend, po, pd, kargs()->grid_piece, slots,
                                                        (kargs()->stack - kStash) * 64, lane, lw, walk_mark);
                }
                light_work_wave(wcnt, lw, lane);
                g.s0 = get(0);
                g.s1 = get(1);
                g.s2 = get(2);
                g.s3 = get(3);
                if constexpr (kHit64) {
                    o64 = V3<double>{bitsd(get(4)), bitsd(get(5)), bitsd(get(6))};
                    d64 = V3<double>{bitsd(get(7)), bitsd(get(8)), bitsd(get(9))};
                } else if constexpr (sizeof(R) == 8) {
                    o = V3<R>{(R)bitsd(get(4)), (R)bitsd(get(5)), (R)bitsd(get(6))};
                    d = V3<R>{(R)bitsd(get(7)), (R)bitsd(get(8)), (R)bitsd(get(9))};
                    mult = V3<R>{(R)bitsd(get(10)), (R)bitsd(get(11)), (R)bitsd(get(12))};
                    pend_aw = V3<R>{(R)bitsd(get(13)), (R)bitsd(get(14)), (R)bitsd(get(15))};
                    pend_ch = (R)bitsd(get(16));
                }
                if (pend) {
                    R lpdf = PR::div_(acc, (R)p.sc.n_list);
                    if (p.sc.light_flags & 1u) lpdf = PR::div_(lpdf * (R)p.sc.n_list, (R)p.sc.n_list);
                    const R pdf = lpdf * (R)0.5 + pend_ch;
                    mult = mult * PR::divs(pend_aw, pdf);
                    pend = false;
                }
            }
            RTW_PROBE_CLK(11);
        }
        acquire();
        RTW_PROBE_CLK(0);
    }
    RTW_PROBE_CLK(10);
    RTW_PROBE_CLK_END();
    RTW_PROBE_WAVE_END();
    // wave-reduce the per-lane counters (segs, lambs are per wave), one atomic per wave
    for (int off = 32; off > 0; off >>= 1) {
        nvis += __shfl_xor(nvis, off);
        ntest += __shfl_xor(ntest, off);
    }
    if (lane == 0 && p.counters) {
        atomicAdd(p.counters + 0, (unsigned long long)segs);
        atomicAdd(p.counters + 1, (unsigned long long)lambs);
        if (nvis) atomicAdd(p.counters + 2, (unsigned long long)nvis);
        if (ntest) atomicAdd(p.counters + 3, (unsigned long long)ntest);
        if constexpr (kLightBvh) {
            if (wcnt[0]) atomicAdd(p.counters + 7, wcnt[0]);
            if (wcnt[1]) atomicAdd(p.counters + 8, wcnt[1]);
        }
    }
}

// Fold the chunk sums of every pixel in chunk order and write the rank's
// packed tiles: out[(lt * 64 + px) * 3], px = ly * 8 + lx (pixels outside the
// image: 0).  The fold accumulates in double whatever R is: with many chunks
// (C4: 4096 spp) an f32 running sum would lose low bits; in f64 mode this is
// the reference's sequential f64 fold (camera.rs:323-335).
// chunks staged per pass: 12 KiB of LDS per wave in f32; f64 12 chunks (19
// KiB: the step 0.24 ms shorter than at 8, profiles/r04_h_fold_window_ab.txt;
// 16 took 25 KiB: six waves per CU, too few to keep the loads in flight)
template <typename R>
constexpr uint32_t kFoldWindow = sizeof(R) == 4 ? 16 : RTW_FOLD_WIN64;

template <typename R>
__global__ void __launch_bounds__(64) reduce_chunks_kernel(const KParams<R> p, R* __restrict__ out,
                                                           const uint8_t* __restrict__ cull) {
    constexpr uint32_t kFoldWin = kFoldWindow<R>;
    constexpr uint32_t kFoldRow = kFoldWin * 3 + 1;    // LDS row (odd: no bank conflicts)
    // one wave per tile; a pixel's chunk sums are contiguous (the sample-major
    // item pool hands the lanes consecutive chunks of one pixel, whose sums
    // then fill whole cache lines together), so the wave stages a window of
    // kFoldWin chunks x 64 pixels through LDS with row-contiguous loads and
    // each lane folds its pixel's row in chunk order
    __shared__ R win[64 * kFoldRow];
    const uint32_t lt = blockIdx.x, lane = threadIdx.x;
    const uint32_t T = global_tile(p, lt);
    const uint32_t ty = T / p.tiles_x, tx = T - ty * p.tiles_x;
    const uint32_t i = tx * kTile + (lane & 7), j = ty * kTile + (lane >> 3);
    const size_t row_len = (size_t)p.n_chunks * 3;
    const R* tile = p.partial + (size_t)lt * 64 * row_len;
    double sx = 0, sy = 0, sz = 0;
    // a provably empty tile (block-uniform): its chunk sums were never written
    const bool empty = cull && cull[lt];
    if (empty) {
        sx = fold_constant<R>(sx, miss_colour(p.bg[0]), p.spp, p.chunk);
        sy = fold_constant<R>(sy, miss_colour(p.bg[1]), p.spp, p.chunk);
        sz = fold_constant<R>(sz, miss_colour(p.bg[2]), p.spp, p.chunk);
    }
    constexpr uint32_t kNv = kFoldWin * 3;
    for (uint32_t c0 = 0; c0 < (empty ? 0u : p.n_chunks); c0 += kFoldWin) {
        const uint32_t kw = min(kFoldWin, p.n_chunks - c0), nv = kw * 3;
        const R* src = tile + (size_t)c0 * 3;
        if (kw == kFoldWin) {
            // full window: every lane's kNv loads issued back to back
            R v[kNv];
#pragma unroll
            for (uint32_t it = 0; it < kNv; ++it) {
                const uint32_t idx = it * 64 + lane, r = idx / kNv, col = idx - r * kNv;
                v[it] = src[r * row_len + col];
            }
#pragma unroll
            for (uint32_t it = 0; it < kNv; ++it) {
                const uint32_t idx = it * 64 + lane, r = idx / kNv, col = idx - r * kNv;
                win[r * kFoldRow + col] = v[it];
            }
        } else {
            for (uint32_t idx = lane; idx < 64 * nv; idx += 64) {
                const uint32_t r = idx / nv, col = idx - r * nv;
                win[r * kFoldRow + col] = src[r * row_len + col];
            }
        }
        __syncthreads();
        const R* row = win + lane * kFoldRow;
        for (uint32_t k = 0; k < kw; ++k) {
            sx = sx + (double)row[3 * k];
            sy = sy + (double)row[3 * k + 1];
            sz = sz + (double)row[3 * k + 2];
        }
        __syncthreads();
    }
    if (i >= p.W || j >= p.H) sx = sy = sz = 0;   // never written
    R* dst = out + ((size_t)lt * 64 + lane) * 3;
    dst[0] = (R)sx;
    dst[1] = (R)sy;
    dst[2] = (R)sz;
}

// The continuing form of reduce_chunks_kernel (sample windows, KParams::s_base):
// each pixel's running sum starts from accum[(lt * 64 + px) * 3] -- the sums of
// the samples before the window, always f64: an f32 carry would round between
// windows, the one-shot fold rounds once -- or from 0 when `first_sample` is 0
// (accum's contents are then ignored), takes the window's chunk sums in chunk
// order and goes back to accum; `out` (may be null) also receives it rounded to
// R, the packed tiles of reduce_chunks_kernel.  Windows of a render folded one
// after another are the one-shot fold at the same chunk, addition by addition.
template <typename R>
__global__ void __launch_bounds__(64) fold_window_kernel(const KParams<R> p, double* __restrict__ accum,
                                                         uint32_t first_sample, R* __restrict__ out,
                                                         const uint8_t* __restrict__ cull) {
    constexpr uint32_t kFoldWin = kFoldWindow<R>;
    constexpr uint32_t kFoldRow = kFoldWin * 3 + 1;    // LDS row (odd: no bank conflicts)
    __shared__ R win[64 * kFoldRow];
    const uint32_t lt = blockIdx.x, lane = threadIdx.x;
    const uint32_t T = global_tile(p, lt);
    const uint32_t ty = T / p.tiles_x, tx = T - ty * p.tiles_x;
    const uint32_t i = tx * kTile + (lane & 7), j = ty * kTile + (lane >> 3);
    const size_t row_len = (size_t)p.n_chunks * 3;
    const R* tile = p.partial + (size_t)lt * 64 * row_len;
    double* acc = accum + ((size_t)lt * 64 + lane) * 3;
    double sx = 0, sy = 0, sz = 0;
    if (first_sample) {
        sx = acc[0];
        sy = acc[1];
        sz = acc[2];
    }
    // a provably empty tile (block-uniform), as reduce_chunks_kernel: the window's samples onto the carry
    const bool empty = cull && cull[lt];
    if (empty) {
        sx = fold_constant<R>(sx, miss_colour(p.bg[0]), p.spp, p.chunk);
        sy = fold_constant<R>(sy, miss_colour(p.bg[1]), p.spp, p.chunk);
        sz = fold_constant<R>(sz, miss_colour(p.bg[2]), p.spp, p.chunk);
    }
    constexpr uint32_t kNv = kFoldWin * 3;
    for (uint32_t c0 = 0; c0 < (empty ? 0u : p.n_chunks); c0 += kFoldWin) {
        const uint32_t kw = min(kFoldWin, p.n_chunks - c0), nv = kw * 3;
        const R* src = tile + (size_t)c0 * 3;
        if (kw == kFoldWin) {
            // full pass: every lane's kNv loads issued back to back (as reduce_chunks_kernel)
            R v[kNv];
#pragma unroll
            for (uint32_t it = 0; it < kNv; ++it) {
                const uint32_t idx = it * 64 + lane, r = idx / kNv, col = idx - r * kNv;
                v[it] = src[r * row_len + col];
            }
#pragma unroll
            for (uint32_t it = 0; it < kNv; ++it) {
                const uint32_t idx = it * 64 + lane, r = idx / kNv, col = idx - r * kNv;
                win[r * kFoldRow + col] = v[it];
            }
        } else {
            for (uint32_t idx = lane; idx < 64 * nv; idx += 64) {
                const uint32_t r = idx / nv, col = idx - r * nv;
                win[r * kFoldRow + col] = src[r * row_len + col];
            }
        }
        __syncthreads();
        const R* row = win + lane * kFoldRow;
        for (uint32_t k = 0; k < kw; ++k) {
            sx = sx + (double)row[3 * k];
            sy = sy + (double)row[3 * k + 1];
            sz = sz + (double)row[3 * k + 2];
        }
        __syncthreads();
    }
    if (i >= p.W || j >= p.H) sx = sy = sz = 0;   // never written
    acc[0] = sx;
    acc[1] = sy;
    acc[2] = sz;
    if (out) {
        R* dst = out + ((size_t)lt * 64 + lane) * 3;
        dst[0] = (R)sx;
        dst[1] = (R)sy;
        dst[2] = (R)sz;
    }
}

// Un-interleave the ranks' packed tiles into the image [H][W][3]: one thread
// per pixel slot of every global tile T (v = slot[T], or T for the round
// robin: rank v % nranks, its local tile v / nranks).  ranks = nranks
// buffers, rank_stride elements apart.
template <typename R>
__global__ void __launch_bounds__(256) assemble_tiles_kernel(const R* __restrict__ ranks, size_t rank_stride,
                                                             uint32_t nranks, uint32_t W, uint32_t H,
                                                             uint32_t tiles_x, uint32_t n_tiles,
                                                             const uint32_t* __restrict__ slot,
                                                             R* __restrict__ img) {
    const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
    const uint32_t T = gid >> 6, lane = gid & 63;
    if (T >= n_tiles) return;
    const uint32_t ty = T / tiles_x, tx = T - ty * tiles_x;
    const uint32_t i = tx * kTile + (lane & 7), j = ty * kTile + (lane >> 3);
    if (i >= W || j >= H) return;
    const uint32_t v = slot ? slot[T] : T;
    const uint32_t k = v % nranks, lt = v / nranks;
    const R* src = ranks + k * rank_stride + ((size_t)lt * 64 + lane) * 3;
    R* dst = img + ((size_t)j * W + i) * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
}

}  // namespace dev

}  // namespace rtw
