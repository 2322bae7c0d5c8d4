// light_pdf.hpp -- the light pdf of a Lambertian bounce (HittableList::pdf_value
// over the light list): the linear sums over a staged list, the all-hits
// queries through the light BVH and the light grid (per lane, and the
// wave-cooperative walks of the f32 and f64 kernels), and the mixed list with
// quads.
#pragma once

#include "bvh_traverse.hpp"
#include "light_grid.hpp"
#include "rtw_device.hpp"
#include "rtw_kernels.h"

namespace rtw {

namespace dev {

// Sum of Sphere::pdf_value over the light list in list order
// (HittableList::pdf_value, hittable_list.rs:408-412; sphere.rs:101-111).
// f64: the reference's arithmetic, light by light, for every light an f32
// pre-pass cannot rule out.  A light the ray misses adds exactly +0.0 (the sum
// starts at +0.0), so skipping it changes no bit.  The pre-pass rounds the ray
// and the light to f32 and tests the closest approach l (see light_hit_f32)
// against r + E and the direction (hb <= 0 or the origin inside) with slack,
// E = 2^-18 (max(|o|_1, 2^-32) + |c|_1 + r): far above the f32 error of l (a
// few 2^-24 (|o| + |c|)) and of the f64 decision itself (disc's rounding), so
// every light the f64 test hits stays in -- while the f32 values are normal
// numbers: the floor under |o|_1 (light_on) keeps E^2 normal for tiny scenes,
// and the compares keep a light on NaN (coordinates beyond f32: inf - inf), so
// the scene's size is free; the direction must keep d . d, its reciprocal and
// d . (o - c) normal f32 numbers: |d|_1 within 2^-60 .. 2^46 (include/rtw.h
// states that range; above it hb can overflow against a finite bound).
// li32 (may be null): the same lights rounded to f32 with |radius| (staged in
// LDS by the LDS-world kernels): the pre-pass reads them instead of converting
// the f64 records -- the same f32 values, the same mask
// the pre-pass test of one light {c, |r|} (rounded to f32) against the f32 ray
__device__ __forceinline__ bool light_may_hit(float cx, float cy, float cz, float r, float ox, float oy, float oz,
                                              float dx, float dy, float dz, float ia, float on, float dn) {
    const float fx = ox - cx, fy = oy - cy, fz = oz - cz;
    const float hb = __builtin_fmaf(dz, fz, __builtin_fmaf(dy, fy, dx * fx));
    const float tc = -hb * ia;
    const float lx = __builtin_fmaf(tc, dx, fx), ly = __builtin_fmaf(tc, dy, fy), lz = __builtin_fmaf(tc, dz, fz);
    const float l2 = __builtin_fmaf(lx, lx, __builtin_fmaf(ly, ly, lz * lz));
    const float f2 = __builtin_fmaf(fx, fx, __builtin_fmaf(fy, fy, fz * fz));
    const float e = 0x1p-18f * (on + fabsf(cx) + fabsf(cy) + fabsf(cz) + r);   // on >= 2^-32: light_on
    const float rr = (r + e) * (r + e);
    // the compares keep the light on a NaN: coordinates beyond f32 (inf - inf)
    // decide nothing here, the f64 test does (a NaN ray's pdf is 0 there too)
    return !(l2 > rr) & (!(hb > 2.0f * e * dn) | !(f2 > rr));
}
// The f32 ray of the pre-pass: o, d rounded, 1 / (d . d), |o|_1, |d|_1
struct LightPre {
    float ox, oy, oz, dx, dy, dz, ia, on, dn;
    __device__ __forceinline__ LightPre(V3<double> o, V3<double> d)
        : ox((float)o.x), oy((float)o.y), oz((float)o.z), dx((float)d.x), dy((float)d.y), dz((float)d.z) {
        ia = __builtin_amdgcn_rcpf(__builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz)));
        on = light_on(ox, oy, oz);
        dn = fabsf(dx) + fabsf(dy) + fabsf(dz);
    }
    __device__ __forceinline__ bool may_hit(const R4<double>& L) const {
        return light_may_hit((float)L.x, (float)L.y, (float)L.z, fabsf((float)L.w), ox, oy, oz, dx, dy, dz, ia, on, dn);
    }
};

// Inserts x into ids[0..kMax) (ascending; empty entries ~0u) by one
// compare-exchange pass with static indices -- a shifting insertion's dynamic
// register indices compile to 8-way select chains per step -- and returns the
// value that fell off the end (~0u: none did).
template <uint32_t kMax>
__device__ __forceinline__ uint32_t sorted_insert(uint32_t (&ids)[kMax], uint32_t x) {
#pragma unroll
    for (uint32_t q = 0; q < kMax; ++q) {
        const uint32_t a = ids[q];
        ids[q] = min(a, x);
        x = max(a, x);
    }
    return x;
}

// HittableList::pdf_value's sum over the hit lights in LIST order (f64) when
// an acceleration structure finds them in another order: `walk(lo, add)` calls
// add(id) once for every light the ray hits, in any order, and each pass keeps
// the kMax smallest list indices >= lo; their pdfs are added in index order
// and, when the pass had to drop hits, the next pass continues above the last
// index summed.  (A ray skimming C5's flat light layer hits ~10 lights.)
// (R: the sum's type; pdf(id): light id's pdf)
template <typename R, typename Walk, typename Pdf>
__device__ __forceinline__ R lights_sum_ids_in_list_order(Walk&& walk, Pdf&& pdf) {
    constexpr uint32_t kMax = 8;
    R acc = (R)0;
    uint32_t lo = 0;
    for (;;) {
        uint32_t ids[kMax];
#pragma unroll
        for (uint32_t q = 0; q < kMax; ++q) ids[q] = 0xffffffffu;
        bool dropped = false;
        walk([&](uint32_t id) {
            if (id < lo) return;
            // by list index; when full the largest gives way
            if (sorted_insert(ids, id) != 0xffffffffu) dropped = true;
        });
        for (uint32_t q = 0; q < kMax && ids[q] != 0xffffffffu; ++q) acc = acc + pdf(ids[q]);
        if (!dropped) return acc;
        lo = ids[kMax - 1] + 1u;
    }
}
template <typename Walk>
__device__ __forceinline__ double lights_sum_in_list_order(const R4<double>* __restrict__ lights, V3<double> o,
                                                           V3<double> d, Walk&& walk) {
    return lights_sum_ids_in_list_order<double>(walk, [&](uint32_t id) {
        const R4<double> L = lights[id];
        return sphere_pdf_value(mk(L.x, L.y, L.z), L.w, o, d);
    });
}

template <bool kRobust = false>
__device__ __forceinline__ double lights_pdf_sum(const R4<double>* __restrict__ li, uint32_t n,
                                                 V3<double> o, V3<double> d,
                                                 const R4<float>* __restrict__ li32 = nullptr) {
    const float ox = (float)o.x, oy = (float)o.y, oz = (float)o.z;
    const float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z;
    const float a = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
    const float ia = __builtin_amdgcn_rcpf(a);
    const float on = light_on(ox, oy, oz);
    const float dn = fabsf(dx) + fabsf(dy) + fabsf(dz);
    double acc = 0.0;
    for (uint32_t base = 0; base < n; base += 32) {
        const uint32_t m = min(32u, n - base);
        uint32_t mask = 0;
        for (uint32_t k = 0; k < m; ++k) {
            float cx, cy, cz, r;
            if (li32) {
                const R4<float> L = li32[base + k];
                cx = L.x;
                cy = L.y;
                cz = L.z;
                r = L.w;
            } else {
                const R4<double> L = li[base + k];
                cx = (float)L.x;
                cy = (float)L.y;
                cz = (float)L.z;
                r = fabsf((float)L.w);
            }
            mask |= (light_may_hit(cx, cy, cz, r, ox, oy, oz, dx, dy, dz, ia, on, dn) ? 1u : 0u) << k;
        }
        while (mask) {
            const uint32_t k = (uint32_t)__builtin_ctz(mask);
            mask &= mask - 1u;
            const R4<double> L = li[base + k];
            acc = acc + sphere_pdf_value(mk(L.x, L.y, L.z), L.w, o, d);
        }
    }
    return acc;
}

// f32 light test: does the ray hit the light sphere with t in [0, inf)?  The
// closest-approach offset l (see sphere_u) gives disc > 0 <=> l.l < r^2
// without cancellation; the far root is >= 0 exactly when tc >= 0 or the
// origin is inside (|f|^2 <= r^2).
template <bool kRobust>
__device__ __forceinline__ bool light_hit_f32(const R4<float>& L, V3<float> o, V3<float> d, float a, float ia) {
    const float fx = o.x - L.x, fy = o.y - L.y, fz = o.z - L.z;
    const float hb = __builtin_fmaf(d.z, fz, __builtin_fmaf(d.y, fy, d.x * fx));
    const float r2 = L.w * L.w;
    if constexpr (kRobust) {
        const float tc = -hb * ia;
        const float lx = __builtin_fmaf(tc, d.x, fx), ly = __builtin_fmaf(tc, d.y, fy),
                    lz = __builtin_fmaf(tc, d.z, fz);
        const float l2 = __builtin_fmaf(lx, lx, __builtin_fmaf(ly, ly, lz * lz));
        const float f2 = __builtin_fmaf(fx, fx, __builtin_fmaf(fy, fy, fz * fz));
        return (l2 < r2) & ((hb <= 0.f) | (f2 <= r2));
    } else {
        // disc = hb^2 - a c > 0 with c = f.f - r^2
        const float c = __builtin_fmaf(fx, fx, __builtin_fmaf(fy, fy, __builtin_fmaf(fz, fz, -r2)));
        const float disc = __builtin_fmaf(hb, hb, -(a * c));
        return (disc > 0.f) & ((hb <= 0.f) | (c <= 0.f));
    }
}
// its solid-angle pdf, 1 / (2 pi (1 - cos_max)) with 1 - cos_max = x / (1 +
// sqrt(1 - x)), x = r^2/d^2 (no cancellation for far lights)
__device__ __forceinline__ float light_pdf_f32(const R4<float>& L, V3<float> o) {
    const float cx = L.x - o.x, cy = L.y - o.y, cz = L.z - o.z;
    const float dist2 = __builtin_fmaf(cx, cx, __builtin_fmaf(cy, cy, cz * cz));
    const float x = L.w * L.w * __builtin_amdgcn_rcpf(dist2);
    const float one_minus_cos = x * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_sqrtf(1.f - x));
    return __builtin_amdgcn_rcpf(6.283185307179586f * one_minus_cos);
}
// f32: pass 1 finds the lights the ray hits (light_hit_f32, no square root) -- with
// disc > 0 the far root (-hb + sqrt(disc)) / a is >= 0 exactly when hb <= 0
// or c <= 0 -- into a bit mask; pass 2 adds the hit lights' solid-angle pdfs
// in list order.  Most rays hit zero or one light.
template <bool kRobust>
__device__ __forceinline__ float lights_pdf_sum(const R4<float>* __restrict__ li, uint32_t n,
                                                V3<float> o, V3<float> d) {
    const float a = len2_f32(d);
    const float ia = __builtin_amdgcn_rcpf(a);
    float acc = 0.f;
    for (uint32_t base = 0; base < n; base += 32) {
        const uint32_t m = min(32u, n - base);
        uint32_t mask = 0;
#pragma unroll 4
        for (uint32_t k = 0; k < m; ++k) {
            const R4<float> L = li[base + k];
            const bool hit = light_hit_f32<kRobust>(L, o, d, a, ia);
            mask |= (hit ? 1u : 0u) << k;
        }
        while (mask) {
            const uint32_t k = (uint32_t)__builtin_ctz(mask);
            mask &= mask - 1u;
            const R4<float> L = li[base + k];
            acc += light_pdf_f32(L, o);
        }
    }
    return acc;
}

// The same with pass 1 on packed FP32 (v_pk_fma/mul/add_f32: two lights per
// instruction).  lp = the light list as pairs, two R4 per pair {x0, x1, y0,
// y1}, {z0, z1, r0^2, r1^2} (an odd list ends with r^2 = -inf: never hit),
// staged in LDS; each packed lane does exactly light_hit_f32's operations, so
// the mask -- and the sum -- are bit-identical to lights_pdf_sum.
typedef float f2v __attribute__((ext_vector_type(2)));
// `sampled` (>= 0): the light the direction was drawn toward (Sphere::random,
// sphere.rs:113-127) counts whatever the f32 test says: the direction lies in
// its cone, so the reference's f64 test hits it (but at an ulp of the cone's
// edge), while the f32 discriminant can lose the grazing edge directions --
// and a lost light there turns the bounce's pdf to 0 and its weight to 0 / 0
// when the light is below the surface (r04: the f32 mode's surplus NaN
// samples on spheres that overlap no light, tools/nan_origins.py).
template <bool kRobust>
__device__ __forceinline__ float lights_pdf_sum_pk(const R4<float>* __restrict__ li,
                                                   const R4<float>* __restrict__ lp, uint32_t n,
                                                   V3<float> o, V3<float> d, int32_t sampled = -1) {
    const float a = len2_f32(d);
    const float ia = __builtin_amdgcn_rcpf(a);
    const f2v ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z};
    const f2v dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z};
    const f2v a2 = {a, a}, ia2 = {ia, ia};
    float acc = 0.f;
    for (uint32_t base = 0; base < n; base += 32) {
        const uint32_t m = min(32u, n - base);
        uint32_t mask = 0;
#pragma unroll 2
        for (uint32_t k = 0; k < m; k += 2) {
            const R4<float> A = lp[base + k], B = lp[base + k + 1];
            const f2v fx = ox - f2v{A.x, A.y}, fy = oy - f2v{A.z, A.w}, fz = oz - f2v{B.x, B.y};
            const f2v r2 = {B.z, B.w};
            const f2v hb = __builtin_elementwise_fma(dz, fz, __builtin_elementwise_fma(dy, fy, dx * fx));
            bool h0, h1;
            if constexpr (kRobust) {
                const f2v tc = -hb * ia2;
                const f2v lx = __builtin_elementwise_fma(tc, dx, fx), ly = __builtin_elementwise_fma(tc, dy, fy),
                          lz = __builtin_elementwise_fma(tc, dz, fz);
                const f2v l2 = __builtin_elementwise_fma(lx, lx, __builtin_elementwise_fma(ly, ly, lz * lz));
                const f2v f2 = __builtin_elementwise_fma(fx, fx, __builtin_elementwise_fma(fy, fy, fz * fz));
                h0 = (l2.x < r2.x) & ((hb.x <= 0.f) | (f2.x <= r2.x));
                h1 = (l2.y < r2.y) & ((hb.y <= 0.f) | (f2.y <= r2.y));
            } else {
                const f2v c = __builtin_elementwise_fma(fx, fx, __builtin_elementwise_fma(fy, fy,
                                                                __builtin_elementwise_fma(fz, fz, -r2)));
                const f2v disc = __builtin_elementwise_fma(hb, hb, -(a2 * c));
                h0 = (disc.x > 0.f) & ((hb.x <= 0.f) | (c.x <= 0.f));
                h1 = (disc.y > 0.f) & ((hb.y <= 0.f) | (c.y <= 0.f));
            }
            mask |= ((h0 ? 1u : 0u) | (h1 ? 2u : 0u)) << k;
        }
        if ((uint32_t)(sampled - (int32_t)base) < 32u) mask |= 1u << (sampled - (int32_t)base);
        while (mask) {
            const uint32_t k = (uint32_t)__builtin_ctz(mask);
            mask &= mask - 1u;
            const R4<float> L = li[base + k];
            acc += light_pdf_f32(L, o);
        }
    }
    return acc;
}

// Light pdf through the light BVH (KParams::light_bvh): every light sphere the
// ray (o, d) hits with t in [0, inf] contributes its solid-angle pdf
// (HittableList::pdf_value, hittable_list.rs:408-412; sphere.rs:101-111).
// Boxes only cull.  The traversal reuses the lane's LDS stack.
//
// Both children of a node are slab-tested against [0, inf); the visit order
// does not matter for an all-hits query.
// Light-pdf work of one lane, counted into KParams::counters[7] / [8]: light
// tests (every light of the big list, a visited grid cell or a light-BVH leaf
// that the ray is tested against) and light-grid cells visited.
struct LightWork {
    uint32_t tests = 0, cells = 0;
};
// ... added to the wave's u64 counters in LDS (w[0] tests, w[1] cells): from
// any subset of lanes (LDS atomics), or from the whole converged wave (one sum)
__device__ __forceinline__ void light_work_lane(unsigned long long* w, const LightWork& lw) {
    if (lw.tests) atomicAdd(w, (unsigned long long)lw.tests);
    if (lw.cells) atomicAdd(w + 1, (unsigned long long)lw.cells);
}
__device__ __forceinline__ void light_work_wave(unsigned long long* w, LightWork lw, uint32_t lane) {
    uint32_t t = lw.tests, c = lw.cells;
    for (int off = 32; off > 0; off >>= 1) {
        t += (uint32_t)__shfl_xor((int)t, off);
        c += (uint32_t)__shfl_xor((int)c, off);
    }
    if (lane == 0) {
        w[0] += t;
        w[1] += c;
    }
}

template <typename R, typename Leaf>
__device__ __forceinline__ void light_bvh_walk(const DevScene<R>& sc, V3<R> o, V3<R> d,
                                               int32_t* __restrict__ stk, Leaf&& leaf) {
    R ix, iy, iz, oix, oiy, oiz;
    slab_axis(o.x, d.x, ix, oix);
    slab_axis(o.y, d.y, iy, oiy);
    slab_axis(o.z, d.z, iz, oiz);
    int32_t sp = 0;
    int32_t node = 0;
    for (;;) {
        if (node >= 0) {
            const BvhNode<R>& nd = sc.lbvh[node];
            bool h[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const R x0 = nd.lo_x[c] * ix - oix, x1 = nd.hi_x[c] * ix - oix;
                const R y0 = nd.lo_y[c] * iy - oiy, y1 = nd.hi_y[c] * iy - oiy;
                const R z0 = nd.lo_z[c] * iz - oiz, z1 = nd.hi_z[c] * iz - oiz;
                const R tn = fmax(fmax(fmin(x0, x1), fmin(y0, y1)), fmax(fmin(z0, z1), (R)0));
                const R tf = fmin(fmax(x0, x1), fmin(fmax(y0, y1), fmax(z0, z1)));
                h[c] = tn <= tf;
            }
            const int32_t c0 = nd.child[0], c1 = nd.child[1];
            if (h[0] && h[1]) {
                stk[sp * 64] = c1;
                ++sp;
                node = c0;
                continue;
            }
            if (h[0] | h[1]) {
                node = h[0] ? c0 : c1;
                continue;
            }
        } else {
            const uint32_t code = (uint32_t)~node;
            const uint32_t first = code >> 4, cnt = code & 15u;
            for (uint32_t k = 0; k < cnt; ++k) leaf(first + k);
        }
        if (sp == 0) break;
        --sp;
        node = stk[sp * 64];
    }
}

// f32: light_hit_f32 / light_pdf_f32 as in lights_pdf_sum; pdfs summed in walk order.
template <bool kRobust>
__device__ __forceinline__ float lights_pdf_bvh(const DevScene<float>& sc, V3<float> o, V3<float> d,
                                                int32_t* __restrict__ stk, LightWork& lw) {
    const float a = len2_f32(d);
    const float ia = __builtin_amdgcn_rcpf(a);
    float acc = 0.f;
    light_bvh_walk(sc, o, d, stk, [&](uint32_t k) {
        ++lw.tests;
        const R4<float> L = sc.lsph[k];
        const bool hit = light_hit_f32<kRobust>(L, o, d, a, ia);
        if (hit) acc += light_pdf_f32(L, o);
    });
    return acc;
}
// f64 (parity mode): collect the hit lights' list indices, then sum their
// pdfs in LIST order with the reference arithmetic -- bit-identical to the
// linear sum (misses add +0.0, which changes nothing).  More than 8 hits
// falls back to the linear loop.
template <bool kRobust>
__device__ __forceinline__ double lights_pdf_bvh(const DevScene<double>& sc, V3<double> o, V3<double> d,
                                                 int32_t* __restrict__ stk, LightWork& lw) {
    const LightPre pre(o, d);
    return lights_sum_in_list_order(sc.lights, o, d, [&](auto&& add) {
        light_bvh_walk(sc, o, d, stk, [&](uint32_t k) {
            ++lw.tests;
            const R4<double> L = sc.lsph[k];
            double t;
            if (pre.may_hit(L) && sphere_t(mk(L.x, L.y, L.z), L.w * L.w, o, d, 0.0, t)) add(sc.lid[k]);
        });
    });
}

// f32: the big list, then the walk; a light counts in the cell whose interval
// holds its closest-approach parameter tc = -(d . (o - c)) / (d . d)
template <bool kRobust>
__device__ __forceinline__ float lights_pdf_grid(const DevScene<float>& sc, V3<float> o, V3<float> d,
                                                 LightWork& lw) {
    const float a = len2_f32(d);
    const float ia = __builtin_amdgcn_rcpf(a);
    float acc = 0.f;
    lw.tests += sc.lg_big;
    for (uint32_t k = 0; k < sc.lg_big; ++k) {
        const R4<float> L = sc.lg_sph[k];
        if (light_hit_f32<kRobust>(L, o, d, a, ia)) acc += light_pdf_f32(L, o);
    }
    light_grid_walk(sc, o, d, [&](uint32_t k, float te, float tx) {
        ++lw.tests;
        const R4<float> L = sc.lg_sph[k];
        const float fx = o.x - L.x, fy = o.y - L.y, fz = o.z - L.z;
        const float tc = -__builtin_fmaf(d.z, fz, __builtin_fmaf(d.y, fy, d.x * fx)) * ia;
        if (light_hit_f32<kRobust>(L, o, d, a, ia) & (tc >= te) & (tc < tx)) acc += light_pdf_f32(L, o);
    }, &lw.cells);
    return acc;
}
// lights_pdf_grid by the whole wave (f32, KParams::grid_piece = P > 0).  A ray
// that skims a flat light layer walks the grid's whole width (C5: a ground
// point sampling one of 50k lights at the same height, ~150 cells of ~4 lights
// each) while most rays walk a few cells, and a lane-per-ray walk keeps its
// wave for the longest one (C5: 10 % of lanes active).  Here every lane of
// the wave walks for the pending rays (`pend`; the ray is (o, d)): each ray's
// grid interval [tn, tf] is cut into k = ceil(cells / P) pieces of equal
// length in t, the pieces of all rays are dealt to the 64 lanes round by
// round, every piece's pdf sum lands in an LDS slot, and each ray's owner
// adds its pieces up in order.  The cut depends on the ray and P alone and
// the sum runs in piece order, so the result does not depend on which rays
// share the wave; the first piece starts from the big list's sum, so a
// one-piece ray (most of them) sums exactly as lights_pdf_grid.  `slots`:
// `cap` (a multiple of 64) floats of the wave's LDS; every lane of the wave
// calls this (converged), with wave-uniform P.
template <bool kRobust, typename Mark>
__device__ __forceinline__ float lights_pdf_grid_coop(const DevScene<float>& sc, bool pend, V3<float> o, V3<float> d,
                                                   uint32_t P, float* __restrict__ slots, uint32_t cap,
                                                   uint32_t lane, LightWork& lw, Mark&& mark) {
    float acc = 0.f, tn = 0.f, tf = 0.f;
    uint32_t k = 0;
    if (pend) {
        const float a = len2_f32(d);
        const float ia = __builtin_amdgcn_rcpf(a);
        lw.tests += sc.lg_big;
        for (uint32_t q = 0; q < sc.lg_big; ++q) {
            const R4<float> L = sc.lg_sph[q];
            if (light_hit_f32<kRobust>(L, o, d, a, ia)) acc += light_pdf_f32(L, o);
        }
        uint32_t cells = 0;
        if (light_grid_span(sc, o, d, grid_inv(d.x), grid_inv(d.y), grid_inv(d.z), tn, tf, cells))
            k = (cells + P - 1u) / P;
    }
    // first piece of each ray: exclusive prefix of k over the lanes
    uint32_t incl = k;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off);
        if (lane >= off) incl += v;
    }
    const uint32_t first = incl - k, total = (uint32_t)__shfl((int)incl, 63);
    mark(13);
    for (uint32_t b = 0; b < total; b += cap) {
        const uint32_t e = min(b + cap, total);
        for (uint32_t r = b; r < e; r += 64) {
            const uint32_t g = r + lane;
            // the piece's ray: the last lane whose first piece is <= g
            uint32_t own = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1) {
                const uint32_t f = (uint32_t)__shfl((int)first, (int)(own + step));
                own = f <= g ? own + step : own;
            }
            const V3<float> ro = mk(bperm_f(o.x, own), bperm_f(o.y, own), bperm_f(o.z, own));
            const V3<float> rd = mk(bperm_f(d.x, own), bperm_f(d.y, own), bperm_f(d.z, own));
            const float rtn = bperm_f(tn, own), rtf = bperm_f(tf, own), racc = bperm_f(acc, own);
            const uint32_t rk = (uint32_t)bperm_i((int32_t)k, own), rfirst = (uint32_t)bperm_i((int32_t)first, own);
            if (g < e) {
                const uint32_t j = g - rfirst;
                const float step = (rtf - rtn) / (float)rk;
                auto t_at = [&](uint32_t q) { return q == 0 ? rtn : __builtin_fmaf((float)q, step, rtn); };
                const float ra = len2_f32(rd);
                const float ria = __builtin_amdgcn_rcpf(ra);
                float part = j == 0 ? racc : 0.f;
                auto test = [&](const R4<float>& L, float te, float tx) {
                    const float fx = ro.x - L.x, fy = ro.y - L.y, fz = ro.z - L.z;
                    const float tc = -__builtin_fmaf(rd.z, fz, __builtin_fmaf(rd.y, fy, rd.x * fx)) * ria;
                    if (light_hit_f32<kRobust>(L, ro, rd, ra, ria) & (tc >= te) & (tc < tx))
                        part += light_pdf_f32(L, ro);
                };
                // the cell records (DevScene::lg_rec): one 64-byte load per cell,
                // not the cell's range and then each light
                RTW_PROBE_LANES(11);
                light_grid_walk_piece_rec(sc, sc.lg_rec, sc.lg_sph, ro, rd, grid_inv(rd.x), grid_inv(rd.y),
                                          grid_inv(rd.z), t_at(j), t_at(j + 1), j == 0, j + 1 == rk,
                                          [&](const R4<float>& L, auto&&, float te, float tx) {
                                              RTW_PROBE_LANES(12);
                                              test(L, te, tx);
                                          }, &lw.cells, &lw.tests);
                slots[g - b] = part;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        mark(14);
        if (k) {
            const uint32_t g0 = max(first, b), g1 = min(first + k, e);
            for (uint32_t g = g0; g < g1; ++g) acc = g == first ? slots[g - b] : acc + slots[g - b];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        mark(15);
    }
    return acc;
}

// f64 (parity mode): the hit lights' list indices, summed in LIST order
// (lights_sum_in_list_order) as in lights_pdf_bvh.
template <bool kRobust>
__device__ __forceinline__ double lights_pdf_grid(const DevScene<double>& sc, V3<double> o, V3<double> d,
                                                  LightWork& lw) {
    const LightPre pre(o, d);   // the f32 pre-pass rules out the lights the ray misses
    const double ia = 1.0 / (d.x * d.x + d.y * d.y + d.z * d.z);
    return lights_sum_in_list_order(sc.lights, o, d, [&](auto&& add) {
        lw.tests += sc.lg_big;
        for (uint32_t k = 0; k < sc.lg_big; ++k) {
            const R4<double> L = sc.lg_sph[k];
            double t;
            if (pre.may_hit(L) && sphere_t(mk(L.x, L.y, L.z), L.w * L.w, o, d, 0.0, t)) add(sc.lg_id[k]);
        }
        light_grid_walk(sc, o, d, [&](uint32_t k, double te, double tx) {
            ++lw.tests;
            const R4<double> L = sc.lg_sph[k];
            double t;
            if (pre.may_hit(L) && sphere_t(mk(L.x, L.y, L.z), L.w * L.w, o, d, 0.0, t)) {
                const double tc = -((o.x - L.x) * d.x + (o.y - L.y) * d.y + (o.z - L.z) * d.z) * ia;
                if (tc >= te && tc < tx) add(sc.lg_id[k]);
            }
        }, &lw.cells);
    });
}

// lights_pdf_grid (f64) by the whole wave.  The sum needs the SET of lights
// the f64 test hits, summed in LIST order; which structure finds them is free.
// So the walk runs in f32 -- the f32 kernels' piece cut (lights_pdf_grid_coop:
// each pending ray's grid interval cut into k = ceil(cells / P) pieces of
// equal length in t, dealt to the 64 lanes), on the f32 copy of the grid
// (DevScene::lg_sph32 and the grid box rounded to f32) -- and a light of a
// visited cell is a candidate when the f64 path's f32 pre-pass (LightPre /
// light_may_hit: slack far above the f32 error) says the ray may hit it and
// its f32 closest-approach parameter falls in the cell's interval: every light
// the f64 test hits is a candidate exactly once (the intervals partition the
// line; the host pads the cells' lists beyond the f32 rounding).  The owner
// sums Sphere::pdf_value over its candidates in list order, in f64 (a
// candidate the f64 test misses adds +0.0: no bit changes).  In passes over
// list indices >= lo: a piece keeps the kPieceIds smallest candidate indices
// >= lo it finds, sorted, in its LDS slot ([count, ids]); each owner merges
// its pieces' indices and the big list's into its kMax smallest; every index
// up to `bound` -- the largest kept index of a piece or an owner list that
// had to drop some, else unbounded -- is then known, so the owner sums those
// and, when something was dropped, the wave walks again for its rays with
// lo = bound + 1 (each pass sums at least one index: the walk always ends).
// Bit-identical to lights_pdf_grid and the linear list-order sum.  (Round 4
// walked in f64 -- f64 DDA, f64 records, the f64 test in the piece: C3 / C5
// spilled the path state at every trip.)  Every lane of the wave calls this
// (converged), with wave-uniform P; `cap_words` (a multiple of 64) of LDS at
// `slots`.
// The pending f64 ray (o, d) is read from the wave's LDS stash (`ray`: words
// [(2k) 64 + lane], [(2k + 1) 64 + lane] for k = 0..5, the kernel's layout)
// where it is needed -- the f32 ray at the start of a pass, the pdfs at its
// end -- so it is not held in registers across the walk's rounds.
// The light grid of an f64 scene as the f32 walk reads it: the arrays, and
// the grid box, cells and their counts rounded to f32.
struct Grid64 {
    const uint32_t* lg_start;
    const R4<float>* lg_rec;          // the cell records (f32 lights: lg_sph32's values)
    const R4<float>* lg_sph32;        // DevScene<double>::lg_sph32
    const uint32_t* lg_id;
    const R4<double>* lights;         // the light list (f64 records: the pdfs)
    float lo[3], hi[3], cell[3], inv[3];
    uint32_t n[3], big;
};
// The cooperative walk with the list-order sum, both precisions (R: the sum).
// `g`: the grid as the f32 walk reads it (lg_start, lg_sph, box, cells);
// `rec` its cell records, `lg_id` the items' list indices, `big` the big
// list's length; (of, df) the pending ray in f32 and ia_own = 1 / (df . df)
// as the owner's tests compute it.  cand(L, ro, rd, ra, ria, ron, rdn): may
// the ray hit light L (a piece's test; the owner's ray bperm'd, ra = its
// len2_f32, ron / rdn = |o|_1, |d|_1); big_hit(L): the owner's test of a big
// light; pdf_at(id, owner): light id's pdf for the ray of lane `owner`
// (evaluated by any lane: the owners' pdfs are dealt to the whole wave).
// `mark(id)`: the clock probes' section marks (RTW_CLOCK builds; else a no-op).
template <typename R, typename Cand, typename BigHit, typename PdfAt, typename Mark>
__device__ __forceinline__ R lights_pdf_grid_coop_list(const DevScene<float>& g, const R4<float>* __restrict__ rec,
                                                       const uint32_t* __restrict__ lg_id, uint32_t big, V3<float> of,
                                                       V3<float> df, float ia_own, bool pend, uint32_t P,
                                                       uint32_t* __restrict__ slots, uint32_t cap_words, uint32_t lane,
                                                       LightWork& lw, Cand&& cand, BigHit&& big_hit, PdfAt&& pdf_at,
                                                       Mark&& mark) {
    // a piece's slot: [count, ids...] padded to 8 words (the owner reads it as two
    // 16-byte LDS loads)
    constexpr uint32_t kPieceIds = kCoop64PieceIds, kSlot = kCoop64Slot, kMax = RTW_COOP64_MAX;
    const uint32_t cap = cap_words / (kSlot * 64) * 64;   // pieces per round
    constexpr uint32_t kCoopAdaptMin = 4;                 // the shortest adaptive piece (cells)
    // (the host sizes the stack area for at least one round of 64 pieces, so a
    // smaller area is a host error: every pending ray ends NaN, never a loop
    // that cannot advance)
    if (cap == 0) return pend ? (R)NAN : (R)0;
    float tn = 0.f, tf = 0.f;
    uint32_t k = 0, cells = 0;
    const bool walks = pend && light_grid_span(g, of, df, grid_inv(df.x), grid_inv(df.y), grid_inv(df.z), tn, tf, cells);
    // pieces of Q cells (wave-uniform): the sum does not depend on the cut (list
    // order), so the wave's pending cells are spread over its lanes -- one round
    // of at most 64 pieces (sum ceil(c / Q) <= C / Q + n <= 64) unless that needs
    // pieces longer than P, the longest the tuning allows (C3: ~27 short rays per
    // trip walked as ~27 one-piece rays left most lanes idle)
    uint32_t Q = P;
    uint32_t C = walks ? cells : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) C += (uint32_t)__shfl_xor((int)C, off);
    const uint32_t nr = (uint32_t)__popcll(__ballot(walks));
    if (nr < 64u) Q = min(P, max(kCoopAdaptMin, (C + (63u - nr)) / (64u - nr)));
    // at most `cap` pieces (longer pieces for a longer ray): every ray's
    // pieces fit one round, so its owner finds all of them in the slots
    if (walks) k = min((cells + Q - 1u) / Q, cap);
    const uint32_t ia_bits = __float_as_uint(ia_own);
    // the big list's candidates of the pending ray: tested once per walk, not at
    // each of the owner's merges (their loads were on the merge's critical path)
    constexpr uint32_t kBigC = 2;
    uint32_t bigc[kBigC] = {0u, 0u};
    uint32_t nbig = 0;
    bool big_over = false;
    if (pend && big) {
        lw.tests += big;
        for (uint32_t q = 0; q < big; ++q) {
            if (big_hit(g.lg_sph[q])) {
                if (nbig < kBigC) bigc[nbig++] = lg_id[q];
                else big_over = true;
            }
        }
    }
    R acc = (R)0;
    uint32_t lo = 0;
    bool more = pend;           // the ray still needs a walk (over list indices >= lo)
    while (__any(more)) {
        const uint32_t kp = more ? k : 0u;   // this walk's pieces
        uint32_t incl = kp;
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, off);
            if (lane >= off) incl += v;
        }
        const uint32_t first = incl - kp, total = (uint32_t)__shfl((int)incl, 63);
        bool walk_again = false;
        mark(13);
        // rounds of whole rays: [B, Bn) holds the pieces of the rays that start
        // at B or later and end by B + cap (a pending ray without pieces -- it
        // misses the grid -- sums its big-list candidates in the first round)
        for (uint32_t B = 0;;) {
            const bool mine = more && (kp ? first >= B && first + kp <= B + cap : B == 0);   // the ray is in the round
            const uint64_t later = __ballot(kp && first >= B && !mine);
            const uint32_t Bn = later ? (uint32_t)__shfl((int)first, (int)__builtin_ctzll(later)) : total;
            // a round of at most 64 pieces (the usual case: cap is 64 at the
            // host's minimum stack) keeps the mask of its pieces that hold a
            // candidate, so that an owner's merge reads only those slots
            const bool one_pass = Bn - B <= 64u;
            uint64_t held = ~0ull;
            for (uint32_t r = B; r < Bn; r += 64) {
                const uint32_t gi = r + lane;
                bool has = false;
                uint32_t own = 0;
#pragma unroll
                for (uint32_t step = 32; step; step >>= 1) {
                    const uint32_t f = (uint32_t)__shfl((int)first, (int)(own + step));
                    own = f <= gi ? own + step : own;
                }
                const V3<float> ro = mk(bperm_f(of.x, own), bperm_f(of.y, own), bperm_f(of.z, own));
                const V3<float> rd = mk(bperm_f(df.x, own), bperm_f(df.y, own), bperm_f(df.z, own));
                const float rtn = bperm_f(tn, own), rtf = bperm_f(tf, own);
                const uint32_t rk = (uint32_t)bperm_i((int32_t)kp, own), rfirst = (uint32_t)bperm_i((int32_t)first, own);
                const uint32_t rlo = (uint32_t)bperm_i((int32_t)lo, own);
                const float ria = __uint_as_float((uint32_t)bperm_i((int32_t)ia_bits, own));
                if (gi < Bn) {
                    const uint32_t j = gi - rfirst;
                    const float step = (rtf - rtn) / (float)rk;
                    auto t_at = [&](uint32_t q) { return q == 0 ? rtn : __builtin_fmaf((float)q, step, rtn); };
                    // the owner's test quantities, from the same f32 ray
                    const float ron = light_on(ro.x, ro.y, ro.z), rdn = fabsf(rd.x) + fabsf(rd.y) + fabsf(rd.z);
                    const float ra = len2_f32(rd);
                    uint32_t* ent = slots + (gi - B) * kSlot + 1;
                    uint32_t cnt = 0;
                    // the candidates in registers (one compare-exchange insert each), the
                    // slot written once: C5 f64 1527 -> 1460 ms, C3 1042 -> 1004 against
                    // insertion in LDS (profiles/r06m_ab_piece_reg.jsonl)
                    uint32_t pid[kPieceIds];
#pragma unroll
                    for (uint32_t q = 0; q < kPieceIds; ++q) pid[q] = 0xffffffffu;
                    // a light of the piece: a candidate (its list index kept) when the
                    // test may hit it in the cell's interval; idx(): its lg_id slot
                    auto test = [&](const R4<float>& L, auto&& idx, float te, float tx) {
                        if (cand(L, ro, rd, ra, ria, ron, rdn)) {
                            const float tc = -__builtin_fmaf(rd.z, ro.z - L.z, __builtin_fmaf(rd.y, ro.y - L.y,
                                                                                               rd.x * (ro.x - L.x))) * ria;
                            if (!(tc >= te && tc < tx)) return;
                            const uint32_t id = lg_id[idx()];
                            if (id >= rlo) {
                                // the piece's kPieceIds smallest, sorted (rare: a candidate)
                                ++cnt;
                                (void)sorted_insert(pid, id);
                            }
                        }
                    };
                    light_grid_walk_piece_rec(g, rec, g.lg_sph, ro, rd, grid_inv(rd.x), grid_inv(rd.y),
                                              grid_inv(rd.z), t_at(j), t_at(j + 1), j == 0, j + 1 == rk, test,
                                              &lw.cells, &lw.tests);
                    {
                        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
                        static_assert(kPieceIds <= 7 && kSlot == 8, "the slot as two 16-byte stores");
                        uint32_t w[7];
#pragma unroll
                        for (uint32_t q = 0; q < 7; ++q) w[q] = q < kPieceIds ? pid[q < kPieceIds ? q : 0] : 0xffffffffu;
                        u4* sl = reinterpret_cast<u4*>(ent - 1);
                        sl[0] = u4{cnt, w[0], w[1], w[2]};
                        sl[1] = u4{w[3], w[4], w[5], w[6]};
                    }
                    has = cnt != 0;
                }
                const uint64_t h = __ballot(has);
                if (one_pass) held = h;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            mark(14);
            // every candidate >= lo of this ray is in its pieces' slots (and the
            // big list) unless a piece kept only its kPieceIds smallest: its owner
            // merges the kMax smallest, sums them in list order, and merges again
            // above the last one summed until done -- or until a piece's dropped
            // candidates are needed, which takes another walk.  The
            // owners' merges run together and the pdfs of all their summable ids
            // are dealt to the wave's lanes (pdf_at(id, owner): any lane evaluates
            // a candidate for the owner's ray); each owner then adds its values
            // in list order, fetched by ds_bpermute -- the sum of each ray is the
            // same, its pdfs no longer computed by its owner lane alone
            bool owning = mine;
            while (__any(owning)) {
                uint32_t ids[kMax];
#pragma unroll
                for (uint32_t q = 0; q < kMax; ++q) ids[q] = 0xffffffffu;
                uint32_t n = 0, bp = 0xffffffffu, bound = 0xffffffffu;   // bp: below a piece's dropped candidates
                if (owning) {
                    RTW_PROBE_LANES(13);
                    bool dropped = false;
                    auto add = [&](uint32_t id) {   // the kMax smallest list indices (lights_sum_in_list_order)
                        if (sorted_insert(ids, id) != 0xffffffffu) dropped = true;
                    };
                    // the big list's candidates, tested once per walk (bigc below)
                    if (!big_over) {
                        for (uint32_t q = 0; q < nbig; ++q)
                            if (bigc[q] >= lo) add(bigc[q]);
                    } else {
                        for (uint32_t q = 0; q < big; ++q) {
                            const uint32_t id = lg_id[q];
                            if (id >= lo && big_hit(g.lg_sph[q])) add(id);
                        }
                    }
                    auto merge_piece = [&](uint32_t gi) {
                        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
                        const u4* sl = reinterpret_cast<const u4*>(slots + (gi - B) * kSlot);
                        RTW_PROBE_LANES(14);
                        const u4 w0 = sl[0], w1 = sl[1];
                        const uint32_t cnt = w0.x;
                        const uint32_t e[7] = {w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                        for (uint32_t q = 0; q < kPieceIds; ++q)
                            if (q < cnt && e[q] >= lo) add(e[q]);
                        if (cnt > kPieceIds) bp = min(bp, e[kPieceIds - 1]);
                    };
                    if (one_pass) {
                        // only the ray's pieces with a candidate (first - B + kp <= 64)
                        uint64_t m = kp ? held >> (first - B) : 0ull;
                        if (kp < 64u) m &= (1ull << kp) - 1ull;
                        for (; m; m &= m - 1ull) merge_piece(first + (uint32_t)__builtin_ctzll(m));
                    } else {
                        for (uint32_t gi = first; gi < first + kp; ++gi) merge_piece(gi);
                    }
                    bound = dropped ? min(bp, ids[kMax - 1]) : bp;
#pragma unroll
                    for (uint32_t q = 0; q < kMax; ++q) n += ids[q] != 0xffffffffu ? 1u : 0u;
                }
                mark(16);
                // the owner's summable ids: ids[0..m) (sorted, <= bound)
                uint32_t m = 0;
                if (owning) {
#pragma unroll
                    for (uint32_t q = 0; q < kMax; ++q) m += (q < n && ids[q] <= bound) ? 1u : 0u;
                }
                uint32_t incl_m = m;
#pragma unroll
                for (uint32_t off = 1; off < 64; off <<= 1) {
                    const uint32_t v = (uint32_t)__shfl_up((int)incl_m, off);
                    if (lane >= off) incl_m += v;
                }
                const uint32_t fm = incl_m - m, T = (uint32_t)__shfl((int)incl_m, 63);
                for (uint32_t r = 0; r < T; r += 64) {
                    const uint32_t gi = r + lane;
                    uint32_t own = 0;   // the owner of candidate gi: the last lane whose first is <= gi
#pragma unroll
                    for (uint32_t step = 32; step; step >>= 1) {
                        const uint32_t f = (uint32_t)__shfl((int)fm, (int)(own + step));
                        own = f <= gi ? own + step : own;
                    }
                    const uint32_t q = gi - (uint32_t)__shfl((int)fm, (int)own);
                    uint32_t id = 0;
#pragma unroll
                    for (uint32_t k2 = 0; k2 < kMax; ++k2) {
                        const uint32_t v = (uint32_t)bperm_i((int32_t)(k2 < n ? ids[k2] : 0u), (int32_t)own);
                        id = k2 == q ? v : id;
                    }
                    RTW_PROBE_LANES(15);
                    const R val = gi < T ? pdf_at(id, own) : (R)0;
                    // each owner adds its values of this pass, in list order
                    const uint32_t g0 = max(fm, r), g1 = min(fm + m, r + 64u);   // its candidates in this pass
                    const uint32_t q0 = g0 - r, cnt = g1 > g0 ? g1 - g0 : 0u;
                    uint32_t cmax = cnt;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) cmax = max(cmax, (uint32_t)__shfl_xor((int)cmax, off));
                    for (uint32_t jq = 0; jq < cmax; ++jq) {
                        const R v = bperm_any(val, (int32_t)((q0 + jq) & 63u));
                        if (jq < cnt) acc = acc + v;
                    }
                }
                mark(15);
                if (owning) {
                    if (bound == 0xffffffffu) {
                        more = false;                       // every candidate summed
                        owning = false;
                    } else {
                        lo = bound + 1u;
                        if (bound == bp) {                  // a piece's dropped candidates are next
                            walk_again = true;
                            owning = false;
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            mark(15);
            B = Bn;
            if (B >= total) break;
        }
        more = more && walk_again;
    }
    return acc;
}


// the f64 instance: candidates by the f64 path's f32 pre-pass (light_may_hit),
// the pdfs in f64 from the pending ray in the wave's LDS stash
template <typename Mark>
__device__ __forceinline__ double lights_pdf_grid_coop64(const Grid64& sc, bool pend,
                                                         const uint32_t* __restrict__ ray, uint32_t P,
                                                         uint32_t* __restrict__ slots, uint32_t cap_words,
                                                         uint32_t lane, LightWork& lw, Mark&& mark) {
    auto ray_at = [&](uint32_t q) {
        return __longlong_as_double((long long)((uint64_t)ray[(2 * q) * 64 + lane] |
                                                ((uint64_t)ray[(2 * q + 1) * 64 + lane] << 32)));
    };
    auto ray_o = [&]() { return mk(ray_at(0), ray_at(1), ray_at(2)); };
    auto ray_d = [&]() { return mk(ray_at(3), ray_at(4), ray_at(5)); };
    // the grid as a DevScene<float> (only the fields the walk reads)
    DevScene<float> g;
    g.lg_start = sc.lg_start;
    g.lg_sph = sc.lg_sph32;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g.lg_lo[a] = sc.lo[a];
        g.lg_hi[a] = sc.hi[a];
        g.lg_cell[a] = sc.cell[a];
        g.lg_inv[a] = sc.inv[a];
        g.lg_n[a] = sc.n[a];
    }
    V3<float> of, df;           // the f32 ray
    {
        const LightPre pre(ray_o(), ray_d());
        of = mk(pre.ox, pre.oy, pre.oz);
        df = mk(pre.dx, pre.dy, pre.dz);
    }
    const float ia = __builtin_amdgcn_rcpf(__builtin_fmaf(df.x, df.x, __builtin_fmaf(df.y, df.y, df.z * df.z)));
    auto cand = [&](const R4<float>& L, V3<float> ro, V3<float> rd, float, float ria, float ron, float rdn) {
        return light_may_hit(L.x, L.y, L.z, L.w, ro.x, ro.y, ro.z, rd.x, rd.y, rd.z, ria, ron, rdn);
    };
    auto big_hit = [&](const R4<float>& L) {
        const float ib = __builtin_amdgcn_rcpf(__builtin_fmaf(df.x, df.x, __builtin_fmaf(df.y, df.y, df.z * df.z)));
        const float on = light_on(of.x, of.y, of.z), dn = fabsf(df.x) + fabsf(df.y) + fabsf(df.z);
        return light_may_hit(L.x, L.y, L.z, L.w, of.x, of.y, of.z, df.x, df.y, df.z, ib, on, dn);
    };
    auto pdf_at = [&](uint32_t id, uint32_t owner) {   // the owner's f64 ray from its stash column
        auto at = [&](uint32_t q) {
            return __longlong_as_double((long long)((uint64_t)ray[(2 * q) * 64 + owner] |
                                                    ((uint64_t)ray[(2 * q + 1) * 64 + owner] << 32)));
        };
        const R4<double> L = sc.lights[id];
        return sphere_pdf_value(mk(L.x, L.y, L.z), L.w, mk(at(0), at(1), at(2)), mk(at(3), at(4), at(5)));
    };
    return lights_pdf_grid_coop_list<double>(g, sc.lg_rec, sc.lg_id, sc.big, of, df, ia, pend, P, slots, cap_words,
                                             lane, lw, cand, big_hit, pdf_at, mark);
}

// Light list with quads (DevScene::lref set): HittableList::pdf_value over
// the mixed list in list order (hittable_list.rs:408-412), reference
// arithmetic per entry; `li` = the sphere lights (LDS-staged or global).
template <typename R>
__device__ __forceinline__ R lights_pdf_mixed(const DevScene<R>& sc, const R4<R>* __restrict__ li, V3<R> o,
                                              V3<R> d) {
    R acc = (R)0;
    for (uint32_t k = 0; k < sc.n_list; ++k) {
        const uint32_t ref = sc.lref[k];
        if (ref & kLrefQuad) {
            acc = acc + quad_pdf_value(sc.lquads + kQuadR * (ref & 0x3fffffffu), o, d);
        } else if (ref & kLrefDefault) {
            acc = acc + (R)0;                      // Hittable::pdf_value default, hittable.rs:175-177
        } else {
            const R4<R> L = li[ref];
            acc = acc + sphere_pdf_value(mk(L.x, L.y, L.z), L.w, o, d);
        }
    }
    return acc;
}

}  // namespace dev

}  // namespace rtw
