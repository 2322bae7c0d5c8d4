// bvh_traverse.hpp -- the closest-hit query of the BVH render kernels: the
// per-sphere testers, the binary (single-loop, while-while, with subtree
// stealing) and 4-wide traversals, and the bvh_closest* entry points the
// kernel body calls.  Also the wave helpers (bperm_*) and the f32 sphere test
// (sphere_u) that the light pdf and the brute-force sweep share with it.
#pragma once

#include "rtw_device.hpp"
#include "rtw_kernels.h"

namespace rtw {

namespace dev {

// Experiment hooks: every RTW_PROBE_* below expands to nothing in the product
// build; rtw_probes.hpp defines them for the profiling builds of
// tools/exp_cost.sh (RTW_EXP), tools/trace_paths.py (RTW_TRACE),
// tools/lane_profile.py (RTW_PROF) and tools/clock_profile.py (RTW_CLOCK).
#include "rtw_probes.hpp"

// f32 (speed mode): the per-sphere test, shared by the brute-force sweep and
// the BVH leaves so both give bit-identical t; every FMA is spelled out so
// that contraction cannot differ between the two call sites.
//
// Closest-approach form (Haines et al., "Precision Improvements for Ray/Sphere
// Intersection", Ray Tracing Gems ch. 7): with f = o - c, the ray's closest
// point to the centre is at tc = -(f.d)/a and l = f + tc d is the offset from
// the centre to it; the discriminant is a (r^2 - l.l).  The reference's
// hb^2 - a c cancels catastrophically in f32 once |f| >> r (C5's 1M-sphere
// field seen from ~700 units: the error exceeds r^2 itself); l.l does not.
// Roots t = tc -/+ sqrt((r^2 - l.l) / a).  Scenes whose extent is small next
// to their radii (C2) keep the cheaper reference form (DevScene::robust = 0,
// chosen per launch by the host).  The range test "t in [tmin, tb)"
// is ONE unsigned compare on u = bits(t) - bits(tmin): for t >= 0 float bits
// are monotonic, while every t < tmin (negative, or in [0, tmin)) and NaN
// maps above bits(+inf) - bits(tmin) >= any live bound.  Since t0 <= t1,
// min_u32(u0, u1) is the near root when it is >= tmin, else the far root
// (sphere.rs:71-80).  A miss gives sqrt(negative) = NaN and so no hit.
template <bool kRobust>
__device__ __forceinline__ uint32_t sphere_u(const R4<float>& s, V3<float> o, V3<float> d, float a,
                                             float ia, uint32_t tminb) {
    const float fx = o.x - s.x, fy = o.y - s.y, fz = o.z - s.z;
    const float hb = __builtin_fmaf(d.z, fz, __builtin_fmaf(d.y, fy, d.x * fx));
    float t0, t1;
    if constexpr (kRobust) {
        const float tc = -hb * ia;
        const float lx = __builtin_fmaf(tc, d.x, fx), ly = __builtin_fmaf(tc, d.y, fy),
                    lz = __builtin_fmaf(tc, d.z, fz);
        const float l2 = __builtin_fmaf(lx, lx, __builtin_fmaf(ly, ly, lz * lz));
        const float h = __builtin_amdgcn_sqrtf((s.w - l2) * ia);   // NaN on a miss
        t0 = tc - h;
        t1 = tc + h;
    } else {
        // the reference's form: c = f.f - r^2, disc = hb^2 - a c
        const float c = __builtin_fmaf(fx, fx, __builtin_fmaf(fy, fy, __builtin_fmaf(fz, fz, -s.w)));
        const float disc = __builtin_fmaf(hb, hb, -(a * c));
        const float sq = __builtin_amdgcn_sqrtf(disc);             // NaN on a miss
        const float nb = -hb * ia;
        t0 = __builtin_fmaf(-sq, ia, nb);
        t1 = __builtin_fmaf(sq, ia, nb);
    }
    return min(__float_as_uint(t0) - tminb, __float_as_uint(t1) - tminb);
}
__device__ __forceinline__ float len2_f32(V3<float> d) {
    return __builtin_fmaf(d.z, d.z, __builtin_fmaf(d.y, d.y, d.x * d.x));
}

// ---------------------------------------------------------------------------
// BVH closest hit (RTW_ACCEL_BVH).  Box tests only cull; every surviving
// sphere goes through the same per-sphere arithmetic as the brute-force
// sweep, and the lowest id wins ties, so the result is the brute-force result.
// ---------------------------------------------------------------------------
template <typename R, bool kRobust>
struct SphereTester;

__device__ __forceinline__ float bperm_f(float x, int32_t src) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(x)));
}
__device__ __forceinline__ int32_t bperm_i(int32_t x, int32_t src) { return __builtin_amdgcn_ds_bpermute(src << 2, x); }
__device__ __forceinline__ float bperm_any(float x, int32_t src) { return bperm_f(x, src); }
__device__ __forceinline__ double bperm_any(double x, int32_t src);
__device__ __forceinline__ double bperm_d(double x, int32_t src) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    const uint32_t lo = (uint32_t)bperm_i((int32_t)(uint32_t)b, src), hi = (uint32_t)bperm_i((int32_t)(b >> 32), src);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ double bperm_any(double x, int32_t src) { return bperm_d(x, src); }

template <bool kRobust>
struct SphereTester<double, kRobust> {   // exact reference arithmetic (sphere.rs:61-80)
    V3<double> o, d;
    double tmin, tb;
    int32_t best;
    __device__ __forceinline__ double bound() const { return tb; }
    // the ray and running result of lane `src` (subtree stealing)
    __device__ __forceinline__ void take(int32_t src) {
        o = mk(bperm_d(o.x, src), bperm_d(o.y, src), bperm_d(o.z, src));
        d = mk(bperm_d(d.x, src), bperm_d(d.y, src), bperm_d(d.z, src));
        tb = bperm_d(tb, src);
        best = bperm_i(best, src);
    }
    // returns whether the sphere is hit at all (t in [tmin, inf])
    __device__ __forceinline__ bool test_hit(const R4<double>& s, int32_t id) {
        double t;
        const bool hit = sphere_t(mk(s.x, s.y, s.z), s.w, o, d, tmin, t);
        if (hit && (best < 0 || t < tb || (t == tb && id < best))) {
            tb = t;
            best = id;
        }
        return hit;
    }
    __device__ __forceinline__ void test(const R4<double>& s, int32_t id) { (void)test_hit(s, id); }
};

template <bool kRobust>
struct SphereTester<float, kRobust> {    // the f32 sweep's arithmetic (see sphere_u)
    V3<float> o, d;
    float a, ia;
    uint32_t tminb, ub;
    int32_t best;
    __device__ __forceinline__ float bound() const { return __uint_as_float(ub + tminb); }
    // (ub, best) as one unsigned key whose order is test()'s: ub first, then the
    // id in signed order (best = -1 below every id); the minimum over partial
    // traversals of one ray is the single traversal's result (subtree stealing)
    __device__ __forceinline__ uint64_t key() const {
        return ((uint64_t)ub << 32) | ((uint32_t)best ^ 0x80000000u);
    }
    __device__ __forceinline__ void from_key(uint64_t k) {
        ub = (uint32_t)(k >> 32);
        best = (int32_t)((uint32_t)k ^ 0x80000000u);
    }
    // the ray and running result of lane `src` (every lane of the wave takes
    // part: ds_bpermute reads the source lane's registers)
    __device__ __forceinline__ void take(int32_t src) {
        o = mk(bperm_f(o.x, src), bperm_f(o.y, src), bperm_f(o.z, src));
        d = mk(bperm_f(d.x, src), bperm_f(d.y, src), bperm_f(d.z, src));
        ub = (uint32_t)bperm_i((int32_t)ub, src);
        best = bperm_i(best, src);
        a = len2_f32(d);
        ia = __builtin_amdgcn_rcpf(a);
    }
    __device__ __forceinline__ void test(const R4<float>& s, int32_t id) {
        const uint32_t u = sphere_u<kRobust>(s, o, d, a, ia, tminb);
        const bool upd = u < ub || (u == ub && id < best);
        ub = upd ? u : ub;
        best = upd ? id : best;
    }
    // returns whether the sphere is hit at all (t in [tmin, inf])
    __device__ __forceinline__ bool test_hit(const R4<float>& s, int32_t id) {
        const uint32_t u = sphere_u<kRobust>(s, o, d, a, ia, tminb);
        const bool upd = u < ub || (u == ub && id < best);
        ub = upd ? u : ub;
        best = upd ? id : best;
        return u <= 0x7f800000u - tminb;
    }
};

__device__ __forceinline__ double inv_(double x) { return 1.0 / x; }
__device__ __forceinline__ float inv_(float x) { return __builtin_amdgcn_rcpf(x); }
// One axis of a ray for the slab tests t = b ix - o ix: ix = 1 / d and o ix.
// f64: when o ix is not finite -- a zero direction component (ix = inf) -- the
// two planes of a box come out as a signed infinity and inf - inf = NaN (a box
// that straddles 0 with o beside 0: lo ix - o ix = -inf, hi ix - o ix = NaN),
// and fmin / fmax, which drop the NaN, would keep the infinity for both the
// near and the far plane: a box the ray passes through, culled.  Such an axis
// gets ix = o ix = NaN: every plane NaN, dropped by fmin / fmax -- the slab
// unbounded, which only ever keeps a box.  (The f32 speed mode keeps the plain
// form and with it that corner -- a direction component exactly 0 beside a
// non-zero origin component: its kernels are the parent's, instruction for
// instruction; the guard in them measured -1.3 % on the f32 headline.)
template <typename R>
__device__ __forceinline__ void slab_axis(R o, R d, R& ix, R& oix) {
    ix = inv_(d);
    oix = o * ix;
    if constexpr (sizeof(R) == 8) {
        if (!(fabs(oix) < (R)INFINITY)) ix = oix = (R)NAN;
    }
}
// The three axes of the while-while traversals' f32 slab tests: plain 1 / d
// and o ix.  kWide (an f64 ray on the f32 tree): a non-finite o ix makes the
// widening slack s = 2^-20 max |o ix| infinite, so an interval that the
// inf - inf above spoils ends as tn - s = NaN or tf + s = NaN, which the
// traversal's compare !(tn > tf) keeps: every box entered, correct and only
// slow, with no work at the ray's setup (the f64 headline pays for any).
__device__ __forceinline__ void ray_slabs(V3<float> o, V3<float> d, float& ix, float& iy, float& iz, float& oix,
                                          float& oiy, float& oiz) {
    ix = inv_(d.x), iy = inv_(d.y), iz = inv_(d.z);
    oix = o.x * ix, oiy = o.y * iy, oiz = o.z * iz;
}

// Near-child-first traversal with a per-lane stack in LDS (stk[entry * 64]).
// Slab test on padded child boxes against [0, tb].
template <typename R, typename TT>
__device__ __forceinline__ void bvh_traverse(const DevScene<R>& sc, int32_t base, V3<R> o, V3<R> d,
                                             TT& T, int32_t* __restrict__ stk,
                                             uint32_t& nvis, uint32_t& ntest, bool skip) {
    if (skip) return;
    R ix, iy, iz, oix, oiy, oiz;
    slab_axis(o.x, d.x, ix, oix);
    slab_axis(o.y, d.y, iy, oiy);
    slab_axis(o.z, d.z, iz, oiz);
    const BvhNode<R>* __restrict__ nodes = sc.bvh;
    int32_t sp = 0;
    int32_t node = 0;
    for (;;) {
        if (node >= 0) {
            ++nvis;
            const BvhNode<R>& nd = nodes[node];
            const R tb = T.bound();
            R tn[2], tf[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const R x0 = nd.lo_x[c] * ix - oix, x1 = nd.hi_x[c] * ix - oix;
                const R y0 = nd.lo_y[c] * iy - oiy, y1 = nd.hi_y[c] * iy - oiy;
                const R z0 = nd.lo_z[c] * iz - oiz, z1 = nd.hi_z[c] * iz - oiz;
                tn[c] = fmax(fmax(fmin(x0, x1), fmin(y0, y1)), fmax(fmin(z0, z1), (R)0));
                tf[c] = fmin(fmin(fmax(x0, x1), fmax(y0, y1)), fmin(fmax(z0, z1), tb));
            }
            const bool h0 = tn[0] <= tf[0], h1 = tn[1] <= tf[1];
            const int32_t c0 = nd.child[0], c1 = nd.child[1];
            if (h0 && h1) {
                const bool first0 = tn[0] <= tn[1];
                stk[sp * 64] = first0 ? c1 : c0;
                ++sp;
                node = first0 ? c0 : c1;
            } else if (h0) {
                node = c0;
            } else if (h1) {
                node = c1;
            } else {
                if (sp == 0) break;
                --sp;
                node = stk[sp * 64];
            }
        } else {
            const uint32_t code = (uint32_t)~node;
            const uint32_t first = code >> 4, cnt = code & 15u;
            for (uint32_t k = 0; k < cnt; ++k)
                T.test(sc.bsph[first + k], base + (int32_t)sc.bid[first + k]);
            ntest += cnt;
            if (sp == 0) break;
            --sp;
            node = stk[sp * 64];
        }
    }
}

// Test a parked leaf (<= 15 spheres, contiguous in bsph/bid) in groups of
// four: each group's slots are fetched at once (indices clamped to the leaf,
// so a short group re-tests its last sphere -- a no-op: same t, same id, and
// ties only move to a LOWER id) and tested without a data-dependent trip
// count.  With the default 4-sphere leaves there is exactly one group.
// f64 leaves: an f32 pre-pass (sphere_may_hit: the light pre-pass of
// lights_pdf_sum on {c, r^2}, with (r + e)^2 <= r^2 + e (r^2 + 1) + e^2) masks
// the spheres the ray may hit (e >= 2^-19 whatever the scale, so nothing here
// underflows, and coordinates beyond f32 keep every sphere, see the compares;
// the direction must keep d . d, its reciprocal and d . (o - c) normal f32
// numbers: |d|_1 within 2^-60 .. 2^46, the range include/rtw.h states -- below
// it d . d underflows and tc = +-inf; above it hb can overflow to tc = -inf,
// l2 = inf while (2^-18 |f|)^2, the bound, is still finite); only those get the f64 test, each read from
// the f64 leaf array -- the closest (t, id) does not depend on the order or on
// spheres the ray misses.  The pre-pass reads the leaf spheres rounded to f32
// (DevScene::bsph32, staged in LDS by the LDS-world kernel: half the bytes of
// the f64 array, which stays in HBM / L1 for the few candidates).  Holding the
// four f64 spheres across the mask loop instead spilled 78 VGPRs and ran
// slower.
__device__ __forceinline__ bool sphere_may_hit(const R4<float>& S, float ox, float oy, float oz, float dx,
                                               float dy, float dz, float ia, float on, float dn) {
    const float cx = S.x, cy = S.y, cz = S.z, r2 = S.w;   // the f64 sphere rounded to f32 (bsph32)
    const float fx = ox - cx, fy = oy - cy, fz = oz - cz;
    const float hb = __builtin_fmaf(dz, fz, __builtin_fmaf(dy, fy, dx * fx));
    const float tc = -hb * ia;
    const float lx = __builtin_fmaf(tc, dx, fx), ly = __builtin_fmaf(tc, dy, fy), lz = __builtin_fmaf(tc, dz, fz);
    const float l2 = __builtin_fmaf(lx, lx, __builtin_fmaf(ly, ly, lz * lz));
    const float f2 = __builtin_fmaf(fx, fx, __builtin_fmaf(fy, fy, fz * fz));
    const float e = 0x1p-18f * (on + fabsf(cx) + fabsf(cy) + fabsf(cz) + 0.5f * (r2 + 1.0f));
    const float rr = __builtin_fmaf(e, r2 + 1.0f + e, r2);
    // the compares keep the sphere on a NaN: coordinates beyond f32 (inf - inf)
    // decide nothing here, the f64 test does (and rejects a NaN ray anyway)
    return !(l2 > rr) & (!(hb > 2.0f * e * dn) | !(f2 > rr));
}
// |o|_1 of the light pre-pass's ray (light_may_hit), not below 2^-32: its slack
// E >= 2^-18 |o|_1 then stays >= 2^-50, so (r + E)^2 and 2 E |d|_1 are normal
// f32 numbers however small the scene (a scene of size 2^-70 squares to f32
// denormals, where the bound on l's error does not hold; there the pre-pass
// simply keeps more).
__device__ __forceinline__ float light_on(float ox, float oy, float oz) {
    return fmaxf(fabsf(ox) + fabsf(oy) + fabsf(oz), 0x1p-32f);
}
template <typename R, typename TT>
__device__ __forceinline__ void test_leaf(const DevScene<R>& sc, int32_t base, int32_t leaf,
                                          TT& T, uint32_t& ntest) {
    const uint32_t code = (uint32_t)~leaf;
    const uint32_t first = code >> 4, cnt = code & 15u;
    if constexpr (sizeof(R) == 8) {
        const float ox = (float)T.o.x, oy = (float)T.o.y, oz = (float)T.o.z;
        const float dx = (float)T.d.x, dy = (float)T.d.y, dz = (float)T.d.z;
        const float ia = __builtin_amdgcn_rcpf(__builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz)));
        const float on = fabsf(ox) + fabsf(oy) + fabsf(oz), dn = fabsf(dx) + fabsf(dy) + fabsf(dz);
        uint32_t mask = 0;
        for (uint32_t k = 0; k < cnt; ++k)
            mask |= (sphere_may_hit(sc.bsph32[first + k], ox, oy, oz, dx, dy, dz, ia, on, dn) ? 1u : 0u) << k;
        while (mask) {
            const uint32_t k = (uint32_t)__builtin_ctz(mask);
            mask &= mask - 1u;
            T.test(sc.bsph[first + k], base + (int32_t)sc.bid[first + k]);
        }
        ntest += cnt;
        return;
    }
    for (uint32_t g0 = 0; g0 < cnt; g0 += 4) {
        R4<R> s[4];
        int32_t id[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t i = first + min(g0 + k, cnt - 1);
            s[k] = sc.bsph[i];
            id[k] = (int32_t)sc.bid[i];
        }
        if constexpr (sizeof(R) == 4) {
            asm volatile("" : "+v"(s[0].x), "+v"(s[1].x), "+v"(s[2].x), "+v"(s[3].x), "+v"(id[0]), "+v"(id[1]),
                         "+v"(id[2]), "+v"(id[3]));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) T.test(s[k], base + id[k]);
    }
    ntest += cnt;
}

// "While-while" traversal with leaf postponing (Aila & Laine 2009): inner
// nodes and leaves are processed in separate wave-uniform phases, so the
// SIMD never runs the box-test and the sphere-test code under one divergent
// branch.  A lane that reaches a leaf parks it and keeps descending until it
// holds a second leaf; the inner phase ends when every lane holds a leaf (or
// is done), then all parked leaves are tested together.
//
// Both precisions cull on the f32 tree (sc.bvh32).  An f64 ray (the parity
// mode) is rounded to f32 and every slab interval is widened by a bound on
// the error of that f32 arithmetic, so a box the exact f64 ray meets within
// [0, tb] is never culled; the spheres that survive are tested in f64 as
// before (the result is the brute-force result, bit for bit).  With ix the
// f32 reciprocal (1 ulp) of the rounded direction, o and d rounded (2^-24),
// each slab parameter t = (b - o) / d comes out within
// |t| 2^-22 + |o ix| 2^-22.9 of its exact value; the interval [tn, tf] is
// widened to [tn (1 - 2^-20) - s, tf (1 + 2^-20) + s], s = 2^-20 max |o ix|,
// and the bound tb is rounded up to f32.
__device__ __forceinline__ const BvhNode<float>* cull_nodes(const DevScene<float>& sc) { return sc.bvh; }
__device__ __forceinline__ const BvhNode<float>* cull_nodes(const DevScene<double>& sc) { return sc.bvh32; }
__device__ __forceinline__ float cull_bound(float t) { return t; }
__device__ __forceinline__ float cull_bound(double t) {   // t rounded up to f32
    const float f = (float)t;
    return (double)f < t ? __uint_as_float(__float_as_uint(f) + 1u) : f;   // t > 0
}
template <typename R, typename TT>
__device__ __forceinline__ void bvh_traverse_ww(const DevScene<R>& sc, int32_t base, V3<R> o, V3<R> d,
                                                TT& T, int32_t* __restrict__ stk,
                                                uint32_t& nvis, uint32_t& ntest, bool skip) {
    constexpr int32_t kDone = 0x7fffffff;
    constexpr bool kWide = sizeof(R) == 8;   // f64 ray on the f32 tree: widened intervals
    float ix, iy, iz, oix, oiy, oiz;
    ray_slabs(mk((float)o.x, (float)o.y, (float)o.z), mk((float)d.x, (float)d.y, (float)d.z), ix, iy, iz, oix,
                     oiy, oiz);
    // fmaxf drops a NaN (0 x inf: that slab is unbounded anyway); kWide: an
    // infinite o ix makes the slack infinite and every widened interval NaN or
    // [-inf, inf] -- kept by the NaN-keeping compare below (ray_slabs)
    const float slack = kWide ? 0x1p-20f * fmaxf(fmaxf(fabsf(oix), fabsf(oiy)), fmaxf(fabsf(oiz), 0.0f)) : 0.0f;
    float tbw = kWide ? cull_bound(T.bound()) : 0.0f;   // kWide: tb as the culling bound, per leaf phase
    const BvhNode<float>* __restrict__ nodes = cull_nodes(sc);
    // b ix - o ix: fused in the f64 build too (built without contraction)
    auto slab = [](float b, float i, float oi) {
        if constexpr (kWide) return __builtin_fmaf(b, i, -oi);
        else return b * i - oi;
    };
    int32_t sp = 0;
    int32_t node = skip ? kDone : 0;   // inner node index, leaf code (< 0) or kDone
    int32_t leaf = 0;   // parked leaf code, 0 = none
    for (;;) {
        for (;;) {
            if (node < 0 && leaf == 0) {   // park the leaf, continue with the stack
                leaf = node;
                node = sp ? stk[--sp * 64] : kDone;
            }
            const bool inner = node >= 0 && node != kDone;
            if (!__any(inner) || __all(leaf != 0 || node == kDone)) break;
            if (inner) {
                RTW_PROBE_LANES(1);
                ++nvis;
                const BvhNode<float> nd = nodes[node];
                const float tb = kWide ? tbw : (float)T.bound();
                float tn[2], tf[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float x0 = slab(nd.lo_x[c], ix, oix), x1 = slab(nd.hi_x[c], ix, oix);
                    const float y0 = slab(nd.lo_y[c], iy, oiy), y1 = slab(nd.hi_y[c], iy, oiy);
                    const float z0 = slab(nd.lo_z[c], iz, oiz), z1 = slab(nd.hi_z[c], iz, oiz);
                    tn[c] = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.0f));
                    tf[c] = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), tb));
                    if constexpr (kWide) {
                        tn[c] = __builtin_fmaf(tn[c], 1.0f - 0x1p-20f, -slack);
                        tf[c] = __builtin_fmaf(tf[c], 1.0f + 0x1p-20f, slack);
                    }
                }
                // (a NaN interval -- kWide, an infinite slack -- keeps the box: ray_slabs)
                const bool h0 = kWide ? !(tn[0] > tf[0]) : tn[0] <= tf[0], h1 = kWide ? !(tn[1] > tf[1]) : tn[1] <= tf[1];
                const int32_t c0 = nd.child[0], c1 = nd.child[1];
                if (h0 && h1) {
                    const bool first0 = tn[0] <= tn[1];
                    stk[sp * 64] = first0 ? c1 : c0;
                    ++sp;
                    node = first0 ? c0 : c1;
                } else if (h0 | h1) {
                    node = h0 ? c0 : c1;
                } else {
                    node = sp ? stk[--sp * 64] : kDone;
                }
            }
        }
        if (!__any(leaf != 0)) break;   // no parked leaves: every lane is done
        if (leaf != 0) {
            RTW_PROBE_LANES(2);
            test_leaf(sc, base, leaf, T, ntest);
            leaf = 0;
            if constexpr (kWide) tbw = cull_bound(T.bound());
        }
    }
}

__device__ __forceinline__ uint32_t sign_bit(float x) { return __float_as_uint(x) >> 31; }
__device__ __forceinline__ int32_t link_of(float x) { return (int32_t)__float_as_uint(x); }
__device__ __forceinline__ int32_t link_of(double x) { return (int32_t)__double_as_longlong(x); }
__device__ __forceinline__ uint32_t sign_bit(double x) {
    return (uint32_t)(__double_as_longlong(x) >> 63) & 1u;
}

// Fetch a whole 4-wide node.  For f32 the eight 16-B loads are issued back
// to back and completed together (the empty asm takes every word as an
// operand); left alone, the scheduler interleaves them with the slab tests
// and waits for each child's second half separately -- four dependent memory
// round trips per visit instead of one.
__device__ __forceinline__ void load_node4(const Bvh4Node<float>& nd, R4<float> (&A)[4], R4<float> (&B)[4]) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4* p = reinterpret_cast<const f4*>(&nd);
    f4 v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3], v4 = p[4], v5 = p[5], v6 = p[6], v7 = p[7];
    asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7));
    const f4 v[8] = {v0, v1, v2, v3, v4, v5, v6, v7};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        A[c] = R4<float>{v[c].x, v[c].y, v[c].z, v[c].w};
        B[c] = R4<float>{v[4 + c].x, v[4 + c].y, v[4 + c].z, v[4 + c].w};
    }
}
__device__ __forceinline__ void load_node4(const Bvh4Node<double>& nd, R4<double> (&A)[4], R4<double> (&B)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        A[c] = nd.a[c];
        B[c] = nd.b[c];
    }
}

// 4-wide version of bvh_traverse_ww on the octant copies of the tree
// (Bvh4Node): the ray's octant picks the copy, whose children are already in
// front-to-back order and whose slab planes are already near/far for this
// octant.  The first hit child is visited next; the other hit children are
// pushed far-to-near (each store is unconditional, only the stack pointer
// advance is predicated, so a visit has no divergent branch).  The stack
// holds at most sc.bvh4_stack entries (host-computed bound) and is written
// one past its top.
template <typename R, typename TT>
__device__ __forceinline__ void bvh4_traverse(const DevScene<R>& sc, int32_t base, V3<R> o, V3<R> d,
                                              TT& T, int32_t* __restrict__ stk,
                                              uint32_t& nvis, uint32_t& ntest, bool skip) {
    constexpr int32_t kDone = 0x7fffffff;
    const R ix = inv_(d.x), iy = inv_(d.y), iz = inv_(d.z);
    const R oix = o.x * ix, oiy = o.y * iy, oiz = o.z * iz;
    const uint32_t oct = sign_bit(ix) | (sign_bit(iy) << 1) | (sign_bit(iz) << 2);
    const Bvh4Node<R>* __restrict__ nodes = sc.bvh4 + oct * sc.n_nodes4;
    int32_t sp = 0;
    int32_t node = skip ? kDone : 0;   // inner node index, leaf code (< 0) or kDone
    int32_t leaf = 0;   // parked leaf code, 0 = none
    for (;;) {
        for (;;) {
            if (node < 0 && leaf == 0) {   // park the leaf, continue with the stack
                leaf = node;
                node = sp ? stk[--sp * 64] : kDone;
            }
            const bool inner = node >= 0 && node != kDone;
            if (!__any(inner) || __all(leaf != 0 || node == kDone)) break;
            if (inner) {
                ++nvis;
                R4<R> NA[4], NB[4];
                load_node4(nodes[node], NA, NB);
                const R tb = T.bound();
                bool h[4];
                int32_t ch[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const R4<R> A = NA[c], B = NB[c];
                    const R xn = A.x * ix - oix, yn = A.y * iy - oiy, zn = A.z * iz - oiz;
                    const R xf = A.w * ix - oix, yf = B.x * iy - oiy, zf = B.y * iz - oiz;
                    const R tn = fmax(fmax(xn, yn), fmax(zn, (R)0));
                    const R tf = fmin(fmin(xf, yf), fmin(zf, tb));
                    h[c] = tn <= tf;
                    ch[c] = link_of(B.z);
                }
                const int32_t c0 = ch[0], c1 = ch[1], c2 = ch[2], c3 = ch[3];
                stk[sp * 64] = c3;
                sp += (h[3] && (h[0] || h[1] || h[2])) ? 1 : 0;
                stk[sp * 64] = c2;
                sp += (h[2] && (h[0] || h[1])) ? 1 : 0;
                stk[sp * 64] = c1;
                sp += (h[1] && h[0]) ? 1 : 0;
                if (h[0] | h[1] | h[2] | h[3])
                    node = h[0] ? c0 : (h[1] ? c1 : (h[2] ? c2 : c3));
                else
                    node = sp ? stk[--sp * 64] : kDone;
            }
        }
        if (!__any(leaf != 0)) break;   // no parked leaves: every lane is done
        if (leaf != 0) {
            test_leaf(sc, base, leaf, T, ntest);
            leaf = 0;
        }
    }
}

// Subtree stealing: the result slots of one wave's rays in LDS.  f32: one
// u64 key per ray (SphereTester<float>::key, folded with an atomic min).  f64:
// the t bits (t >= t_min > 0: their unsigned order is t's) and the id, folded
// in two wave-synchronous steps -- an atomic min of t, then the id of a lane
// whose t is the new minimum (stored by the lane that lowered it, atomic min
// among equal t) -- the tester's order (smallest t, then lowest id, best = -1
// above every id).  fold() must be called by every lane of the wave
// (`on` selects the folding lanes).
template <typename R>
struct StealSlots;
template <>
struct StealSlots<float> {
    unsigned long long* key;
    __device__ __forceinline__ explicit StealSlots(unsigned char* area)
        : key(reinterpret_cast<unsigned long long*>(area)) {}
    template <typename TT>
    __device__ __forceinline__ void init(uint32_t lane, const TT& T) { key[lane] = T.key(); }
    template <typename TT>
    __device__ __forceinline__ void fold(bool on, int32_t owner, TT& T, bool share) {
        if (on) {
            const uint64_t k = T.key();
            const uint64_t prev = atomicMin(key + owner, (unsigned long long)k);
            if (share) T.from_key(prev < k ? prev : k);
        }
    }
    template <typename TT>
    __device__ __forceinline__ void refresh(bool on, int32_t owner, TT& T) {
        if (on) {
            const uint64_t ko = key[owner];
            if (ko < T.key()) T.from_key(ko);
        }
    }
    template <typename TT>
    __device__ __forceinline__ void result(uint32_t lane, TT& T) { T.from_key(key[lane]); }
};
template <>
struct StealSlots<double> {
    // per ray: the exact result (t bits, id) -- lowered only by full folds, so
    // its id always belongs to its t -- and a culling bound (t bits) that the
    // lanes on the ray lower after every leaf phase with one atomic
    unsigned long long* tb;
    uint32_t* id;
    unsigned long long* cull;
    // a lane whose bound came from another lane's hit holds no hit at that t:
    // its id is above every real id (ties at that t go to the real hit; the
    // full fold's id step never picks it)
    static constexpr int32_t kForeign = 0x7fffffff;
    __device__ __forceinline__ explicit StealSlots(unsigned char* area)
        : tb(reinterpret_cast<unsigned long long*>(area)), id(reinterpret_cast<uint32_t*>(area + 64 * 8)),
          cull(reinterpret_cast<unsigned long long*>(area + 64 * 12)) {}
    static __device__ __forceinline__ uint64_t bits(double t) { return (uint64_t)__double_as_longlong(t); }
    template <typename TT>
    __device__ __forceinline__ void init(uint32_t lane, const TT& T) {
        tb[lane] = bits(T.tb);
        id[lane] = (uint32_t)T.best;
        cull[lane] = bits(T.tb);
    }
    // the exact (t, id) into the owner's result, in the tester's order
    // (smallest t, then lowest id; best = -1 above every id): an atomic min of
    // t, then the id of a lane whose t is the new minimum (stored by the lane
    // that lowered it, atomic min among equal t).  Every lane of the wave calls
    // it (`on` selects the folding lanes).
    template <typename TT>
    __device__ __forceinline__ void fold(bool on, int32_t owner, TT& T, bool) {
        const uint64_t t = bits(T.tb);
        bool lowered = false;
        if (on) {
            lowered = t < atomicMin(tb + owner, (unsigned long long)t);
            atomicMin(cull + owner, (unsigned long long)t);
        }
        __builtin_amdgcn_wave_barrier();
        const uint64_t cur = on ? tb[owner] : 0;
        if (on && t == cur && lowered) id[owner] = (uint32_t)T.best;
        __builtin_amdgcn_wave_barrier();
        if (on && t == cur) atomicMin(id + owner, (uint32_t)T.best);
    }
    // after a leaf phase: share the bound only (one returning atomic); a lane
    // whose t is above the ray's bound takes it with the foreign id
    template <typename TT>
    __device__ __forceinline__ void share(bool on, int32_t owner, TT& T) {
        if (on) {
            const uint64_t t = bits(T.tb);
            const uint64_t prev = atomicMin(cull + owner, (unsigned long long)t);
            if (prev < t) {
                T.tb = __longlong_as_double((long long)prev);
                T.best = kForeign;
            }
        }
    }
    template <typename TT>
    __device__ __forceinline__ void refresh(bool on, int32_t owner, TT& T) {
        if (on) {
            const uint64_t t = cull[owner];
            if (t < bits(T.tb)) {
                T.tb = __longlong_as_double((long long)t);
                T.best = kForeign;
            }
        }
    }
    template <typename TT>
    __device__ __forceinline__ void result(uint32_t lane, TT& T) {
        T.tb = __longlong_as_double((long long)tb[lane]);
        T.best = (int32_t)id[lane];
    }
};
template <typename TT>
__device__ __forceinline__ void steal_share(StealSlots<float>& S, bool on, int32_t owner, TT& T) {
    S.fold(on, owner, T, true);
}
template <typename TT>
__device__ __forceinline__ void steal_share(StealSlots<double>& S, bool on, int32_t owner, TT& T) {
    S.share(on, owner, T);
}

// bvh_traverse_ww with intra-wave subtree stealing.  A lane with nothing left
// to traverse -- its ray done, or never started (the own-sphere shortcut) --
// takes the bottom entry of another lane's stack (the largest subtree that
// lane has postponed) together with that lane's ray and running result, and
// traverses it as its own; lanes pair up by rank (the k-th idle lane with the
// k-th lane holding stack entries) through 64 rendezvous bytes in LDS, the ray
// moves with ds_bpermute.  Every lane on a ray folds its result into the ray
// owner's slot after each leaf phase and culls with the minimum so far (the
// bound is shared), and a finished partial traversal is folded before the
// lane steals again; the owner reads the minimum at the end.  Box tests only
// cull and the slot order is the tester's (smallest t, then lowest id), so
// the result is the single traversal's bit for bit (tests: BVH == brute
// force, f64 == oracle).  f64 rays cull on the f32 tree with widened slab
// intervals exactly as bvh_traverse_ww.  tools/steal_sim.cpp (lockstep
// simulation on C2 ray batches): 17.0 -> 8.4 inner passes and 3.9 -> 1.9
// leaf passes per 64 segments.
template <typename R, typename TT>
__device__ __forceinline__ void bvh_traverse_steal(const DevScene<R>& sc, int32_t base, TT& T,
                                                   int32_t* __restrict__ stk_wave, uint32_t lane,
                                                   unsigned char* __restrict__ steal_area, uint32_t& nvis,
                                                   uint32_t& ntest, bool skip) {
    constexpr int32_t kDone = 0x7fffffff;
    constexpr bool kWide = sizeof(R) == 8;   // f64 ray on the f32 tree: widened intervals
    StealSlots<R> slots(steal_area);
    uint8_t* __restrict__ rv = steal_area + kStealSlotBytes<R>;
    int32_t* __restrict__ stk = stk_wave + lane;
    float ix, iy, iz, oix, oiy, oiz, slack, tbw;
    auto setup = [&]() {
        ray_slabs(mk((float)T.o.x, (float)T.o.y, (float)T.o.z), mk((float)T.d.x, (float)T.d.y, (float)T.d.z),
                         ix, iy, iz, oix, oiy, oiz);
        slack = kWide ? 0x1p-20f * fmaxf(fmaxf(fabsf(oix), fabsf(oiy)), fmaxf(fabsf(oiz), 0.0f)) : 0.0f;
    };
    auto bound = [&]() { tbw = kWide ? cull_bound(T.bound()) : 0.0f; };
    setup();
    bound();
    auto slab = [](float b, float i, float oi) {
        if constexpr (kWide) return __builtin_fmaf(b, i, -oi);
        else return b * i - oi;
    };
    const BvhNode<float>* __restrict__ nodes = cull_nodes(sc);
    int32_t sp = 0, sb = 0;             // stack entries [sb, sp): below sb they were given away
    int32_t owner = (int32_t)lane;      // the lane whose ray this lane traverses
    int32_t node = skip ? kDone : 0;
    int32_t leaf = 0;
    slots.init(lane, T);
    for (;;) {
        for (;;) {
            if (node < 0 && leaf == 0) {   // park the leaf, continue with the stack
                leaf = node;
                node = sp > sb ? stk[--sp * 64] : kDone;
            }
            const bool idle = node == kDone && leaf == 0, donor = sp > sb;
            const uint64_t mi = __ballot(idle), md = __ballot(donor);
            if (mi != 0 && md != 0) {
                const uint32_t np = min(__popcll(mi), __popcll(md));
                const uint32_t ri = __builtin_amdgcn_mbcnt_hi((uint32_t)(mi >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mi, 0u));
                const uint32_t rd = __builtin_amdgcn_mbcnt_hi((uint32_t)(md >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)md, 0u));
                const bool thief = idle && ri < np, give = donor && rd < np;
                if (give) rv[rd] = (uint8_t)lane;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int32_t src = thief ? (int32_t)rv[ri] : (int32_t)lane;
                slots.fold(thief, owner, T, false);   // the thief's finished traversal
                const int32_t v_owner = bperm_i(owner, src), v_sb = bperm_i(sb, src);
                // every lane reads the ray of `src`: a thief its donor's, the
                // others their own (src = lane), so no copy of T is needed
                T.take(src);
                if (thief) {
                    owner = v_owner;
                    node = stk_wave[v_sb * 64 + src];
                    sp = sb = 0;
                    setup();
                }
                slots.refresh(thief, owner, T);       // the freshest shared bound
                if (thief) bound();
                if (give) ++sb;
            }
            const bool inner = node >= 0 && node != kDone;
            if (!__any(inner) || __all(leaf != 0 || node == kDone)) break;
            if (inner) {
                RTW_PROBE_LANES(1);
                ++nvis;
                const BvhNode<float>& nd = nodes[node];
                const float tb = kWide ? tbw : (float)T.bound();
                float tn[2], tf[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float x0 = slab(nd.lo_x[c], ix, oix), x1 = slab(nd.hi_x[c], ix, oix);
                    const float y0 = slab(nd.lo_y[c], iy, oiy), y1 = slab(nd.hi_y[c], iy, oiy);
                    const float z0 = slab(nd.lo_z[c], iz, oiz), z1 = slab(nd.hi_z[c], iz, oiz);
                    tn[c] = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.0f));
                    tf[c] = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), tb));
                    if constexpr (kWide) {
                        tn[c] = __builtin_fmaf(tn[c], 1.0f - 0x1p-20f, -slack);
                        tf[c] = __builtin_fmaf(tf[c], 1.0f + 0x1p-20f, slack);
                    }
                }
                // (a NaN interval -- kWide, an infinite slack -- keeps the box: ray_slabs)
                const bool h0 = kWide ? !(tn[0] > tf[0]) : tn[0] <= tf[0], h1 = kWide ? !(tn[1] > tf[1]) : tn[1] <= tf[1];
                const int32_t c0 = nd.child[0], c1 = nd.child[1];
                if (h0 && h1) {
                    const bool first0 = tn[0] <= tn[1];
                    stk[sp * 64] = first0 ? c1 : c0;
                    ++sp;
                    node = first0 ? c0 : c1;
                } else if (h0 | h1) {
                    node = h0 ? c0 : c1;
                } else {
                    node = sp > sb ? stk[--sp * 64] : kDone;
                }
            }
        }
        if (!__any(leaf != 0)) break;   // no parked leaves: every lane is done
        const bool tested = leaf != 0;
        if (tested) {
            RTW_PROBE_LANES(2);
            test_leaf(sc, base, leaf, T, ntest);
            leaf = 0;
        }
        // share the bound: every lane on this ray culls with the best hit any
        // of them has found so far (f32: the exact key; f64: the bound only,
        // the exact (t, id) is folded when a lane leaves the ray)
        steal_share(slots, tested, owner, T);
        if (tested) bound();
    }
    slots.fold(true, owner, T, false);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    slots.result(lane, T);
}

// A ray with a NaN component hits nothing (every sphere, plane and light test
// compares a NaN), but its slab tests keep every box (fmin / fmax drop the
// NaN), so a traversal would visit the whole tree for a miss -- C5: the NaN
// directions a Lambertian point inside a light sphere samples (sphere.rs:
// 113-127) cost one wave a quarter of a second.  Such rays skip the traversal
// (bvh_dispatch: the trees outside LDS; a tree in LDS is small, its stealing
// traversal shares such a walk, and the check costs C2 more than it saves).
template <typename R>
__device__ __forceinline__ bool ray_nan(V3<R> o, V3<R> d) {
    return __builtin_isnan(o.x) | __builtin_isnan(o.y) | __builtin_isnan(o.z) | __builtin_isnan(d.x) |
           __builtin_isnan(d.y) | __builtin_isnan(d.z);
}

// `self` >= 0: the ray starts on that (isolated) sphere; it is tested first
// and, when the ray hits it again, that hit is the closest sphere hit (see
// isolated_spheres, host/bvh.hpp) and the traversal is skipped.
template <int kKind, typename R, typename TT>
__device__ __forceinline__ void bvh_dispatch(const DevScene<R>& sc, int32_t base, V3<R> o, V3<R> d,
                                             TT& T, int32_t* stk, uint32_t& nvis,
                                             uint32_t& ntest, int32_t self) {
    bool skip = ray_nan(o, d);
    if (!skip && self >= 0) {
        skip = T.test_hit(sc.sph[self], base + self);
        ++ntest;
    }
    if constexpr (kKind == kWorldBvh4) bvh4_traverse(sc, base, o, d, T, stk, nvis, ntest, skip);
    else if constexpr (kKind == kWorldBvhWW) bvh_traverse_ww(sc, base, o, d, T, stk, nvis, ntest, skip);
    else bvh_traverse(sc, base, o, d, T, stk, nvis, ntest, skip);
}

template <int kKind, bool kRobust>
__device__ __forceinline__ void bvh_closest(const DevScene<double>& sc, int32_t base, V3<double> o,
                                            V3<double> d, double tmin, double& tb, int32_t& best,
                                            int32_t* stk, uint32_t& nvis, uint32_t& ntest, int32_t self) {
    SphereTester<double, kRobust> T{o, d, tmin, tb, best};
    bvh_dispatch<kKind>(sc, base, o, d, T, stk, nvis, ntest, self);
    tb = T.tb;
    best = T.best;
}
template <int kKind, bool kRobust>
__device__ __forceinline__ void bvh_closest(const DevScene<float>& sc, int32_t base, V3<float> o,
                                            V3<float> d, float tmin, float& tb, int32_t& best,
                                            int32_t* stk, uint32_t& nvis, uint32_t& ntest, int32_t self) {
    SphereTester<float, kRobust> T;
    T.o = o;
    T.d = d;
    T.a = len2_f32(d);
    T.ia = __builtin_amdgcn_rcpf(T.a);
    T.tminb = __float_as_uint(tmin);
    T.ub = __float_as_uint(tb) - T.tminb;
    T.best = best;
    bvh_dispatch<kKind>(sc, base, o, d, T, stk, nvis, ntest, self);
    tb = T.bound();
    best = T.best;
}

// The f32 sphere test with one sphere id excluded (kOptHit64: the sphere the
// ray starts on, whose re-hit is decided in f64).
template <bool kRobust>
struct SphereTesterX : SphereTester<float, kRobust> {
    int32_t excl;
    __device__ __forceinline__ void take(int32_t src) {
        SphereTester<float, kRobust>::take(src);
        excl = bperm_i(excl, src);
    }
    __device__ __forceinline__ void test(const R4<float>& s, int32_t id) {
        const uint32_t u = sphere_u<kRobust>(s, this->o, this->d, this->a, this->ia, this->tminb);
        const bool upd = (u < this->ub || (u == this->ub && id < this->best)) && id != excl;
        this->ub = upd ? u : this->ub;
        this->best = upd ? id : this->best;
    }
};
template <int kKind, bool kRobust>
__device__ __forceinline__ void bvh_closest_excl(const DevScene<float>& sc, int32_t base, V3<float> o,
                                                 V3<float> d, float tmin, float& tb, int32_t& best,
                                                 int32_t* stk, uint32_t& nvis, uint32_t& ntest, int32_t excl) {
    SphereTesterX<kRobust> T;
    T.o = o;
    T.d = d;
    T.a = len2_f32(d);
    T.ia = __builtin_amdgcn_rcpf(T.a);
    T.tminb = __float_as_uint(tmin);
    T.ub = __float_as_uint(tb) - T.tminb;
    T.best = best;
    T.excl = excl;
    bvh_dispatch<kKind>(sc, base, o, d, T, stk, nvis, ntest, -1);
    tb = T.bound();
    best = T.best;
}

// The same two queries with subtree stealing (while-while kernels): every
// active lane of the wave calls them -- a lane whose ray needs no traversal
// (the own-sphere shortcut: `skip`) helps the others.
template <bool kRobust>
__device__ __forceinline__ void bvh_closest_steal(const DevScene<double>& sc, int32_t base, V3<double> o,
                                                  V3<double> d, double tmin, double& tb, int32_t& best,
                                                  int32_t* stk_wave, uint32_t lane, unsigned char* steal_area,
                                                  uint32_t& nvis, uint32_t& ntest, int32_t self) {
    SphereTester<double, kRobust> T{o, d, tmin, tb, best};
    bool skip = false;
    if (self >= 0) {
        skip = T.test_hit(sc.sph[self], base + self);
        ++ntest;
    }
    bvh_traverse_steal(sc, base, T, stk_wave, lane, steal_area, nvis, ntest, skip);
    tb = T.tb;
    best = T.best;
}
template <bool kRobust>
__device__ __forceinline__ void bvh_closest_steal(const DevScene<float>& sc, int32_t base, V3<float> o, V3<float> d,
                                                  float tmin, float& tb, int32_t& best, int32_t* stk_wave,
                                                  uint32_t lane, unsigned char* steal_area, uint32_t& nvis,
                                                  uint32_t& ntest, int32_t self) {
    SphereTester<float, kRobust> T;
    T.o = o;
    T.d = d;
    T.a = len2_f32(d);
    T.ia = __builtin_amdgcn_rcpf(T.a);
    T.tminb = __float_as_uint(tmin);
    T.ub = __float_as_uint(tb) - T.tminb;
    T.best = best;
    bool skip = false;
    if (self >= 0) {
        skip = T.test_hit(sc.sph[self], base + self);
        ++ntest;
    }
    bvh_traverse_steal(sc, base, T, stk_wave, lane, steal_area, nvis, ntest, skip);
    tb = T.bound();
    best = T.best;
}
template <bool kRobust>
__device__ __forceinline__ void bvh_closest_excl_steal(const DevScene<float>& sc, int32_t base, V3<float> o,
                                                       V3<float> d, float tmin, float& tb, int32_t& best,
                                                       int32_t* stk_wave, uint32_t lane, unsigned char* steal_area,
                                                       uint32_t& nvis, uint32_t& ntest, int32_t excl, bool skip) {
    SphereTesterX<kRobust> T;
    T.o = o;
    T.d = d;
    T.a = len2_f32(d);
    T.ia = __builtin_amdgcn_rcpf(T.a);
    T.tminb = __float_as_uint(tmin);
    T.ub = __float_as_uint(tb) - T.tminb;
    T.best = best;
    T.excl = excl;
    bvh_traverse_steal(sc, base, T, stk_wave, lane, steal_area, nvis, ntest, skip);
    tb = T.bound();
    best = T.best;
}

}  // namespace dev

}  // namespace rtw
