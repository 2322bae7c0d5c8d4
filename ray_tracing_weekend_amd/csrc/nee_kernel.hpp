// nee_kernel.hpp -- what an integrator outside the library needs per shading
// point next to the light pdf (query_kernel.hpp), one ray / point per lane:
//   occlusion_kernel<R, world, robust>      world.hit(&r, t_min..=t_max[i]).is_some()
//                                           (hittable_list.rs:395-406, bvh.rs:164-188): any hit
//                                           in the inclusive range, stopping at the first
//   light_sample_kernel<R, path, robust>    lights.random(origin, rng) (hittable_list.rs:414-419)
//                                           and, fused, lights.pdf_value(origin, direction drawn)
// Both call the render kernel's device functions (render_kernel.hpp,
// bvh_traverse.hpp, light_pdf.hpp): per primitive the t that is compared with
// the range is the closest-hit query's t bit for bit, the traversals are its
// traversals with another tester, and the pdf is light_pdf_rays_kernel's.
//
// Any hit instead of the closest: a candidate is accepted when t_min <= t <=
// t_max (inclusive, the reference's RangeInclusive); a sphere whose near root
// is below t_min is tried at its far root (sphere.rs:72-80) -- sphere_t /
// sphere_u return exactly that root, and a near root above t_max has its far
// root above it too, so "the first root >= t_min is <= t_max" is the
// reference's answer.  The range is never shrunk (hittable_list.rs:399-405).
// Each plane, quad and cuboid sits behind its AABB gate over the same range
// (bounded_hit, hittable.rs:39-86): aabb_hit_range.  Spheres are tested
// without a box of their own, as in the closest-hit query.
//
// Early exit: a lane blocked by a plane, quad or cuboid does not enter the
// sphere traversal, and AnyTester::bound() falls to -inf with the first
// accepted sphere: every box still on the lane's stack is then culled by the
// traversal's own slab test (tf = min(.., -inf) < tn), and parked leaves are
// not tested.  The LDS tree runs the plain while-while traversal, without
// subtree stealing: a lane that is done simply idles.
#pragma once

#include "nee_kernels.h"
#include "query_kernel.hpp"

namespace rtw {

namespace dev {

// aabb_hit_ref (render_kernel.hpp; AABBox::hit, hittable.rs:291-339) over
// [rs, re]: with a finite upper end the gate's last compare takes it.
template <typename R, typename PP>
__device__ __forceinline__ bool aabb_hit_range(PP lo, PP hi, V3<R> o, V3<R> d, R rs, R re) {
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
    return P<R>::max_(rs, tmin) <= P<R>::min_(re, tmax);
}

// The traversals' tester (bvh_traverse.hpp SphereTester) for any hit in
// [tmin, tmax]: the per-sphere arithmetic is the closest-hit tester's.
template <typename R, bool kRobust>
struct AnyTester;
template <bool kRobust>
struct AnyTester<double, kRobust> {
    V3<double> o, d;
    double tmin, tmax;
    bool found;
    __device__ __forceinline__ void init(V3<double> o_, V3<double> d_, double tmin_, double tmax_) {
        o = o_, d = d_, tmin = tmin_, tmax = tmax_, found = false;
    }
    __device__ __forceinline__ double bound() const { return found ? -INFINITY : tmax; }
    __device__ __forceinline__ void test(const R4<double>& s, int32_t) {
        if (found) return;
        double t;
        found = sphere_t(mk(s.x, s.y, s.z), s.w, o, d, tmin, t) && t <= tmax;
    }
};
template <bool kRobust>
struct AnyTester<float, kRobust> {
    V3<float> o, d;
    float a, ia, tmax;
    uint32_t tminb, umax;   // u = bits(t) - bits(tmin) <= umax: t in [tmin, tmax] (sphere_u)
    bool found;
    __device__ __forceinline__ void init(V3<float> o_, V3<float> d_, float tmin_, float tmax_) {
        o = o_, d = d_, tmax = tmax_, found = false;
        a = len2_f32(d);
        ia = __builtin_amdgcn_rcpf(a);
        tminb = __float_as_uint(tmin_);
        umax = __float_as_uint(tmax_) - tminb;
    }
    __device__ __forceinline__ float bound() const { return found ? -INFINITY : tmax; }
    __device__ __forceinline__ void test(const R4<float>& s, int32_t) {
        found = found | (sphere_u<kRobust>(s, o, d, a, ia, tminb) <= umax);
    }
};

template <typename R, int kWorld, bool kRobust>
__global__ void __launch_bounds__(kQueryBlock) occlusion_kernel(const NParams<R> p) {
    extern __shared__ __attribute__((aligned(32))) unsigned char smem[];
    const R4<R>* __restrict__ sph = p.sc.sph;
    DevScene<R> scw = p.sc;
    if constexpr (kWorld == kWorldLds) {
        // the sphere list {c, r^2} in LDS, once per workgroup (hit_rays_kernel's)
        R4<R>* s_sph = reinterpret_cast<R4<R>*>(smem);
        for (uint32_t k = threadIdx.x; k < p.sc.n_sph; k += kQueryBlock) s_sph[k] = p.sc.sph[k];
        __syncthreads();
        sph = s_sph;
    }
    if constexpr (kWorld == kWorldBvhLds) {
        // hit_rays_kernel's staging, at its offsets (query_kernels.h query_hit_lds): the f32
        // tree the while-while traversal culls on, the f32 leaf spheres and their ids
        unsigned char* base = smem + traversal_lds<R>(p.stack, false, kQueryWaves);
        BvhNode<float>* l_nodes = reinterpret_cast<BvhNode<float>*>(base);
        R4<float>* l_bsph = reinterpret_cast<R4<float>*>(l_nodes + p.sc.n_nodes);
        uint32_t* l_bid = reinterpret_cast<uint32_t*>(l_bsph + p.sc.n_sph);
        const uint4* g_nodes = reinterpret_cast<const uint4*>(cull_nodes(p.sc));
        constexpr uint32_t kNode16 = sizeof(BvhNode<float>) / 16;
        for (uint32_t k = threadIdx.x; k < p.sc.n_nodes * kNode16; k += kQueryBlock)
            reinterpret_cast<uint4*>(l_nodes)[k] = g_nodes[k];
        const R4<float>* g_bsph32;
        if constexpr (sizeof(R) == 4) g_bsph32 = p.sc.bsph;
        else g_bsph32 = p.sc.bsph32;
        for (uint32_t k = threadIdx.x; k < p.sc.n_sph; k += kQueryBlock) {
            l_bsph[k] = g_bsph32[k];
            l_bid[k] = p.sc.bid[k];
        }
        __syncthreads();
        if constexpr (sizeof(R) == 4) {
            scw.bvh = l_nodes;
            scw.bsph = l_bsph;
        } else {
            scw.bvh32 = l_nodes;
            scw.bsph32 = l_bsph;
        }
        scw.bid = l_bid;
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int32_t* const stk = reinterpret_cast<int32_t*>(smem) + wave * p.stack * 64 + lane;
    (void)stk;
    const R tmin = p.tmin;
    const int32_t nplanes = (int32_t)p.sc.n_planes, nquads = (int32_t)p.sc.n_quads;
    const int32_t sbase = nplanes + nquads + (int32_t)p.sc.n_boxes;
    unsigned long long cnt[kQueryCounters] = {};

    // a workgroup takes ray blocks grid-stride: the staging above is paid once
    const uint64_t n_blocks = (p.n + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t k = blk * kQueryBlock + threadIdx.x;
        const bool live = k < p.n;
        V3<R> o = mk((R)NAN, (R)NAN, (R)NAN), d = o;
        R tmax = (R)INFINITY;
        if (live) {
            const R* r = p.rays + 6 * k;
            o = mk(r[0], r[1], r[2]);
            d = mk(r[3], r[4], r[5]);
            if (p.tmax) tmax = p.tmax[k];
        }
        // an empty or NaN range, a NaN ray, a lane without a ray: nothing to test, 0
        const bool open = live && tmax >= tmin && !ray_nan(o, d);
        bool blocked = false;
        if (open) {
            for (int32_t q = 0; q < nplanes && !blocked; ++q) {
                R t;
                const R* pl = p.sc.planes + kPlaneR * q;
                blocked = aabb_hit_range(pl + 6, pl + 9, o, d, tmin, tmax) && plane_t(pl, o, d, tmin, t, nullptr) &&
                          t <= tmax;
            }
            for (int32_t q = 0; q < nquads && !blocked; ++q) {
                R t;
                const R* Q = p.sc.quads + kQuadR * q;
                blocked = aabb_hit_range(Q + 16, Q + 19, o, d, tmin, tmax) && quad_t_hit(Q, o, d, tmin, tmax, t);
            }
            for (int32_t q = 0; q < (int32_t)p.sc.n_boxes && !blocked; ++q) {
                R t;
                int qd;
                V3<R> o2, d2;
                const R* B = p.sc.boxes + kBoxR * q;
                blocked = aabb_hit_range(B + kBoxLo, B + kBoxHi, o, d, tmin, tmax) &&
                          box_t_hit(B, o, d, tmin, tmax, t, qd, o2, d2);
            }
        }
        // ---- the spheres: only the lanes still open
        const bool walk = open && !blocked;
        AnyTester<R, kRobust> T;
        T.init(o, d, tmin, tmax);
        uint32_t nvis = 0, ntest = 0;
        if constexpr (kWorld == kWorldBvh4) {
            bvh4_traverse(scw, sbase, o, d, T, stk, nvis, ntest, !walk);
        } else if constexpr (kWorld == kWorldBvhWW || kWorld == kWorldBvhLds) {
            // wave-wide loops: every lane enters, the ones with nothing to walk skip
            bvh_traverse_ww(scw, sbase, o, d, T, stk, nvis, ntest, !walk);
        } else if constexpr (kWorld == kWorldBvh) {
            bvh_traverse(scw, sbase, o, d, T, stk, nvis, ntest, !walk);
        } else {
            if (walk) {
                const uint32_t ns = p.sc.n_sph;
                for (uint32_t k0 = 0; k0 < ns && !T.found; k0 += 8) {
                    const uint32_t k1 = min(k0 + 8u, ns);
                    for (uint32_t s = k0; s < k1; ++s) T.test(sph[s], sbase + (int32_t)s);
                    ntest += k1 - k0;
                }
            }
        }
        cnt[kQcNodeVisits] += nvis;
        cnt[kQcSphereTests] += ntest;
        if (!live) continue;
        const bool occ = blocked || (walk && T.found);
        cnt[kQcRays] += 1;
        cnt[kQcHits] += occ ? 1 : 0;
        p.occluded[k] = occ ? (uint8_t)1 : (uint8_t)0;
    }
    query_counters_flush(smem, p.counters, cnt);
}

template <typename R, int kPath, bool kRobust>
__global__ void __launch_bounds__(kQueryBlock) light_sample_kernel(const NParams<R> p) {
    using PR = P<R>;
    extern __shared__ __attribute__((aligned(32))) unsigned char smem[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int32_t* const stk = reinterpret_cast<int32_t*>(smem) + wave * p.stack * 64 + lane;
    (void)stk;
    unsigned long long cnt[kQueryCounters] = {};
    const uint64_t n_blocks = (p.n + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t k = blk * kQueryBlock + threadIdx.x;
        if (k >= p.n) continue;   // (the draws and the light walks are per lane)
        const R* r = p.origins + 3 * k;
        const V3<R> o = mk(r[0], r[1], r[2]);
        // the stream a render gives to (seed, pixel first_stream + k, sample); the draws of
        // its Lambertian branch for lights.random: one index, then the entry's random()
        Rng g;
        g.seed(p.seed, p.first_stream + k, (uint64_t)p.sample);
        const uint32_t idx = g.index(p.sc.n_list);   // (the host refuses an empty list)
        const uint32_t ref = p.sc.lref ? p.sc.lref[idx] : idx;
        V3<R> d;
        if (ref & kLrefQuad) {
            d = quad_random(p.sc.lquads + kQuadR * (ref & 0x3fffffffu), o, g);
        } else if (ref & kLrefDefault) {
            d = mk<R>(1, 0, 0);                      // Hittable::random default
        } else {
            const R4<R> L = p.sc.lights[ref];
            d = sphere_random(mk(L.x, L.y, L.z), L.w, o, g);
        }
        R* out = p.dirs + 3 * k;
        out[0] = d.x;
        out[1] = d.y;
        out[2] = d.z;
        if (p.light) p.light[k] = (int32_t)idx;
        cnt[kQcRays] += 1;
        if (!p.pdf) continue;
        R acc;                    // light_pdf_rays_kernel's, on {o, d}
        LightWork lw;
        if constexpr (kPath == kLightMixed) {
            acc = lights_pdf_mixed(p.sc, p.sc.lights, o, d);
            lw.tests = p.sc.n_list;
        } else if constexpr (kPath == kLightGrid) {
            acc = lights_pdf_grid<kRobust>(p.sc, o, d, lw);
        } else if constexpr (kPath == kLightBvh) {
            acc = lights_pdf_bvh<kRobust>(p.sc, o, d, stk, lw);
        } else {
            acc = lights_pdf_sum<kRobust>(p.sc.lights, p.sc.n_lights, o, d);
            lw.tests = p.sc.n_lights;
        }
        R lpdf = PR::div_(acc, (R)p.sc.n_list);
        if (p.sc.light_flags & 1u) lpdf = PR::div_(lpdf * (R)p.sc.n_list, (R)p.sc.n_list);
        p.pdf[k] = lpdf;
        cnt[kQcLightTests] += lw.tests;
    }
    query_counters_flush(smem, p.counters, cnt);
}

}  // namespace dev

}  // namespace rtw
