// query_kernel.hpp -- the batched ray queries on the staged scene, one ray
// per lane:
//   hit_rays_kernel<R, world, robust>       world.hit(&r, t_min..=INFINITY) of a HittableList /
//                                           BoundedVolumeHierarchy (hittable_list.rs, bvh.rs:164-188)
//                                           -> HitRecord::new (hittable.rs:100-129)
//   light_pdf_rays_kernel<R, path, robust>  HittableList::pdf_value of the light list
//                                           (hittable_list.rs:408-412; the BVH-leaf form bvh.rs:67-76)
// Both call the render kernel's device functions (render_kernel.hpp,
// bvh_traverse.hpp, light_pdf.hpp): the same per-primitive tests, the same
// traversals -- the f32-culled f64 walk and subtree stealing included -- so
// what a query answers is what a render's segment would have met.  Two pieces
// of render_kernel's body are restated here, because sharing them would change
// the render kernels' code: the staging of the tree into LDS (kWorldBvhLds)
// and the hit record; tests/test_gpu_query*.py hold each against the oracle.
//
// f32: the plain f32 arithmetic of the f32 kernels (sphere_u); the f64 hit
// point refinement of the render (kOptHit64) is not part of a query.
#pragma once

#include "query_kernels.h"
#include "render_kernel.hpp"

namespace rtw {

namespace dev {

// The workgroup's counters: every wave sums its lanes' (all lanes arrive here
// together), lane 0 adds the wave's to the workgroup's in LDS, and the
// workgroup adds each sum to the global counter once.
template <int kN>
__device__ __forceinline__ void query_counters_flush(unsigned char* smem, unsigned long long* __restrict__ global,
                                                     const unsigned long long (&mine)[kN]) {
    static_assert(kN * sizeof(unsigned long long) <= kQueryLdsMin, "the counters fit the smallest LDS block");
    unsigned long long* wg = reinterpret_cast<unsigned long long*>(smem);
    __syncthreads();   // (the LDS is free: every wave has left the ray loop)
    if (threadIdx.x < (uint32_t)kN) wg[threadIdx.x] = 0ull;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kN; ++q) {
        unsigned long long v = mine[q];
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off);
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
            v += ((unsigned long long)hi << 32) | lo;
        }
        if ((threadIdx.x & 63u) == 0 && v) atomicAdd(wg + q, v);
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kN && wg[threadIdx.x]) atomicAdd(global + threadIdx.x, wg[threadIdx.x]);
}

// bvh_closest_steal (bvh_traverse.hpp) for a wave whose lanes may have no ray:
// such a lane passes `skip` and starts as a thief.  No own-sphere shortcut: a
// query ray does not know what it starts on.
template <bool kRobust>
__device__ __forceinline__ void query_closest_steal(const DevScene<double>& sc, int32_t base, V3<double> o,
                                                    V3<double> d, double tmin, double& tb, int32_t& best,
                                                    int32_t* stk_wave, uint32_t lane, unsigned char* steal_area,
                                                    uint32_t& nvis, uint32_t& ntest, bool skip) {
    SphereTester<double, kRobust> T{o, d, tmin, tb, best};
    bvh_traverse_steal(sc, base, T, stk_wave, lane, steal_area, nvis, ntest, skip);
    tb = T.tb;
    best = T.best;
}
template <bool kRobust>
__device__ __forceinline__ void query_closest_steal(const DevScene<float>& sc, int32_t base, V3<float> o, V3<float> d,
                                                    float tmin, float& tb, int32_t& best, int32_t* stk_wave,
                                                    uint32_t lane, unsigned char* steal_area, uint32_t& nvis,
                                                    uint32_t& ntest, bool skip) {
    SphereTester<float, kRobust> T;
    T.o = o;
    T.d = d;
    T.a = len2_f32(d);
    T.ia = __builtin_amdgcn_rcpf(T.a);
    T.tminb = __float_as_uint(tmin);
    T.ub = __float_as_uint(tb) - T.tminb;
    T.best = best;
    bvh_traverse_steal(sc, base, T, stk_wave, lane, steal_area, nvis, ntest, skip);
    tb = T.bound();
    best = T.best;
}

template <typename R, int kWorld, bool kRobust>
__global__ void __launch_bounds__(kQueryBlock) hit_rays_kernel(const QParams<R> p) {
    using PR = P<R>;
    extern __shared__ __attribute__((aligned(32))) unsigned char smem[];
    const R4<R>* __restrict__ sph = p.sc.sph;
    DevScene<R> scw = p.sc;
    if constexpr (kWorld == kWorldLds) {
        // the sphere list {c, r^2} in LDS, once per workgroup (render_kernel's kWorldLds)
        R4<R>* s_sph = reinterpret_cast<R4<R>*>(smem);
        for (uint32_t k = threadIdx.x; k < p.sc.n_sph; k += kQueryBlock) s_sph[k] = p.sc.sph[k];
        __syncthreads();
        sph = s_sph;
    }
    if constexpr (kWorld == kWorldBvhLds) {
        // render_kernel's kWorldBvhLds staging, its head: the f32 tree (f64: bvh32) the
        // while-while traversal culls on, the f32 leaf spheres (f64: the pre-pass copy
        // bsph32; the f64 candidates stay in global memory) and their ids
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
    int32_t* const stk_wave = reinterpret_cast<int32_t*>(smem) + wave * p.stack * 64;
    unsigned char* const steal_area =
        smem + (size_t)kQueryWaves * p.stack * 64 * sizeof(int32_t) + wave * kStealLdsPerWave<R>;
    (void)stk_wave;
    (void)steal_area;
    const R tmin = p.tmin;
    const int32_t nplanes = (int32_t)p.sc.n_planes, nquads = (int32_t)p.sc.n_quads;
    const int32_t bbase = nplanes + nquads;                  // object ids: planes, quads,
    const int32_t sbase = bbase + (int32_t)p.sc.n_boxes;     // cuboids, spheres
    unsigned long long cnt[kQueryCounters] = {};

    // a workgroup takes ray blocks grid-stride: the staging above is paid once
    const uint64_t n_blocks = (p.n + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t k = blk * kQueryBlock + threadIdx.x;
        const bool live = k < p.n;
        // a lane without a ray carries a NaN ray: it hits nothing, and the per-lane
        // traversals skip it (bvh_dispatch: ray_nan)
        V3<R> o = mk((R)NAN, (R)NAN, (R)NAN), d = o;
        if (live) {
            const R* r = p.rays + 6 * k;
            o = mk(r[0], r[1], r[2]);
            d = mk(r[3], r[4], r[5]);
        }
        // ---- world.hit(&r, t_min..=INFINITY): closest over all primitives, the lowest
        // id on equal t (render_kernel's segment, without the own-sphere shortcut)
        R tb = (R)INFINITY;
        int32_t best = -1;
        if (live) {
            for (int32_t q = 0; q < nplanes; ++q) {
                R t;
                const R* pl = p.sc.planes + kPlaneR * q;
                if (aabb_hit_plane(pl + 6, pl + 9, o, d, tmin) && plane_t(pl, o, d, tmin, t, nullptr) &&
                    (best < 0 || t < tb)) {
                    tb = t;
                    best = q;
                }
            }
            // quads and transformed cuboids, each behind its AABB (bounded_hit, hittable.rs:190-196)
            for (int32_t q = 0; q < nquads; ++q) {
                R t;
                const R* Q = p.sc.quads + kQuadR * q;
                if (aabb_hit_ref(Q + 16, Q + 19, o, d, tmin) && quad_t_hit(Q, o, d, tmin, (R)INFINITY, t) &&
                    (best < 0 || t < tb)) {
                    tb = t;
                    best = nplanes + q;
                }
            }
            for (int32_t q = 0; q < (int32_t)p.sc.n_boxes; ++q) {
                R t;
                int qd;
                V3<R> o2, d2;
                const R* B = p.sc.boxes + kBoxR * q;
                if (aabb_hit_ref(B + kBoxLo, B + kBoxHi, o, d, tmin) &&
                    box_t_hit(B, o, d, tmin, (R)INFINITY, t, qd, o2, d2) && (best < 0 || t < tb)) {
                    tb = t;
                    best = bbase + q;
                }
            }
        }
        uint32_t nvis = 0, ntest = 0;
        if constexpr (kWorld == kWorldBvhLds) {
            // wave-wide: every lane enters, the ones without a ray as thieves
            query_closest_steal<kRobust>(scw, sbase, o, d, tmin, tb, best, stk_wave, lane, steal_area, nvis, ntest,
                                         !live);
        } else if constexpr (kWorld >= kWorldBvh) {
            bvh_closest<kWorld, kRobust>(scw, sbase, o, d, tmin, tb, best, stk_wave + lane, nvis, ntest, -1);
        } else {
            if (live) {
                sweep_spheres<kRobust>(sph, p.sc.n_sph, sbase, o, d, tmin, tb, best);
                ntest = p.sc.n_sph;
            }
        }
        cnt[kQcNodeVisits] += nvis;
        cnt[kQcSphereTests] += ntest;
        if (!live) continue;
        cnt[kQcRays] += 1;
        R* h = p.hits + 9 * k;
        int32_t* id = p.ids + 4 * k;
        if (best < 0) {   // a miss: object -1, every other field 0
#pragma unroll
            for (int q = 0; q < 9; ++q) h[q] = (R)0;
            id[0] = -1;
            id[1] = id[2] = id[3] = 0;
            continue;
        }
        cnt[kQcHits] += 1;
        // ---- HitRecord::new, hittable.rs:101-129 (render_kernel's, with the UVs of
        // every primitive)
        V3<R> pnt = o + d * tb;
        V3<R> outward;
        R hu = (R)0, hv = (R)0;
        uint32_t m;
        int32_t kind;
        bool front;
        if (best >= bbase && best < sbase) {
            // Transformed<Cuboid>: the record of the object-space hit, its point mapped
            // back; the normal and front face stay in object space (transformations.rs:14-29)
            const R* B = p.sc.boxes + kBoxR * (best - bbase);
            R t2;
            int qd = 0;
            V3<R> o2, d2;
            box_t_hit(B, o, d, tmin, (R)INFINITY, t2, qd, o2, d2);
            const R* Q = B + kQuadR * qd;
            outward = q3(Q, 12);
            front = dot(d2, outward) < (R)0;
            const V3<R> po = o2 + d2 * t2;
            pnt = mat3_mul(B + kBoxRot, po) + q3(B, kBoxT);
            const V3<R> pq = po - q3(Q, 0);                    // get_quad_uv, object space
            hu = dot(cross(pq, q3(Q, 6)), q3(Q, 9));
            hv = dot(cross(q3(Q, 3), pq), q3(Q, 9));
            m = p.sc.box_mat[best - bbase];
            kind = kPrimCuboid;
        } else if (best < nplanes) {
            const R* pl = p.sc.planes + kPlaneR * best;
            outward = mk(pl[3], pl[4], pl[5]);
            front = dot(d, outward) < (R)0;
            plane_uv(pl, pnt, hu, hv);                         // get_plane_uv, plane.rs:40-54
            m = p.sc.plane_mat[best];
            kind = kPrimPlane;
        } else if (best < bbase) {
            const R* Q = p.sc.quads + kQuadR * (best - nplanes);
            outward = q3(Q, 12);                               // quadrilateral.rs:97
            front = dot(d, outward) < (R)0;
            const V3<R> pq = pnt - q3(Q, 0);                   // get_quad_uv, quadrilateral.rs:58-63
            hu = dot(cross(pq, q3(Q, 6)), q3(Q, 9));
            hv = dot(cross(q3(Q, 3), pq), q3(Q, 9));
            m = p.sc.quad_mat[best - nplanes];
            kind = kPrimQuad;
        } else {
            const uint32_t s = (uint32_t)(best - sbase);
            const R4<R> sk = p.sc.sph[s];
            outward = PR::divs(pnt - mk(sk.x, sk.y, sk.z), p.sc.sph_r[s]);   // sphere.rs:82-83
            front = dot(d, outward) < (R)0;
            sphere_uv(outward, hu, hv);                        // get_sphere_uv, sphere.rs:49-58
            m = p.sc.sph_mat[s] & 0xffffffu;
            kind = kPrimSphere;
        }
        const V3<R> nrm = front ? outward : -outward;
        h[0] = tb;
        h[1] = pnt.x;
        h[2] = pnt.y;
        h[3] = pnt.z;
        h[4] = nrm.x;
        h[5] = nrm.y;
        h[6] = nrm.z;
        h[7] = hu;
        h[8] = hv;
        id[0] = best;
        id[1] = (int32_t)m;
        id[2] = front ? 1 : 0;
        id[3] = kind;
    }
    query_counters_flush(smem, p.counters, cnt);
}

template <typename R, int kPath, bool kRobust>
__global__ void __launch_bounds__(kQueryBlock) light_pdf_rays_kernel(const QParams<R> p) {
    using PR = P<R>;
    extern __shared__ __attribute__((aligned(32))) unsigned char smem[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int32_t* const stk = reinterpret_cast<int32_t*>(smem) + wave * p.stack * 64 + lane;
    (void)stk;
    unsigned long long cnt[kQueryCounters] = {};
    const uint64_t n_blocks = (p.n + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t k = blk * kQueryBlock + threadIdx.x;
        if (k >= p.n) continue;   // (the light walks are per lane)
        const R* r = p.rays + 6 * k;
        const V3<R> o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
        R acc;                    // hittable_list.rs:408-412, as render_kernel's Lambertian bounce
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
        // / len (an empty list: 0 / 0); a BVH leaf list multiplies by len and divides
        // again (bvh.rs:67-76, 191-194)
        R lpdf = PR::div_(acc, (R)p.sc.n_list);
        if (p.sc.light_flags & 1u) lpdf = PR::div_(lpdf * (R)p.sc.n_list, (R)p.sc.n_list);
        p.pdf[k] = lpdf;
        cnt[kQcRays] += 1;
        cnt[kQcLightTests] += lw.tests;
    }
    query_counters_flush(smem, p.counters, cnt);
}

}  // namespace dev

}  // namespace rtw
