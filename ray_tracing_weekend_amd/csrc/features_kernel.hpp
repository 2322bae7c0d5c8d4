// features_kernel.hpp -- the feature pass for denoisers, one pixel per lane:
//   primary_features_kernel<R, world, robust>  for each sample s of a pixel, the primary ray of
//                                              Camera::get_ray (camera.rs:274-293) ->
//                                              world.hit(&r, EPSILON..=INFINITY) -> 8 channels
//                                              {albedo, normal, distance, hit}, folded in f64
// A wave takes one 8 x 8 tile at a time from a global counter; lane l owns pixel
// (l & 7, l >> 3) of the tile and folds its samples in increasing order into 8
// f64 accumulators in registers, so a pixel's sums do not depend on how its
// samples were split over calls (windows) or cut short (counts).  The
// per-primitive tests, the traversals and the textures are the render
// kernel's device functions, called as they are.  Two pieces are restated,
// because sharing them would change the existing kernels' code: the primary
// ray of render_kernel's start_sample and the hit record of hit_rays_kernel
// (with its LDS staging); tests/test_gpu_features.py holds both to the oracle.
//
// f32: a query's plain f32 arithmetic per sample, widened exactly; the fold is
// f64 in both precisions.
#pragma once

#include "features_kernels.h"
#include "query_kernel.hpp"

namespace rtw {

namespace dev {

// t * |d| (each operation rounded by itself in both precisions)
template <typename R>
__device__ __forceinline__ R ray_distance(V3<R> d, R t) {
#pragma clang fp contract(off)
    return t * P<R>::sqrt_((d.x * d.x + d.y * d.y) + d.z * d.z);
}

template <typename R, int kWorld, bool kRobust>
__global__ void __launch_bounds__(kQueryBlock) primary_features_kernel(const FParams<R> p) {
    using PR = P<R>;
    extern __shared__ __attribute__((aligned(32))) unsigned char smem[];
    const R4<R>* __restrict__ sph = p.sc.sph;
    DevScene<R> scw = p.sc;
    if constexpr (kWorld == kWorldLds) {
        // the sphere list {c, r^2} in LDS, once per workgroup (hit_rays_kernel's kWorldLds)
        R4<R>* s_sph = reinterpret_cast<R4<R>*>(smem);
        for (uint32_t k = threadIdx.x; k < p.sc.n_sph; k += kQueryBlock) s_sph[k] = p.sc.sph[k];
        __syncthreads();
        sph = s_sph;
    }
    if constexpr (kWorld == kWorldBvhLds) {
        // hit_rays_kernel's kWorldBvhLds staging: the f32 tree, the f32 leaf spheres and
        // their ids after the traversal area (query_hit_lds)
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
    const R tmin = PR::kEps;
    const int32_t nplanes = (int32_t)p.sc.n_planes, nquads = (int32_t)p.sc.n_quads;
    const int32_t bbase = nplanes + nquads;                  // object ids: planes, quads,
    const int32_t sbase = bbase + (int32_t)p.sc.n_boxes;     // cuboids, spheres
    unsigned long long cnt[kQueryCounters] = {};

    // tile costs differ (sky against a sphere field): every wave takes its next
    // tile from the counter, one atomic per wave and tile
    for (;;) {
        uint32_t tile = 0;
        if (lane == 0) tile = (uint32_t)atomicAdd(p.counters + kFeatureNextTile, 1ull);
        tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile);
        if (tile >= p.n_tiles) break;
        const uint32_t ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
        const uint32_t i = tx * kTile + (lane & 7u), j = ty * kTile + (lane >> 3);
        const bool inside = i < p.W && j < p.H;
        const uint64_t pix = inside ? (uint64_t)j * p.W + i : 0;
        // this pixel's samples [first, end)
        uint32_t end = inside ? p.end : 0u;
        if (inside && p.counts) end = min(end, p.counts[pix]);
        const uint32_t mine = end > p.first ? end - p.first : 0u;
        double acc[kFeatureChannels];
#pragma unroll
        for (int q = 0; q < (int)kFeatureChannels; ++q) acc[q] = 0.0;
        double2* const out = reinterpret_cast<double2*>(p.features + pix * kFeatureChannels);
        if (mine && p.first) {
#pragma unroll
            for (int q = 0; q < (int)kFeatureChannels / 2; ++q) {
                const double2 v = out[q];
                acc[2 * q] = v.x;
                acc[2 * q + 1] = v.y;
            }
        }
        // the stealing traversal needs the whole wave in every trip: the trips are the
        // wave's longest pixel's, and a lane out of samples (or of the image) goes along
        // without a ray
        uint32_t trips = mine;
        for (int off = 32; off > 0; off >>= 1) trips = max(trips, (uint32_t)__shfl_xor((int)trips, off));
        for (uint32_t k = 0; k < trips; ++k) {
            const bool live = k < mine;
            const uint32_t s = p.first + k;
            // a lane without a ray carries a NaN ray: it hits nothing, and the per-lane
            // traversals skip it (bvh_dispatch: ray_nan)
            V3<R> o = mk((R)NAN, (R)NAN, (R)NAN), d = o;
            if (live) {
                // Camera::get_ray, camera.rs:274-293 (render_kernel's start_sample)
                Rng g;
                g.seed(p.seed, pix, s);
                R ox = PR::u_incl(g.next(), (R)-0.5, p.u_scale);
                R oy = PR::u_incl(g.next(), (R)-0.5, p.u_scale);
                V3<R> ps = (mk(p.p00[0], p.p00[1], p.p00[2]) + mk(p.du[0], p.du[1], p.du[2]) * ((R)i + ox)) +
                           mk(p.dv[0], p.dv[1], p.dv[2]) * ((R)j + oy);
                const V3<R> center = mk(p.center[0], p.center[1], p.center[2]);
                V3<R> origin = center;
                if (p.defocus) {
                    V3<R> qd = unit_disk<R>(g);
                    origin = (center + mk(p.disk_u[0], p.disk_u[1], p.disk_u[2]) * qd.x) +
                             mk(p.disk_v[0], p.disk_v[1], p.disk_v[2]) * qd.z;
                }
                o = origin;
                d = ps - origin;
            }
            // ---- world.hit(&r, EPSILON..=INFINITY): closest over all primitives, the
            // lowest id on equal t (hit_rays_kernel's)
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
                query_closest_steal<kRobust>(scw, sbase, o, d, tmin, tb, best, stk_wave, lane, steal_area, nvis,
                                             ntest, !live);
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
            R f[kFeatureChannels];
            uint32_t m = 0;
            if (best < 0) {   // a miss: the camera's background, +0 elsewhere
                f[0] = p.bg[0];
                f[1] = p.bg[1];
                f[2] = p.bg[2];
#pragma unroll
                for (int q = 3; q < (int)kFeatureChannels; ++q) f[q] = (R)0;
            } else {
                cnt[kQcHits] += 1;
                // ---- HitRecord::new, hittable.rs:101-129 (hit_rays_kernel's; the UVs only
                // where a texture reads them)
                const bool tex = p.sc.mat_tex != nullptr;
                V3<R> pnt = o + d * tb;
                V3<R> outward;
                R hu = (R)0, hv = (R)0;
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
                    if (tex) {
                        const V3<R> pq = po - q3(Q, 0);                // get_quad_uv, object space
                        hu = dot(cross(pq, q3(Q, 6)), q3(Q, 9));
                        hv = dot(cross(q3(Q, 3), pq), q3(Q, 9));
                    }
                    m = p.sc.box_mat[best - bbase];
                } else if (best < nplanes) {
                    const R* pl = p.sc.planes + kPlaneR * best;
                    outward = mk(pl[3], pl[4], pl[5]);
                    front = dot(d, outward) < (R)0;
                    if (tex) plane_uv(pl, pnt, hu, hv);                // get_plane_uv, plane.rs:40-54
                    m = p.sc.plane_mat[best];
                } else if (best < bbase) {
                    const R* Q = p.sc.quads + kQuadR * (best - nplanes);
                    outward = q3(Q, 12);                               // quadrilateral.rs:97
                    front = dot(d, outward) < (R)0;
                    if (tex) {
                        const V3<R> pq = pnt - q3(Q, 0);               // get_quad_uv, quadrilateral.rs:58-63
                        hu = dot(cross(pq, q3(Q, 6)), q3(Q, 9));
                        hv = dot(cross(q3(Q, 3), pq), q3(Q, 9));
                    }
                    m = p.sc.quad_mat[best - nplanes];
                } else {
                    const uint32_t sk_i = (uint32_t)(best - sbase);
                    const R4<R> sk = p.sc.sph[sk_i];
                    outward = PR::divs(pnt - mk(sk.x, sk.y, sk.z), p.sc.sph_r[sk_i]);   // sphere.rs:82-83
                    front = dot(d, outward) < (R)0;
                    if (tex) sphere_uv(outward, hu, hv);               // get_sphere_uv, sphere.rs:49-58
                    m = p.sc.sph_mat[sk_i] & 0xffffffu;
                }
                const V3<R> nrm = front ? outward : -outward;
                // the albedo by material: a Lambertian's and a DiffuseLight's texture at
                // (u, v, p) (material.rs:347-355, 508-514), a Metal's albedo, (1, 1, 1)
                // through a Dielectric, nothing from an Invisible
                const uint32_t mtype = p.sc.mat_type[m];
                const R4<R> mp = p.sc.mat_p[m];
                V3<R> alb = mk(mp.x, mp.y, mp.z);
                if (mtype == kMatLambertian || mtype == kMatDiffuseLight) {
                    if (tex) alb = tex_colour(p.sc, p.sc.mat_tex[m], hu, hv, pnt);
                } else if (mtype == kMatDielectric) {
                    alb = mk<R>(1, 1, 1);
                } else if (mtype != kMatMetal) {
                    alb = mk<R>(0, 0, 0);
                }
                f[0] = alb.x;
                f[1] = alb.y;
                f[2] = alb.z;
                f[3] = nrm.x;
                f[4] = nrm.y;
                f[5] = nrm.z;
                f[6] = ray_distance(d, tb);
                f[7] = (R)1;
            }
            // the reference's fold: acc = acc + f, sample after sample
#pragma unroll
            for (int q = 0; q < (int)kFeatureChannels; ++q) acc[q] = acc[q] + (double)f[q];
            if (s == 0 && p.ids) {
                p.ids[2 * pix] = best;
                p.ids[2 * pix + 1] = (int32_t)m;
            }
        }
        // the pixel's 64 bytes, in 16-byte stores.  A call that starts at sample 0
        // defines every pixel (one without samples: zeros); a later window leaves
        // the pixels it adds nothing to as they are.
        if (inside && (mine || p.first == 0)) {
#pragma unroll
            for (int q = 0; q < (int)kFeatureChannels / 2; ++q) out[q] = make_double2(acc[2 * q], acc[2 * q + 1]);
        }
    }
    query_counters_flush(smem, p.counters, cnt);
}

}  // namespace dev

}  // namespace rtw
