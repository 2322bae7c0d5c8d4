// direct_kernel.hpp -- direct lighting as one query, one shading point per lane:
//   direct_light_kernel<R, world, robust>   for a point {p, normal} and the samples
//                                           s = first_sample .. first_sample + S - 1:
//                                           lights.random(p, rng) and lights.pdf_value(p, d)
//                                           (hittable_list.rs:408-419), world.hit of {p, d} over
//                                           t_min..=INFINITY, Material::emitted of what it meets,
//                                           Lambertian::scattering_pdf (material.rs:372-375), and
//                                           the fold of emitted * scattering_pdf / pdf in f64
// That is the light half of the reference's Lambertian bounce followed by the next
// segment's emission (camera.rs:480-521).  Every piece is a device function of the
// other queries, called as it is: light_sample_kernel's draws (sphere_random /
// quad_random), light_list_pdf (path_kernel.hpp) over the four light paths,
// hit_rays_kernel's primitive tests and traversals, shade_rays_kernel's emitted
// (tex_colour).  As in features_kernel.hpp two pieces of hit_rays_kernel's body are
// restated, because sharing them would change that kernel's code: the staging of
// kWorldLds / kWorldBvhLds into LDS and the hit record (here only what emitted reads:
// the hit point, and u, v of a textured emitter).
//
// The light path is a wave-uniform runtime switch (DParams::light_path), not a
// template axis: one kernel per closest-hit kernel.  The light BVH's per-lane stacks
// lie behind the closest hit's LDS (direct_kernels.h direct_lds).
//
// The stealing traversal and the wave-wide loops need the whole wave in every trip:
// every lane of a block runs the S trips, and a lane that is out of range or skipped
// (a zero normal) goes along without a ray, as primary_features_kernel's lanes do.
// The S samples of a point stay in registers: `direct` is read at most once and
// written once per point.
#pragma once

#include "direct_kernels.h"
#include "path_kernel.hpp"

namespace rtw {

namespace dev {

template <typename R, int kWorld, bool kRobust>
__global__ void __launch_bounds__(kQueryBlock) direct_light_kernel(const DParams<R> p) {
    using PR = P<R>;
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
    int32_t* const stk_wave = reinterpret_cast<int32_t*>(smem) + wave * p.stack * 64;
    unsigned char* const steal_area =
        smem + (size_t)kQueryWaves * p.stack * 64 * sizeof(int32_t) + wave * kStealLdsPerWave<R>;
    // the light BVH's stacks, laid out as light_pdf_rays_kernel's
    int32_t* const lstk = reinterpret_cast<int32_t*>(smem + p.light_off) + wave * p.light_stack * 64 + lane;
    (void)stk_wave;
    (void)steal_area;
    const R tmin = p.tmin;
    const int32_t nplanes = (int32_t)p.sc.n_planes, nquads = (int32_t)p.sc.n_quads;
    const int32_t bbase = nplanes + nquads;                  // object ids: planes, quads,
    const int32_t sbase = bbase + (int32_t)p.sc.n_boxes;     // cuboids, spheres
    const int32_t light_path = p.light_path;
    const uint32_t S = p.n_samples;
    unsigned long long cnt[kQueryCounters] = {};

    // a workgroup takes point blocks grid-stride: the staging above is paid once
    const uint64_t n_blocks = (p.n + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t k = blk * kQueryBlock + threadIdx.x;
        const bool in_range = k < p.n;
        R pt[6] = {};
        if (in_range) load_rec<record_align(6 * sizeof(R))>(p.points + 6 * k, pt);
        const V3<R> o = mk(pt[0], pt[1], pt[2]), nrm = mk(pt[3], pt[4], pt[5]);
        // a normal of exactly (0, 0, 0) -- a miss row of rtw_hit_rays -- is no shading
        // point: no draws, no traversal, its sums untouched, its records 0
        const bool live = in_range && !(nrm.x == (R)0 && nrm.y == (R)0 && nrm.z == (R)0);
        double acc[3] = {0.0, 0.0, 0.0};
        if (live && p.accumulate) {
            const double* a = p.direct + 3 * k;
            acc[0] = a[0], acc[1] = a[1], acc[2] = a[2];
        }
        for (uint32_t j = 0; j < S; ++j) {
            // a lane without a point carries a NaN ray: it hits nothing, and the per-lane
            // traversals skip it (bvh_dispatch: ray_nan)
            V3<R> d = mk((R)NAN, (R)NAN, (R)NAN);
            const V3<R> ro = live ? o : d;
            uint32_t idx = 0;
            R lpdf = (R)0;
            if (live) {
                // ---- lights.random(p, rng), light_sample_kernel's draws from the stream's start
                Rng g;
                g.seed(p.seed, p.first_stream + k, (uint64_t)p.first_sample + j);
                idx = g.index(p.sc.n_list);   // (the host refuses an empty list)
                const uint32_t ref = p.sc.lref ? p.sc.lref[idx] : idx;
                if (ref & kLrefQuad) {
                    d = quad_random(p.sc.lquads + kQuadR * (ref & 0x3fffffffu), o, g);
                } else if (ref & kLrefDefault) {
                    d = mk<R>(1, 0, 0);                      // Hittable::random default
                } else {
                    const R4<R> L = p.sc.lights[ref];
                    d = sphere_random(mk(L.x, L.y, L.z), L.w, o, g);
                }
                // ---- lights.pdf_value(p, d), light_pdf_rays_kernel's on the plan's path
                uint32_t tests = 0;
                if (light_path == kLightMixed) lpdf = light_list_pdf<R, kLightMixed, kRobust>(p.sc, o, d, lstk, tests);
                else if (light_path == kLightGrid) lpdf = light_list_pdf<R, kLightGrid, kRobust>(p.sc, o, d, lstk, tests);
                else if (light_path == kLightBvh) lpdf = light_list_pdf<R, kLightBvh, kRobust>(p.sc, o, d, lstk, tests);
                else lpdf = light_list_pdf<R, kLightLinear, kRobust>(p.sc, o, d, lstk, tests);
                cnt[kQcLightTests] += tests;
            }
            // ---- world.hit(&{p, d}, t_min..=INFINITY): hit_rays_kernel's closest hit
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
                query_closest_steal<kRobust>(scw, sbase, ro, d, tmin, tb, best, stk_wave, lane, steal_area, nvis,
                                             ntest, !live);
            } else if constexpr (kWorld >= kWorldBvh) {
                bvh_closest<kWorld, kRobust>(scw, sbase, ro, d, tmin, tb, best, stk_wave + lane, nvis, ntest, -1);
            } else {
                if (live) {
                    sweep_spheres<kRobust>(sph, p.sc.n_sph, sbase, o, d, tmin, tb, best);
                    ntest = p.sc.n_sph;
                }
            }
            cnt[kQcNodeVisits] += nvis;
            cnt[kQcSphereTests] += ntest;
            if (!in_range) continue;
            const bool hit = live && best >= 0;
            // ---- Material::emitted at the record's (u, v, p): shade_rays_kernel's
            uint32_t m = 0;
            V3<R> Le = mk<R>(0, 0, 0);
            if (hit) {
                if (best >= bbase && best < sbase) m = p.sc.box_mat[best - bbase];
                else if (best < nplanes) m = p.sc.plane_mat[best];
                else if (best < bbase) m = p.sc.quad_mat[best - nplanes];
                else m = p.sc.sph_mat[best - sbase] & 0xffffffu;
                if (m < p.sc.n_mat && p.sc.mat_type[m] == kMatDiffuseLight) {
                    const R4<R> mp = p.sc.mat_p[m];
                    Le = mk(mp.x, mp.y, mp.z);
                    if (p.sc.mat_tex) {
                        // HitRecord::new's point and UVs (hittable.rs:101-129), as hit_rays_kernel
                        // writes them
                        V3<R> pnt = o + d * tb;
                        R hu = (R)0, hv = (R)0;
                        if (best >= bbase && best < sbase) {
                            const R* B = p.sc.boxes + kBoxR * (best - bbase);
                            R t2;
                            int qd = 0;
                            V3<R> o2, d2;
                            box_t_hit(B, o, d, tmin, (R)INFINITY, t2, qd, o2, d2);
                            const R* Q = B + kQuadR * qd;
                            const V3<R> po = o2 + d2 * t2;
                            pnt = mat3_mul(B + kBoxRot, po) + q3(B, kBoxT);
                            const V3<R> pq = po - q3(Q, 0);
                            hu = dot(cross(pq, q3(Q, 6)), q3(Q, 9));
                            hv = dot(cross(q3(Q, 3), pq), q3(Q, 9));
                        } else if (best < nplanes) {
                            plane_uv(p.sc.planes + kPlaneR * best, pnt, hu, hv);
                        } else if (best < bbase) {
                            const R* Q = p.sc.quads + kQuadR * (best - nplanes);
                            const V3<R> pq = pnt - q3(Q, 0);
                            hu = dot(cross(pq, q3(Q, 6)), q3(Q, 9));
                            hv = dot(cross(q3(Q, 3), pq), q3(Q, 9));
                        } else {
                            const uint32_t s = (uint32_t)(best - sbase);
                            const R4<R> sk = p.sc.sph[s];
                            const V3<R> outward = PR::divs(pnt - mk(sk.x, sk.y, sk.z), p.sc.sph_r[s]);
                            sphere_uv(outward, hu, hv);
                        }
                        Le = tex_colour(p.sc, p.sc.mat_tex[m], hu, hv, pnt);
                    }
                }
            }
            // ---- Lambertian::scattering_pdf (material.rs:372-375, path_kernel.hpp's form),
            // the term and the fold
            R spdf = (R)0;
            V3<R> term = mk<R>(0, 0, 0);
            bool adds = false;
            if (live) {
                spdf = PR::max_(PR::over_pi(dot(nrm, PR::normalize(d))), (R)0);
                adds = hit && lpdf > (R)0 && spdf > (R)0;   // (false for NaN)
                if (adds) {
                    term = PR::divs(Le * spdf, lpdf);
                    acc[0] += (double)term.x;
                    acc[1] += (double)term.y;
                    acc[2] += (double)term.z;
                }
                cnt[kQcRays] += 1;
                cnt[kQcHits] += adds ? 1 : 0;
            }
            const uint64_t row = k * S + j;
            if (p.samples) {
                R rec[kDirectSampleValues] = {};
                if (live) {
                    rec[0] = d.x, rec[1] = d.y, rec[2] = d.z, rec[3] = lpdf;
                    rec[4] = hit ? tb : (R)0, rec[5] = spdf;
                    rec[6] = Le.x, rec[7] = Le.y, rec[8] = Le.z;
                    rec[9] = term.x, rec[10] = term.y, rec[11] = term.z;
                }
                store_rec<16>(p.samples + kDirectSampleValues * row, rec);
            }
            if (p.sample_ids) {
                const int32_t id[kDirectIdValues] = {(int32_t)idx, hit ? best : -1, (int32_t)m, adds ? 1 : 0};
                store_rec<16>(p.sample_ids + kDirectIdValues * row, id);
            }
        }
        if (live) {
            double* a = p.direct + 3 * k;
            a[0] = acc[0], a[1] = acc[1], a[2] = acc[2];
        }
    }
    query_counters_flush(smem, p.counters, cnt);
}

}  // namespace dev

}  // namespace rtw
