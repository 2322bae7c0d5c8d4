// radiance_kernel.hpp -- incoming radiance along arbitrary rays as one query, one
// ray per lane:
//   radiance_kernel<R, world, robust>   for a ray {origin, direction} and the samples
//                                       s = first_sample .. first_sample + S - 1:
//                                       Camera::ray_colour_tail_call (camera.rs:460-522) run
//                                       to the end of the path -- world.hit, HitRecord::new,
//                                       emitted, scatter, the MixturePdf bounce, the fold of
//                                       mult and res -- and the sample colours summed in f64
// That is the loop of rtw_hit_rays, rtw_shade_rays and rtw_path_advance with every
// record kept in registers.  Every piece is a device function of those queries,
// called as it is: hit_rays_kernel's primitive tests and traversals, shade_rays_kernel's
// tex_colour, specular_dir64, mixture_direction, quad_random and light_list_pdf
// (path_kernel.hpp) over the four light paths.  As in features_kernel.hpp and
// direct_kernel.hpp the pieces that are kernel bodies are restated, because sharing
// them would change those kernels' code: hit_rays_kernel's staging of kWorldLds /
// kWorldBvhLds into LDS and its hit record (point, normal, front face, u, v),
// shade_rays_kernel's bounce and path_advance_kernel's fold.
//
// The light path is a wave-uniform runtime switch (RParams::light_path), as in
// direct_light_kernel; the light BVH's per-lane stacks lie behind the closest hit's
// LDS (radiance_kernels.h radiance_lds).
//
// Shape: a trip of the loop traces one segment per lane.  The lane keeps its ray,
// its stream, mult, res, its sample index and the f64 sums in registers.  A lane
// whose path ended folds the colour and starts the path of its next sample for the
// following trip, so the lanes of a wave run out of phase and the wave stays full
// until its lanes run out of samples.  The stealing traversal needs the whole wave in
// every trip: a lane without a path goes along with a NaN ray, as direct_light_kernel's
// lanes do.  The loop's condition holds an explicit bound of S * max(max_depth, 1)
// trips (radiance_trip_bound): each path takes at most max(max_depth, 1), so the
// bound is never what ends a correct run, and a slip in the bookkeeping cannot spin.
// `radiance` is read at most once and written once per ray.
#pragma once

#include "path_kernel.hpp"
#include "radiance_kernels.h"

namespace rtw {

namespace dev {

// a * b + c with the product rounded before the add, in both precisions
// (path_advance_kernel's unit is built without contraction; the f32 unit of this
// kernel contracts within an expression)
template <typename R>
__device__ __forceinline__ R mul_round_add(R a, R b, R c) {
#pragma clang fp contract(off)
    const R ab = a * b;
    return ab + c;
}

template <typename R, int kWorld, bool kRobust>
__global__ void __launch_bounds__(kQueryBlock) radiance_kernel(const RParams<R> p) {
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
    const uint32_t S = p.n_samples, max_depth = p.max_depth;
    const uint64_t trip_bound = radiance_trip_bound(S, max_depth);
    const V3<R> zero = mk<R>(0, 0, 0);
    unsigned long long cnt[kQueryCounters] = {};

    // a workgroup takes ray blocks grid-stride: the staging above is paid once
    const uint64_t n_blocks = (p.n + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t k = blk * kQueryBlock + threadIdx.x;
        const bool in_range = k < p.n;
        double acc[3] = {0.0, 0.0, 0.0};
        if (in_range && p.accumulate) {
            const double* a = p.radiance + 3 * k;
            acc[0] = a[0], acc[1] = a[1], acc[2] = a[2];
        }
        // ---- the lane's path: ray, stream, mult, res, rounds done, sample index
        V3<R> o = zero, d = zero, mult = zero, res = zero;
        Rng g = {0, 0, 0, 0};
        uint32_t depth = 0, j = 0;
        bool has = in_range;   // a path is running
        // the path of sample j from its start: mult = 1, res = 0, the caller's ray, and the
        // stream of (seed, first_stream + k, first_sample + j) or the caller's state
        auto begin = [&]() {
            R ray[6];
            load_rec<record_align(6 * sizeof(R))>(p.rays + 6 * k, ray);
            o = mk(ray[0], ray[1], ray[2]);
            d = mk(ray[3], ray[4], ray[5]);
            mult = mk<R>(1, 1, 1);
            res = zero;
            depth = 0;
            if (p.rng) {
                uint64_t st[4];
                load_rec<16>(p.rng + 4 * k, st);
                g.s0 = st[0], g.s1 = st[1], g.s2 = st[2], g.s3 = st[3];
            } else {
                g.seed(p.seed, p.first_stream + k, (uint64_t)p.first_sample + j);
            }
        };
        if (has) begin();
        // The condition is wave-uniform: `trip` and the bound are, and the ballot is taken with
        // the whole wave active -- both `continue`s below lead to the loop's latch, where the
        // lanes reconverge before the header is evaluated again, so every lane of the wave
        // leaves the loop on the same trip.  No block barrier lies inside the loop.
        for (uint64_t trip = 0; trip < trip_bound && __ballot(has) != 0ull; ++trip) {
            // a lane without a segment to trace carries a NaN ray: it hits nothing, and the
            // per-lane traversals skip it (bvh_dispatch: ray_nan)
            const bool live = has && max_depth > 0;
            V3<R> ro = mk((R)NAN, (R)NAN, (R)NAN), rd = ro;
            if (live) ro = o, rd = d;
            // ---- world.hit(&r, t_min..=INFINITY): hit_rays_kernel's closest hit
            R tb = (R)INFINITY;
            int32_t best = -1;
            if (live) {
                for (int32_t q = 0; q < nplanes; ++q) {
                    R t;
                    const R* pl = p.sc.planes + kPlaneR * q;
                    if (aabb_hit_plane(pl + 6, pl + 9, ro, rd, tmin) && plane_t(pl, ro, rd, tmin, t, nullptr) &&
                        (best < 0 || t < tb)) {
                        tb = t;
                        best = q;
                    }
                }
                for (int32_t q = 0; q < nquads; ++q) {
                    R t;
                    const R* Q = p.sc.quads + kQuadR * q;
                    if (aabb_hit_ref(Q + 16, Q + 19, ro, rd, tmin) && quad_t_hit(Q, ro, rd, tmin, (R)INFINITY, t) &&
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
                    if (aabb_hit_ref(B + kBoxLo, B + kBoxHi, ro, rd, tmin) &&
                        box_t_hit(B, ro, rd, tmin, (R)INFINITY, t, qd, o2, d2) && (best < 0 || t < tb)) {
                        tb = t;
                        best = bbase + q;
                    }
                }
            }
            uint32_t nvis = 0, ntest = 0;
            if constexpr (kWorld == kWorldBvhLds) {
                // wave-wide: every lane enters, the ones without a ray as thieves
                query_closest_steal<kRobust>(scw, sbase, ro, rd, tmin, tb, best, stk_wave, lane, steal_area, nvis,
                                             ntest, !live);
            } else if constexpr (kWorld >= kWorldBvh) {
                bvh_closest<kWorld, kRobust>(scw, sbase, ro, rd, tmin, tb, best, stk_wave + lane, nvis, ntest, -1);
            } else {
                if (live) {
                    sweep_spheres<kRobust>(sph, p.sc.n_sph, sbase, ro, rd, tmin, tb, best);
                    ntest = p.sc.n_sph;
                }
            }
            cnt[kQcNodeVisits] += nvis;
            cnt[kQcSphereTests] += ntest;
            if (!has) continue;
            V3<R> colour = zero;
            bool ended = true;
            if (!live) {
                colour = zero + res;   // max_depth == 0: 0 + 0, nothing traced
            } else {
                cnt[kQcRays] += 1;
                depth += 1;
                // ---- HitRecord::new, hittable.rs:101-129 (hit_rays_kernel's record; a miss
                // is object -1 and every other field 0)
                V3<R> pnt = zero, nrm = zero;
                R hu = (R)0, hv = (R)0;
                uint32_t m = 0;
                bool front = false;
                if (best >= 0) {
                    V3<R> outward;
                    pnt = o + d * tb;
                    if (best >= bbase && best < sbase) {
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
                        const V3<R> pq = po - q3(Q, 0);
                        hu = dot(cross(pq, q3(Q, 6)), q3(Q, 9));
                        hv = dot(cross(q3(Q, 3), pq), q3(Q, 9));
                        m = p.sc.box_mat[best - bbase];
                    } else if (best < nplanes) {
                        const R* pl = p.sc.planes + kPlaneR * best;
                        outward = mk(pl[3], pl[4], pl[5]);
                        front = dot(d, outward) < (R)0;
                        plane_uv(pl, pnt, hu, hv);
                        m = p.sc.plane_mat[best];
                    } else if (best < bbase) {
                        const R* Q = p.sc.quads + kQuadR * (best - nplanes);
                        outward = q3(Q, 12);
                        front = dot(d, outward) < (R)0;
                        const V3<R> pq = pnt - q3(Q, 0);
                        hu = dot(cross(pq, q3(Q, 6)), q3(Q, 9));
                        hv = dot(cross(q3(Q, 3), pq), q3(Q, 9));
                        m = p.sc.quad_mat[best - nplanes];
                    } else {
                        const uint32_t s = (uint32_t)(best - sbase);
                        const R4<R> sk = p.sc.sph[s];
                        outward = PR::divs(pnt - mk(sk.x, sk.y, sk.z), p.sc.sph_r[s]);
                        front = dot(d, outward) < (R)0;
                        sphere_uv(outward, hu, hv);
                        m = p.sc.sph_mat[s] & 0xffffffu;
                    }
                    nrm = front ? outward : -outward;
                }
                // ---- shade_rays_kernel's bounce on that record.  A material id that is not
                // the scene's is answered as a miss: no table is read out of bounds
                const bool hit = best >= 0 && m < p.sc.n_mat;
                uint32_t mtype = kMatInvisible;
                R4<R> mp = R4<R>{0, 0, 0, 0};
                if (hit) {
                    // four zero words are no xoshiro256++ state: the stream of (0, 0, 0) instead,
                    // from the first hit on, as rtw_shade_rays (a miss leaves the state untouched)
                    if ((g.s0 | g.s1 | g.s2 | g.s3) == 0) g.seed(0, 0, 0);
                    mtype = p.sc.mat_type[m];
                    mp = p.sc.mat_p[m];
                } else {
                    m = 0;
                }
                V3<R> mcol = mk(mp.x, mp.y, mp.z);
                if (p.sc.mat_tex && (mtype == kMatDiffuseLight || mtype == kMatLambertian))
                    mcol = tex_colour(p.sc, p.sc.mat_tex[m], hu, hv, pnt);
                const V3<R> emitted = mtype == kMatDiffuseLight ? mcol : zero;
                int32_t event = hit ? kEventAbsorbed : kEventMiss;
                V3<R> dir = zero, weight = zero;
                if (mtype == kMatMetal || mtype == kMatDielectric) {
                    const bool metal = mtype == kMatMetal;
                    bool keep = true;
                    if constexpr (sizeof(R) == 8) {
                        dir = specular_dir64<true>(metal, to64(d), to64(nrm), front, p.sc.mat64[m], g, keep);
                    } else if (metal) {
                        const V3<R> refl = reflect(PR::normalize(d), nrm);
                        dir = refl + unit_sphere<R>(g) * mp.w;
                        keep = dot(dir, nrm) > (R)0;
                    } else {
                        const R ratio = front ? PR::div_((R)1, mp.w) : mp.w;
                        const V3<R> unit = PR::normalize(d);
                        const R cos_t = PR::min_(dot(unit, -nrm), (R)1);
                        const R sin_t = PR::sqrt_((R)1 - cos_t * cos_t);
                        const bool cannot = ratio * sin_t > (R)1;
                        if (cannot || reflectance(cos_t, ratio) > PR::u_open01(g.next())) dir = reflect(unit, nrm);
                        else dir = refract(unit, nrm, ratio);
                    }
                    if (keep) {
                        event = kEventReflect;
                        weight = metal ? mk(mp.x, mp.y, mp.z) : mk<R>(1, 1, 1);
                    } else {
                        dir = zero;
                    }
                }
                const bool lamb = mtype == kMatLambertian;
                if (lamb) {
                    // MixturePdf(HittablePdf(lights), CosinePdf)::generate, shade_rays_kernel's draws
                    const bool to_light = PR::u_std(g.next()) < (R)0.5;
                    bool sampled = false;
                    R4<R> L = R4<R>{0, 0, 0, 0};
                    if (to_light) {   // (the host refuses an empty list)
                        const uint32_t idx = g.index(p.sc.n_list);
                        const uint32_t ref = p.sc.lref ? p.sc.lref[idx] : idx;
                        if (ref & kLrefQuad) {
                            dir = quad_random(p.sc.lquads + kQuadR * (ref & 0x3fffffffu), pnt, g);
                            sampled = true;
                        } else if (ref & kLrefDefault) {
                            dir = mk<R>(1, 0, 0);
                            sampled = true;
                        } else {
                            L = p.sc.lights[ref];
                        }
                    }
                    if (!sampled) dir = mixture_direction(to_light, nrm, mk(L.x, L.y, L.z), L.w, pnt, g);
                }
                // ---- the Lambertian lanes' light pdf, together, on the plan's path
                if (lamb) {
                    uint32_t tests = 0;
                    R lpdf;
                    if (light_path == kLightMixed) lpdf = light_list_pdf<R, kLightMixed, kRobust>(p.sc, pnt, dir, lstk, tests);
                    else if (light_path == kLightGrid) lpdf = light_list_pdf<R, kLightGrid, kRobust>(p.sc, pnt, dir, lstk, tests);
                    else if (light_path == kLightBvh) lpdf = light_list_pdf<R, kLightBvh, kRobust>(p.sc, pnt, dir, lstk, tests);
                    else lpdf = light_list_pdf<R, kLightLinear, kRobust>(p.sc, pnt, dir, lstk, tests);
                    cnt[kQcLightTests] += tests;
                    const V3<R> ndir = PR::normalize(dir);
                    const V3<R> wn = PR::normalize(nrm);
                    const R cos_w = PR::over_pi(dot(ndir, wn));
                    const R pdf = lpdf * (R)0.5 + PR::max_(cos_w, (R)0) * (R)0.5;
                    const R spdf = PR::max_(PR::over_pi(dot(nrm, ndir)), (R)0);
                    weight = PR::divs(mcol * spdf, pdf);
                    event = kEventScatter;
                    cnt[kQcHits] += 1;
                }
                // ---- path_advance_kernel's fold (camera.rs:470-521), every product rounded
                // before its add
                if (event >= kEventReflect) {
                    if (event == kEventScatter)
                        res = mk(mul_round_add(mult.x, emitted.x, res.x), mul_round_add(mult.y, emitted.y, res.y),
                                 mul_round_add(mult.z, emitted.z, res.z));
                    mult = mk(mult.x * weight.x, mult.y * weight.y, mult.z * weight.z);
                    o = pnt;
                    d = dir;
                    ended = depth >= max_depth;   // alive after max_depth rounds: 0 + res
                    if (ended) colour = zero + res;
                } else {
                    const V3<R> with = event == kEventMiss ? mk(p.bg[0], p.bg[1], p.bg[2]) : emitted;
                    colour = mk(mul_round_add(mult.x, with.x, res.x), mul_round_add(mult.y, with.y, res.y),
                                mul_round_add(mult.z, with.z, res.z));
                }
            }
            if (!ended) continue;
            // ---- the path's end: the fold, the records, the state; then the next sample's path
            acc[0] += (double)colour.x;
            acc[1] += (double)colour.y;
            acc[2] += (double)colour.z;
            const uint64_t row = k * S + j;
            if (p.colours) {
                const R c3[3] = {colour.x, colour.y, colour.z};
                store_rec<record_align(3 * sizeof(R))>(p.colours + 3 * row, c3);
            }
            if (p.segments) p.segments[row] = depth;
            if (p.rng) {
                const uint64_t st[4] = {g.s0, g.s1, g.s2, g.s3};
                store_rec<16>(p.rng + 4 * k, st);
            }
            j += 1;
            has = j < S;
            if (has) begin();
        }
        if (in_range) {
            double* a = p.radiance + 3 * k;
            a[0] = acc[0], a[1] = acc[1], a[2] = acc[2];
        }
    }
    query_counters_flush(smem, p.counters, cnt);
}

}  // namespace dev

}  // namespace rtw
