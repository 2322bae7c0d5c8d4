// ambient_kernel.hpp -- ambient occlusion as one query, one (point, sample) pair
// per lane:
//   ambient_kernel<R, world, robust>   for a point {p, normal} and the samples
//                                      s = first_sample .. first_sample + S - 1: the two draws
//                                      of CosinePdf::new(normal).generate(rng) (pdf.rs:38-52,
//                                      onb.rs:8-35, utils.rs:146-161), world.hit of {p, d} over
//                                      t_min..=t_max as occlusion_kernel answers it, and the
//                                      count of the pairs nothing blocks
// Every piece is a device function of the other queries, called as it is:
// mixture_direction's cosine lobe (rtw_device.hpp), occlusion_kernel's gates
// (aabb_hit_range), primitive tests, AnyTester and traversals (nee_kernel.hpp,
// bvh_traverse.hpp).  As in direct_kernel.hpp and features_kernel.hpp only the
// staging of kWorldLds / kWorldBvhLds into LDS is restated, because sharing it
// would change those kernels' code.
//
// The answer is an integer count, and integer adds commute: a point's samples
// are spread over lanes, not looped in one.  Pair q = k * S + j is flattened, 256
// pairs a block, so a point's samples sit in adjacent lanes and share an origin,
// and a lane that exits early costs one pair.  k and j come from one division
// of the wave's first pair index a block, then increments (carrying k and j across
// the grid-stride loop instead was measured and was no faster).
//
// The reduction: the wave ballots its open lanes; a lane is its segment's leader
// when it is lane 0 or the first sample of its point (its k differs from the
// lane below exactly then: j == 0, so no cross-lane read is needed); the leader
// counts the ballot's bits under its segment's mask and adds them to open[k]
// with one atomic whose result is not read.  One atomic a wave when S >= 64,
// at most 64 when S = 1.  The host zeroes `open` before the launch unless the
// call continues it.
//
// The wave-wide traversals need the whole wave in every trip: a lane past the
// end, or on a skipped point (a zero normal), goes along without a ray.
#pragma once

#include "ambient_kernels.h"
#include "nee_kernel.hpp"
#include "path_kernel.hpp"   // load_rec / store_rec

namespace rtw {

namespace dev {

template <typename R, int kWorld, bool kRobust>
__global__ void __launch_bounds__(kQueryBlock) ambient_kernel(const AParams<R> p) {
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
    const R tmin = p.tmin, tmax = p.tmax;
    const int32_t nplanes = (int32_t)p.sc.n_planes, nquads = (int32_t)p.sc.n_quads;
    const int32_t sbase = nplanes + nquads + (int32_t)p.sc.n_boxes;
    const uint32_t S = p.n_samples;
    const uint64_t n_pairs = p.n * S;   // (the host bounds the product)
    unsigned long long cnt[kQueryCounters] = {};

    // a workgroup takes pair blocks grid-stride: the staging above is paid once
    const uint64_t n_blocks = (n_pairs + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        // ---- the pair: one 64-bit division of the wave's first pair index, then increments
        const uint64_t q0 = blk * kQueryBlock + (uint32_t)__builtin_amdgcn_readfirstlane((int)wave) * 64u;
        uint64_t k = q0 / S, j = q0 - k * S;
        if (S >= 64u) {
            j += lane;                       // (at most one point ends within the wave's reach)
            if (j >= S) {
                j -= S;
                k += 1;
            }
        } else {
            const uint32_t t = (uint32_t)j + lane, dq = t / S;   // t < 127
            k += dq;
            j = t - dq * S;
        }
        const uint64_t q = q0 + lane;
        const bool in_range = q < n_pairs;
        R pt[6] = {};
        if (in_range) load_rec<record_align(6 * sizeof(R))>(p.points + 6 * k, pt);
        const V3<R> nrm = mk(pt[3], pt[4], pt[5]);
        // a normal of exactly (0, 0, 0) -- a miss row of rtw_hit_rays -- is no shading
        // point: no draws, no traversal, its count untouched, its records 0
        const bool live = in_range && !(nrm.x == (R)0 && nrm.y == (R)0 && nrm.z == (R)0);
        // a lane without a pair carries a NaN ray: it hits nothing, and the traversals skip it
        V3<R> o = mk((R)NAN, (R)NAN, (R)NAN), d = o;
        if (live) {
            // ---- CosinePdf::new(normal).generate(rng): the stream's first two draws
            o = mk(pt[0], pt[1], pt[2]);
            Rng g;
            g.seed(p.seed, p.first_stream + k, (uint64_t)p.first_sample + j);
            d = mixture_direction<R>(false, nrm, o, (R)0, o, g);
        }
        // ---- world.hit(&{p, d}, t_min..=t_max).is_some(): occlusion_kernel's body
        // an empty or NaN range, a NaN ray, a lane without a pair: nothing to test, 0
        const bool trace = live && tmax >= tmin && !ray_nan(o, d);
        bool blocked = false;
        if (trace) {
            for (int32_t i = 0; i < nplanes && !blocked; ++i) {
                R t;
                const R* pl = p.sc.planes + kPlaneR * i;
                blocked = aabb_hit_range(pl + 6, pl + 9, o, d, tmin, tmax) && plane_t(pl, o, d, tmin, t, nullptr) &&
                          t <= tmax;
            }
            for (int32_t i = 0; i < nquads && !blocked; ++i) {
                R t;
                const R* Q = p.sc.quads + kQuadR * i;
                blocked = aabb_hit_range(Q + 16, Q + 19, o, d, tmin, tmax) && quad_t_hit(Q, o, d, tmin, tmax, t);
            }
            for (int32_t i = 0; i < (int32_t)p.sc.n_boxes && !blocked; ++i) {
                R t;
                int qd;
                V3<R> o2, d2;
                const R* B = p.sc.boxes + kBoxR * i;
                blocked = aabb_hit_range(B + kBoxLo, B + kBoxHi, o, d, tmin, tmax) &&
                          box_t_hit(B, o, d, tmin, tmax, t, qd, o2, d2);
            }
        }
        // ---- the spheres: only the lanes still open
        const bool walk = trace && !blocked;
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
        const bool occ = blocked || (walk && T.found);
        // ---- open[k] += !occ: the ballot under the segment's mask, one atomic a segment
        const unsigned long long open_lanes = __ballot(live && !occ);
        const bool leader = lane == 0 || j == 0;
        const unsigned long long leaders = __ballot(leader);
        if (leader && in_range) {
            const unsigned long long above = leaders & ~((2ull << lane) - 1ull);   // (lane 63: none)
            const unsigned long long upto = above ? (1ull << __builtin_ctzll(above)) - 1ull : ~0ull;
            const uint32_t add = (uint32_t)__popcll(open_lanes & upto & ~((1ull << lane) - 1ull));
            if (add) (void)atomicAdd(p.open + k, add);
        }
        if (!in_range) continue;
        if (live) {
            cnt[kQcRays] += 1;
            cnt[kQcHits] += occ ? 1 : 0;
        }
        if (p.directions) {
            const R rec[3] = {live ? d.x : (R)0, live ? d.y : (R)0, live ? d.z : (R)0};
            store_rec<record_align(3 * sizeof(R))>(p.directions + 3 * q, rec);
        }
        if (p.occluded) p.occluded[q] = live && occ ? (uint8_t)1 : (uint8_t)0;
    }
    query_counters_flush(smem, p.counters, cnt);
}

}  // namespace dev

}  // namespace rtw
