// wavefront_kernel.hpp -- the bookkeeping of a wavefront path tracer's round,
// on the device, one path per lane:
//   path_begin_kernel<R>     mult = 1, res = 0, slot = first_slot + k
//   path_advance_kernel<R>   ray_colour_tail_call's fold of one round's events
//                            (camera.rs:470-521) and the stream compaction of the
//                            paths that go on
//   path_fold_kernel<R>      the batch's sample colours onto the f64 sums, in sample order
// Between closest hit and bounce (query_kernel.hpp, path_kernel.hpp) they make the
// loop of Renderer.render_wavefront without a host array operation: every
// component is computed in R, each product rounded before its add (the unit is
// built with -ffp-contract=off), so in f64 the colours are that loop's bits.
//
// Compaction: each wave counts its survivors with a ballot, the four counts are
// summed through LDS and the workgroup takes its place with ONE returning
// atomicAdd per block of kQueryBlock paths; a lane stores at base + the
// survivors before it.  The survivors of a block are contiguous and keep their
// order (a wave's rays stay coherent for the next traversal); the order of the
// blocks is whatever the atomics gave.  `slot` travels with the path, so nothing
// depends on a path's position.
// Memory: bandwidth-shaped, records through load_rec / store_rec at the widths
// record_align gives; no scene, no scratch, static LDS of a few words.
#pragma once

#include "path_kernel.hpp"
#include "wavefront_kernels.h"

namespace rtw {

namespace dev {

template <typename R>
__global__ void __launch_bounds__(kQueryBlock) path_begin_kernel(const PathBegin<R> p) {
    const uint64_t n_blocks = (p.n + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t k = blk * kQueryBlock + threadIdx.x;
        if (k >= p.n) continue;
        const R one[3] = {(R)1, (R)1, (R)1}, zero[3] = {(R)0, (R)0, (R)0};
        store_rec<record_align(3 * sizeof(R))>(p.mult + 3 * k, one);
        store_rec<record_align(3 * sizeof(R))>(p.res + 3 * k, zero);
        p.slot[k] = p.first_slot + (uint32_t)k;
    }
}

template <typename R>
__global__ void __launch_bounds__(kQueryBlock) path_advance_kernel(const PathAdvance<R> p) {
    __shared__ __attribute__((aligned(32))) unsigned char s_counters[kQueryLdsMin];
    __shared__ uint32_t s_wave[kQueryWaves];
    __shared__ unsigned long long s_base;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long cnt[kQueryCounters] = {};
    const uint64_t n_blocks = (p.n + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t k = blk * kQueryBlock + threadIdx.x;
        const bool live = k < p.n;
        bool keep = false;
        R m[3] = {}, r[3] = {};
        uint32_t slot = 0;
        if (live) {
            const int32_t ev = p.event[k];
            R w[3], e[3];
            load_rec<record_align(3 * sizeof(R))>(p.mult + 3 * k, m);
            load_rec<record_align(3 * sizeof(R))>(p.res + 3 * k, r);
            load_rec<record_align(3 * sizeof(R))>(p.weight + 3 * k, w);
            load_rec<record_align(3 * sizeof(R))>(p.emitted + 3 * k, e);
            slot = p.slot[k];
            R c[3];
            if (ev == kEventScatter || ev == kEventReflect) {
                keep = true;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    if (ev == kEventScatter) r[q] = r[q] + m[q] * e[q];   // camera.rs:519
                    m[q] = m[q] * w[q];                                   // camera.rs:496, 518
                }
                if (p.last) {   // alive after max_depth rounds, camera.rs:470-472
                    keep = false;
#pragma unroll
                    for (int q = 0; q < 3; ++q) c[q] = (R)0 + r[q];
                }
            } else {
                // MISS: the background (camera.rs:473-475); ABSORBED: the emission
                // (camera.rs:484-486); any other value: a miss into black
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const R with = ev == kEventMiss ? p.bg[q] : ev == kEventAbsorbed ? e[q] : (R)0;
                    c[q] = m[q] * with + r[q];
                }
            }
            if (!keep && (uint64_t)slot < p.colour_slots)
                store_rec<record_align(3 * sizeof(R))>(p.colour + 3 * (uint64_t)slot, c);
            cnt[kQcRays] += 1;
            cnt[kQcHits] += (p.count_scatter ? ev == kEventScatter : keep) ? 1 : 0;
        }
        // ---- the survivors' places: ballot, the waves' counts through LDS, one atomic
        const unsigned long long mask = __ballot(keep);
        const uint32_t before_lane = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t total = 0;
#pragma unroll
            for (uint32_t q = 0; q < kQueryWaves; ++q) total += s_wave[q];
            s_base = total ? atomicAdd(p.count, (unsigned long long)total) : 0ull;
        }
        __syncthreads();
        if (keep) {
            uint32_t before = before_lane;
            for (uint32_t q = 0; q < wave; ++q) before += s_wave[q];
            const uint64_t at = s_base + before;
            R nx[6];
            uint64_t st[4];
            load_rec<record_align(6 * sizeof(R))>(p.next + 6 * k, nx);
            load_rec<16>(p.rng + 4 * k, st);
            store_rec<record_align(6 * sizeof(R))>(p.out_rays + 6 * at, nx);
            store_rec<16>(p.out_rng + 4 * at, st);
            store_rec<record_align(3 * sizeof(R))>(p.out_mult + 3 * at, m);
            store_rec<record_align(3 * sizeof(R))>(p.out_res + 3 * at, r);
            p.out_slot[at] = slot;
        }
        __syncthreads();   // (s_wave and s_base are the next block's)
    }
    query_counters_flush(s_counters, p.counters, cnt);
}

template <typename R>
__global__ void __launch_bounds__(kQueryBlock) path_fold_kernel(const PathFold p) {
    const R* __restrict__ colour = reinterpret_cast<const R*>(p.colour);
    const uint64_t n_blocks = (p.n + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t i = blk * kQueryBlock + threadIdx.x;
        if (i >= p.n) continue;
        double s = p.sums[i];
        for (uint32_t b = 0; b < p.batch; ++b) s += (double)colour[(uint64_t)b * p.n + i];
        p.sums[i] = s;
    }
}

}  // namespace dev

}  // namespace rtw
