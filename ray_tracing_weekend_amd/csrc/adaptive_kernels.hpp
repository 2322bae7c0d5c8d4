// adaptive_kernels.hpp -- the device side of adaptive sampling
// (rtw_render_adaptive; the rule: host/render_adaptive.hpp): between two
// sample passes of the render kernel, fold_adaptive_kernel folds the pass's
// chunk sums onto each pixel's f64 state and votes per tile,
// compact_tiles_kernel lists the tiles that go on, and at the end
// unpack_adaptive_kernel writes the image -- or, over the ranks of a
// multi-device context, pack_adaptive_kernel writes each rank's records for the
// gather and assemble_adaptive_kernel the image on rank 0.  Compiled by
// adaptive.hip alone, without FMA contraction in either precision: the
// statistic is f64 arithmetic whose every operation rounds on its own.
#pragma once

#include "host/render_adaptive.hpp"

namespace rtw {
namespace dev {

// chunks staged per pass of the fold, as reduce_chunks_kernel stages them
template <typename R>
constexpr uint32_t kAdaptiveFoldWin = sizeof(R) == 4 ? 16 : RTW_FOLD_WIN64;

// One wave per active tile, one lane per pixel.  The pass's chunk sums (one
// sample each) are those of fold_window_kernel: partial[(a * 64 + px) *
// n_chunks * 3], a = the tile's position in the active list; the state lives
// in the tile's stable slot T = list[a] (list null: a itself): sums[(T * 64 +
// px) * 3] and s12[(T * 64 + px) * 2] = {S1, S2}.  first == 0: the state starts
// from 0.  The colour sums take exactly fold_window_kernel's additions; Y and
// Y * Y of each sample go onto S1 and S2 in the same order.  A deciding
// (sub-)pass ends the pass at n_end samples: each lane evaluates
// adaptive_settled, the lanes inside the image vote, and lane 0 writes the
// tile's count and whether it goes on (it stops at `last`, the pass that ends
// at max_samples, whatever the vote).
template <typename R>
__global__ void __launch_bounds__(64) fold_adaptive_kernel(AdaptiveFold f) {
    constexpr uint32_t kFoldWin = kAdaptiveFoldWin<R>;
    constexpr uint32_t kFoldRow = kFoldWin * 3 + 1;    // LDS row (odd: no bank conflicts)
    __shared__ R win[64 * kFoldRow];
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const uint32_t T = f.list ? f.list[a] : a;
    const uint32_t tiles_x = (f.W + kTile - 1) / kTile;
    const uint32_t ty = T / tiles_x, tx = T - ty * tiles_x;
    const uint32_t i = tx * kTile + (lane & 7), j = ty * kTile + (lane >> 3);
    const size_t row_len = (size_t)f.n_chunks * 3;
    const R* tile = reinterpret_cast<const R*>(f.partial) + (size_t)a * 64 * row_len;
    double* acc = f.sums + ((size_t)T * 64 + lane) * 3;
    double* st = f.s12 + ((size_t)T * 64 + lane) * 2;
    double sx = 0, sy = 0, sz = 0, s1 = 0, s2 = 0;
    if (f.first) {
        sx = acc[0];
        sy = acc[1];
        sz = acc[2];
        s1 = st[0];
        s2 = st[1];
    }
    constexpr uint32_t kNv = kFoldWin * 3;
    for (uint32_t c0 = 0; c0 < f.n_chunks; c0 += kFoldWin) {
        const uint32_t kw = min(kFoldWin, f.n_chunks - c0), nv = kw * 3;
        const R* src = tile + (size_t)c0 * 3;
        if (kw == kFoldWin) {
            // full pass: every lane's kNv loads issued back to back
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
            const double r = (double)row[3 * k], g = (double)row[3 * k + 1], b = (double)row[3 * k + 2];
            sx = sx + r;
            sy = sy + g;
            sz = sz + b;
            const double y = adaptive_luma(r, g, b);
            const double yy = y * y;
            s1 = s1 + y;
            s2 = s2 + yy;
        }
        __syncthreads();
    }
    const bool inside = i < f.W && j < f.H;
    if (!inside) sx = sy = sz = s1 = s2 = 0;   // never written
    acc[0] = sx;
    acc[1] = sy;
    acc[2] = sz;
    st[0] = s1;
    st[1] = s2;
    if (f.decide) {
        // lanes outside the image do not vote
        const bool settled = !inside || adaptive_settled(s1, s2, f.n_end, f.tolerance);
        const bool all = __all(settled) != 0;
        if (lane == 0) {
            f.counts[T] = f.n_end;
            f.flags[T] = (all || f.last) ? 0u : 1u;
        }
    }
}

// The tiles that go on, in ascending tile order: one workgroup steps over the
// flags 256 at a time with a ballot scan (no atomic append: the list is the
// same every run), and writes the list, its length (meta[0]) and the pixels
// inside the image it covers (meta[1]).
__global__ void __launch_bounds__(256) compact_tiles_kernel(const uint32_t* __restrict__ flags, uint32_t n_tiles,
                                                            uint32_t W, uint32_t H, uint32_t* __restrict__ list,
                                                            uint32_t* __restrict__ meta) {
    __shared__ uint32_t wave_n[4];
    __shared__ uint32_t wave_px[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tiles_x = (W + kTile - 1) / kTile;
    uint32_t base_out = 0, px = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += 256) {
        const uint32_t T = t0 + tid;
        const bool on = T < n_tiles && flags[T] != 0;
        const unsigned long long m = __ballot(on);
        const uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_n[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = base_out, total = 0;
        for (uint32_t w = 0; w < 4; ++w) {
            if (w < wave) off += wave_n[w];
            total += wave_n[w];
        }
        if (on) {
            list[off + before] = T;
            const uint32_t ty = T / tiles_x, tx = T - ty * tiles_x;
            px += min(kTile, W - tx * kTile) * min(kTile, H - ty * kTile);
        }
        base_out += total;
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) px += __shfl_xor(px, o);
    if (lane == 0) wave_px[wave] = px;
    __syncthreads();
    if (tid == 0) {
        meta[0] = base_out;
        meta[1] = ((wave_px[0] + wave_px[1]) + wave_px[2]) + wave_px[3];
    }
}

// The slot-ordered state -> the image: sums [H][W][3] and counts [H][W] (every
// pixel of a tile has the tile's count); one thread per pixel slot.
__global__ void __launch_bounds__(256) unpack_adaptive_kernel(const double* __restrict__ sums,
                                                              const uint32_t* __restrict__ counts, uint32_t W,
                                                              uint32_t H, uint32_t n_tiles,
                                                              double* __restrict__ img,
                                                              uint32_t* __restrict__ img_counts) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t T = (uint32_t)(gid >> 6), lane = (uint32_t)gid & 63;
    if (T >= n_tiles) return;
    const uint32_t tiles_x = (W + kTile - 1) / kTile;
    const uint32_t ty = T / tiles_x, tx = T - ty * tiles_x;
    const uint32_t i = tx * kTile + (lane & 7), j = ty * kTile + (lane >> 3);
    if (i >= W || j >= H) return;
    const double* src = sums + ((size_t)T * 64 + lane) * 3;
    double* dst = img + ((size_t)j * W + i) * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    img_counts[(size_t)j * W + i] = counts[T];
}

// A rank of a multi-device render packs the tiles it owns for the gather: one
// wave per tile of `tiles` (ascending), each lane its pixel's three sums (24
// bytes, consecutive lanes consecutive); lane 0 adds the tile's count.  Copies
// only, no arithmetic.
__global__ void __launch_bounds__(64) pack_adaptive_kernel(const uint32_t* __restrict__ tiles,
                                                           const double* __restrict__ sums,
                                                           const uint32_t* __restrict__ counts,
                                                           double* __restrict__ records) {
    const uint32_t lt = blockIdx.x, lane = threadIdx.x;
    const uint32_t T = tiles[lt];
    const double* src = sums + ((size_t)T * 64 + lane) * 3;
    double* rec = records + (size_t)lt * kAdaptiveRecord;
    double* dst = rec + lane * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    if (lane == 0) {
        uint32_t* w = reinterpret_cast<uint32_t*>(rec + 64 * 3);
        w[0] = counts[T];
        w[1] = 0;
    }
}

// Rank 0 un-interleaves the ranks' gathered records into the image: one thread
// per pixel slot of every global tile T, decoded as assemble_tiles_kernel
// decodes it (v = slot[T], or T for the round robin: rank v % nranks, its
// local tile v / nranks).  Pixels outside the image are never written; every
// pixel of a tile gets the tile's count.
__global__ void __launch_bounds__(256) assemble_adaptive_kernel(const double* __restrict__ ranks, size_t rank_stride,
                                                                uint32_t nranks, uint32_t W, uint32_t H,
                                                                uint32_t tiles_x, uint32_t n_tiles,
                                                                const uint32_t* __restrict__ slot,
                                                                double* __restrict__ img,
                                                                uint32_t* __restrict__ img_counts) {
    const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
    const uint32_t T = gid >> 6, lane = gid & 63;
    if (T >= n_tiles) return;
    const uint32_t ty = T / tiles_x, tx = T - ty * tiles_x;
    const uint32_t i = tx * kTile + (lane & 7), j = ty * kTile + (lane >> 3);
    if (i >= W || j >= H) return;
    const uint32_t v = slot ? slot[T] : T;
    const uint32_t k = v % nranks, lt = v / nranks;
    const double* rec = ranks + k * rank_stride + (size_t)lt * kAdaptiveRecord;
    const double* src = rec + lane * 3;
    double* dst = img + ((size_t)j * W + i) * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    img_counts[(size_t)j * W + i] = reinterpret_cast<const uint32_t*>(rec + 64 * 3)[0];
}

}  // namespace dev
}  // namespace rtw
