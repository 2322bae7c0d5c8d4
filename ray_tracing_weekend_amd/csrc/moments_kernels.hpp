// moments_kernels.hpp -- the per-pixel luminance moments of a render
// (rtw_render_window_moments, rtw_adaptive_moments; include/rtw.h):
// fold_moments_kernel folds a pass's chunk sums -- one sample each -- onto the
// image-order f64 colour sums and {S1, S2}, with the additions of
// fold_adaptive_kernel (adaptive_kernels.hpp) and no vote; unpack_moments_kernel
// writes the {S1, S2} an adaptive render left in slot order as an image.
// Compiled by moments.hip alone, without FMA contraction in either precision, as
// the adaptive unit: the statistic is f64 arithmetic whose every operation
// rounds on its own.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host/render_adaptive.hpp"

namespace rtw {

struct MomentsFold {
    const void* partial;      // [n_tiles][64][n_chunks][3] of the context's precision, one sample per chunk
    uint32_t n_chunks;
    uint32_t n_tiles;         // every tile of the image, in tile order
    double* sums;             // [H][W][3] colour sums, image order
    double* moments;          // [H][W][2] {S1, S2} of the luminance, image order
    uint32_t first;           // the (sub-)pass's first sample (0: the state starts from 0)
    uint32_t W, H;
};
// each returns 0, or -1 when the launch failed
int launch_fold_moments(bool f64, const MomentsFold& f, hipStream_t stream);
// s12 [n_tiles][64][2] by tile -> image-order moments [H][W][2]
int launch_unpack_moments(const double* s12, uint32_t W, uint32_t H, double* img, hipStream_t stream);

#ifdef RTW_MOMENTS_KERNELS
namespace dev {

// chunks staged per pass of the fold, as fold_adaptive_kernel stages them
template <typename R>
constexpr uint32_t kMomentsFoldWin = sizeof(R) == 4 ? 16 : RTW_FOLD_WIN64;

// One wave per tile, one lane per pixel; the chunk sums are staged through LDS
// as fold_window_kernel and fold_adaptive_kernel stage them.  A lane inside the
// image continues its pixel's sums and {S1, S2} (from 0 when first == 0) in
// sample order: the colour sums take fold_window_kernel's additions at one
// sample per item, Y and Y * Y of each sample go onto S1 and S2.  A lane outside
// the image reads and writes no state.
template <typename R>
__global__ void __launch_bounds__(64) fold_moments_kernel(MomentsFold f) {
    constexpr uint32_t kFoldWin = kMomentsFoldWin<R>;
    constexpr uint32_t kFoldRow = kFoldWin * 3 + 1;    // LDS row (odd: no bank conflicts)
    __shared__ R win[64 * kFoldRow];
    const uint32_t T = blockIdx.x, lane = threadIdx.x;
    const uint32_t tiles_x = (f.W + kTile - 1) / kTile;
    const uint32_t ty = T / tiles_x, tx = T - ty * tiles_x;
    const uint32_t i = tx * kTile + (lane & 7), j = ty * kTile + (lane >> 3);
    const bool inside = i < f.W && j < f.H;
    const size_t row_len = (size_t)f.n_chunks * 3;
    const R* tile = reinterpret_cast<const R*>(f.partial) + (size_t)T * 64 * row_len;
    const size_t px = inside ? (size_t)j * f.W + i : 0;
    double* acc = f.sums + px * 3;
    double* st = f.moments + px * 2;
    double sx = 0, sy = 0, sz = 0, s1 = 0, s2 = 0;
    if (f.first && inside) {
        sx = acc[0];
        sy = acc[1];
        sz = acc[2];
        s1 = st[0];
        s2 = st[1];
    }
    for (uint32_t c0 = 0; c0 < f.n_chunks; c0 += kFoldWin) {
        const uint32_t kw = min(kFoldWin, f.n_chunks - c0), nv = kw * 3;
        const R* src = tile + (size_t)c0 * 3;
        for (uint32_t idx = lane; idx < 64 * nv; idx += 64) {
            const uint32_t r = idx / nv, col = idx - r * nv;
            win[r * kFoldRow + col] = src[r * row_len + col];
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
    if (!inside) return;
    acc[0] = sx;
    acc[1] = sy;
    acc[2] = sz;
    st[0] = s1;
    st[1] = s2;
}

// The slot-ordered {S1, S2} of an adaptive render -> the image; one thread per
// pixel slot, as unpack_adaptive_kernel.
__global__ void __launch_bounds__(256) unpack_moments_kernel(const double* __restrict__ s12, uint32_t W, uint32_t H,
                                                             uint32_t n_tiles, double* __restrict__ img) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t T = (uint32_t)(gid >> 6), lane = (uint32_t)gid & 63;
    if (T >= n_tiles) return;
    const uint32_t tiles_x = (W + kTile - 1) / kTile;
    const uint32_t ty = T / tiles_x, tx = T - ty * tiles_x;
    const uint32_t i = tx * kTile + (lane & 7), j = ty * kTile + (lane >> 3);
    if (i >= W || j >= H) return;
    const double* src = s12 + ((size_t)T * 64 + lane) * 2;
    double* dst = img + ((size_t)j * W + i) * 2;
    dst[0] = src[0];
    dst[1] = src[1];
}

}  // namespace dev
#endif  // RTW_MOMENTS_KERNELS

}  // namespace rtw
