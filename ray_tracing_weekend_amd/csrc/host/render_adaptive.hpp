// render_adaptive.hpp -- adaptive sampling (rtw_render_adaptive): the pass plan
// -- where the sample passes end, how a pass is cut into sub-passes under the
// chunk-sum budget, the argument check -- and the stop rule itself, one inline
// function that the fold kernel (adaptive_kernels.hpp) and the host share.
// No HIP call is made here (rtw_kernels.h brings the __host__ __device__
// qualifiers): the CPU checks build it without a device.
//
// A pass ends at b_0 = min_samples, b_k = min(min_samples + k * window,
// max_samples); pass 0 renders samples [0, b_0) of every tile, pass k samples
// [b_(k-1), b_k) of the tiles still active, one sample per item.  After a pass
// that ends at n samples a pixel is settled when the standard error of its
// displayed value sqrt(mean luminance) is at most `tolerance`, written without
// sqrt or a quotient by the mean (adaptive_settled); a tile stops when all its
// pixels inside the image are settled, or at max_samples, and never resumes.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../../include/rtw.h"
#include "../rtw_kernels.h"
#include "render_plan.hpp"

namespace rtw {

// Y of one sample's value: ((0.2126 r) + (0.7152 g)) + (0.0722 b), every
// operation rounded on its own
__host__ __device__ inline double adaptive_luma(double r, double g, double b) {
#pragma clang fp contract(off)
    const double yr = 0.2126 * r, yg = 0.7152 * g, yb = 0.0722 * b;
    const double s = yr + yg;
    return s + yb;
}

// The stop rule of one pixel after n >= 2 samples: S1 = sum of Y, S2 = sum of
// Y * Y in sample order.  A sum that is not finite is settled: more samples
// cannot repair it.  Else the variance of the mean, var / (n - 1), against
// (2 tolerance)^2 * mean -- the standard error of sqrt(mean) to first order --
// with the mean floored at 2^-16 (one 8-bit level, squared).
__host__ __device__ inline bool adaptive_settled(double S1, double S2, uint32_t n, double tolerance) {
#pragma clang fp contract(off)
    if (!__builtin_isfinite(S1) || !__builtin_isfinite(S2)) return true;
    const double nn = (double)n;
    const double m = S1 / nn;
    const double q = S2 / nn;
    const double mm = m * m;
    const double var = fmax(q - mm, 0.0);
    const double v = var / (nn - 1.0);
    const double t4 = 4.0 * tolerance;
    const double t = t4 * tolerance;
    const double bound = t * fmax(m, 0x1p-16);
    return v <= bound;
}

// rtw_render_adaptive's scalar arguments (chunk: the explicit rtw_set_chunk, 0
// = none): null, or what is wrong with them
inline const char* adaptive_check(uint32_t min_samples, uint32_t max_samples, uint32_t window, double tolerance,
                                  uint32_t chunk) {
    if (min_samples < 2) return "min_samples must be at least 2";
    if (max_samples < min_samples) return "max_samples is below min_samples";
    if (window == 0) return "window must be at least 1";
    if (!__builtin_isfinite(tolerance) || tolerance < 0.0) return "tolerance must be finite and not negative";
    if (chunk > 1) return "adaptive sampling renders one sample per item: rtw_set_chunk above 1";
    return nullptr;
}

// passes of an adaptive render that no tile leaves early
inline uint32_t adaptive_passes(uint32_t min_samples, uint32_t max_samples, uint32_t window) {
    return 1u + (uint32_t)(((uint64_t)(max_samples - min_samples) + window - 1) / window);
}

// the sample index pass k ends at
inline uint32_t adaptive_pass_end(uint32_t min_samples, uint32_t max_samples, uint32_t window, uint32_t k) {
    return (uint32_t)std::min<uint64_t>((uint64_t)min_samples + (uint64_t)k * window, max_samples);
}

// The most samples one sub-pass of n_tiles active tiles may hold: their chunk
// sums (one per sample) stay within partial_max and half of dev_total (0:
// unknown), plan_chunk's budget; at least one.
template <typename R>
inline uint32_t adaptive_sub_samples(const RenderKnobs& k, uint32_t n_tiles, size_t dev_total) {
    size_t budget = k.partial_max;
    if (dev_total) budget = std::min(budget, dev_total / 2);
    const size_t per_sample = std::max<size_t>((size_t)n_tiles * 64 * 3 * sizeof(R), 1);
    return (uint32_t)std::min<size_t>(std::max<size_t>(budget / per_sample, 1), 0xFFFFFFFFu);
}

}  // namespace rtw
