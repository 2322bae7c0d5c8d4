// denoise_variance_plan.hpp -- what a variance-guided denoise launches
// (rtw_denoise_variance; the filter is include/rtw.h's contract): the checked
// parameters, the per-iteration schedule of svgf_atrous_kernel (step, the
// staged or the direct form with its dynamic LDS, the grid) and the sizes of
// the state's buffers -- the three record arrays of rtw_denoise plus the
// ping-pong variance array.  Host only, no HIP call; of denoise_plan.hpp it
// takes the constants alone (the tile, the block, the record), none of its
// functions: capi_denoise_variance.cpp allocates and launches.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../../include/rtw.h"
#include "denoise_plan.hpp"

namespace rtw {

// a variance record: {ve, has_var (1 or 0)}, one 16-byte access
constexpr size_t kSvgfVarRecord = 16;
// what the staged form keeps per pixel of the tile and its halo: guide + colour + variance
constexpr size_t kSvgfLdsPerPixel = 2 * kDenoiseRecord + kSvgfVarRecord;
// tuning denoise_lds = 1: the steps up to this one are staged -- the old filter's
// choice (denoise_plan.hpp) until a measurement of this kernel says otherwise
constexpr uint32_t kSvgfLdsDefaultMaxStep = kDenoiseLdsDefaultMaxStep;
// the floor of the colour stop's variance: 2^-40
constexpr double kSvgfEps = 0x1p-40;

struct SvgfStep {
    uint32_t step = 1;        // 2^k
    uint32_t lds = 0;         // 1: the staged form
    size_t lds_bytes = 0;     // its dynamic LDS (0: direct)
    uint32_t grid_x = 0, grid_y = 0;
};

struct SvgfPlan {
    int err = RTW_OK;
    const char* err_text = "";
    rtw_denoise_variance_params params{};   // the checked parameters (the defaults for NULL)
    double sv2 = 0.0;                       // sigma_var * sigma_var
    uint64_t pixels = 0;
    uint32_t blocks = 0;                    // prepare / finish grid
    uint32_t iterations = 0;
    uint32_t lds_iterations = 0;            // ... of which staged
    SvgfStep steps[kDenoiseMaxIterations];
    // the state's buffers: guide, albedo, two colour record arrays, two variance arrays
    size_t record_bytes = 0;                // of one record array
    size_t var_bytes = 0;                   // of one variance array
    size_t state_bytes = 0;                 // of the six
    // the arrays of a call
    size_t sums_bytes_f32 = 0, sums_bytes_f64 = 0, features_bytes = 0, moments_bytes = 0, counts_bytes = 0,
           out_bytes = 0;
};

void denoise_variance_params_default(rtw_denoise_variance_params* out);

// dynamic LDS of the staged form at `step`: the tile and its 2 * step halo
size_t svgf_lds_bytes(uint32_t step);

// params NULL: the defaults.  has_counts false: spp is every pixel's count.
// denoise_lds: the tuning key (0 direct, 1 the default plan, 2 staged wherever it fits).
SvgfPlan plan_denoise_variance(const rtw_denoise_variance_params* params, uint32_t width, uint32_t height,
                               bool has_counts, uint32_t spp, uint32_t denoise_lds);

// The device form's arrays: "" when they can be used, else what is wrong --
// one that is too small, not 16-byte aligned, or an output that overlaps an
// input.  Addresses as integers (nothing is dereferenced); counts 0: none.
const char* svgf_check_arrays(const SvgfPlan& pl, bool sums_f32, uintptr_t sums, size_t sums_bytes, uintptr_t features,
                              size_t features_bytes, uintptr_t moments, size_t moments_bytes, uintptr_t counts,
                              size_t counts_bytes, uintptr_t out, size_t out_bytes);

}  // namespace rtw
