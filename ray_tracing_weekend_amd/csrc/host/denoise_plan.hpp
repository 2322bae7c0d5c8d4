// denoise_plan.hpp -- what a denoise launches (rtw_denoise; the filter is
// include/rtw.h's contract): the checked parameters, the per-iteration schedule
// of denoise_atrous_kernel (step, colour variance, the staged or the direct form
// with its dynamic LDS, the grid) and the sizes of the denoise state's buffers.
// Host only, no HIP call: capi_denoise.cpp allocates and launches.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../../include/rtw.h"
#include "render_plan.hpp"

namespace rtw {

constexpr uint32_t kDenoiseMaxIterations = 16;
constexpr uint32_t kDenoiseMaxNormalPower = 10;
// the workgroup of denoise_atrous_kernel: a tile of 32 x 8 pixels, one per lane
constexpr uint32_t kDenoiseTileW = 32, kDenoiseTileH = 8;
// prepare / finish: one pixel per lane of a 256-lane workgroup
constexpr uint32_t kDenoiseBlock = 256;
// a record: 4 doubles, read and written as two 16-byte halves
constexpr size_t kDenoiseRecord = 32;
// what the staged form keeps per pixel of the tile and its halo: guide + colour
constexpr size_t kDenoiseLdsPerPixel = 2 * kDenoiseRecord;
// tuning denoise_lds = 1: the steps up to this one are staged (0: none).
// Measured on the MI355X (tools/denoise_bench.py ab, profiles/denoise_bench.jsonl):
// at 1200 x 800 the staged form takes 0.045 ms less than the direct one at step 1
// and 0.078 against 0.116 ms at step 2, ties at step 4 and takes twice as long at
// step 8 (one 160 KiB workgroup per CU); at 600 x 600 steps 1 and 2 tie.
constexpr uint32_t kDenoiseLdsDefaultMaxStep = 2;

struct DenoiseStep {
    uint32_t step = 1;        // 2^k
    double sc2 = 0.0;         // (sigma_colour * 2^-k)^2
    uint32_t lds = 0;         // 1: the staged form
    size_t lds_bytes = 0;     // its dynamic LDS (0: direct)
    uint32_t grid_x = 0, grid_y = 0;
};

struct DenoisePlan {
    int err = RTW_OK;
    const char* err_text = "";
    rtw_denoise_params params{};          // the checked parameters (the defaults for NULL)
    uint64_t pixels = 0;
    uint32_t blocks = 0;                  // prepare / finish grid
    uint32_t iterations = 0;
    uint32_t lds_iterations = 0;          // ... of which staged
    DenoiseStep steps[kDenoiseMaxIterations];
    // the denoise state's buffers: guide, albedo and two colour record arrays
    size_t record_bytes = 0;              // of one array
    size_t state_bytes = 0;               // of the four
    // the arrays of a call
    size_t sums_bytes_f32 = 0, sums_bytes_f64 = 0, features_bytes = 0, counts_bytes = 0, out_bytes = 0;
};

void denoise_params_default(rtw_denoise_params* out);

// dynamic LDS of the staged form at `step`: the tile and its 2 * step halo
size_t denoise_lds_bytes(uint32_t step);

// params NULL: the defaults.  has_counts false: spp is every pixel's count.
// denoise_lds: the tuning key (0 direct, 1 the default plan, 2 staged wherever it fits).
DenoisePlan plan_denoise(const rtw_denoise_params* params, uint32_t width, uint32_t height, bool has_counts,
                         uint32_t spp, uint32_t denoise_lds);

// The device form's arrays: "" when they can be used, else what is wrong --
// one that is too small, not 16-byte aligned, or an output that overlaps an
// input.  Addresses as integers (nothing is dereferenced); counts 0: none.
const char* denoise_check_arrays(const DenoisePlan& pl, bool sums_f32, uintptr_t sums, size_t sums_bytes,
                                 uintptr_t features, size_t features_bytes, uintptr_t counts, size_t counts_bytes,
                                 uintptr_t out, size_t out_bytes);

}  // namespace rtw
