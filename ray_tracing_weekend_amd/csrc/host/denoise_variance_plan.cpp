// denoise_variance_plan.cpp -- see denoise_variance_plan.hpp.
#include "denoise_variance_plan.hpp"

#include <math.h>

namespace rtw {

void denoise_variance_params_default(rtw_denoise_variance_params* out) {
    if (!out) return;
    *out = rtw_denoise_variance_params{};
    out->iterations = 5;
    out->normal_power_log2 = 5;
    out->sigma_var = 2.0;
    out->sigma_depth = 0.125;
    out->demodulate = 1;
    out->fill_nonfinite = 1;
}

size_t svgf_lds_bytes(uint32_t step) {
    const uint64_t halo = 2ull * step;
    return (size_t)((kDenoiseTileW + 2 * halo) * (kDenoiseTileH + 2 * halo) * kSvgfLdsPerPixel);
}

static SvgfPlan refuse(SvgfPlan pl, const char* text) {
    pl.err = RTW_E_INVALID;
    pl.err_text = text;
    return pl;
}

SvgfPlan plan_denoise_variance(const rtw_denoise_variance_params* params, uint32_t width, uint32_t height,
                               bool has_counts, uint32_t spp, uint32_t denoise_lds) {
    SvgfPlan pl;
    if (params) pl.params = *params;
    else denoise_variance_params_default(&pl.params);
    const rtw_denoise_variance_params& p = pl.params;
    if (p.iterations < 1 || p.iterations > kDenoiseMaxIterations) return refuse(pl, "iterations must be 1..16");
    if (p.normal_power_log2 > kDenoiseMaxNormalPower) return refuse(pl, "normal_power_log2 must be 0..10");
    if (!(p.sigma_var >= 0.0) || !isfinite(p.sigma_var)) return refuse(pl, "sigma_var must be finite and >= 0");
    if (!(p.sigma_depth > 0.0) || !isfinite(p.sigma_depth)) return refuse(pl, "sigma_depth must be finite and > 0");
    if (p.demodulate > 1 || p.fill_nonfinite > 1) return refuse(pl, "demodulate and fill_nonfinite are 0 or 1");
    if (!has_counts && spp == 0) return refuse(pl, "spp is 0 and there are no counts");
    if (width > 65535 || height > 65535) return refuse(pl, "image width or height beyond 65535");

    pl.sv2 = p.sigma_var * p.sigma_var;
    pl.pixels = (uint64_t)width * height;
    pl.blocks = (uint32_t)((pl.pixels + kDenoiseBlock - 1) / kDenoiseBlock);
    pl.iterations = p.iterations;
    pl.record_bytes = (size_t)pl.pixels * kDenoiseRecord;
    pl.var_bytes = (size_t)pl.pixels * kSvgfVarRecord;
    pl.state_bytes = 4 * pl.record_bytes + 2 * pl.var_bytes;
    pl.sums_bytes_f32 = (size_t)pl.pixels * 3 * sizeof(float);
    pl.sums_bytes_f64 = (size_t)pl.pixels * 3 * sizeof(double);
    pl.features_bytes = (size_t)pl.pixels * 8 * sizeof(double);
    pl.moments_bytes = (size_t)pl.pixels * 2 * sizeof(double);
    pl.counts_bytes = (size_t)pl.pixels * sizeof(uint32_t);
    pl.out_bytes = (size_t)pl.pixels * 3 * sizeof(double);
    for (uint32_t k = 0; k < pl.iterations; ++k) {
        SvgfStep& s = pl.steps[k];
        s.step = 1u << k;
        const size_t bytes = svgf_lds_bytes(s.step);
        const bool fits = bytes <= kLdsLimit;
        const bool want = denoise_lds >= 2 || (denoise_lds == 1 && s.step <= kSvgfLdsDefaultMaxStep);
        s.lds = want && fits ? 1u : 0u;
        s.lds_bytes = s.lds ? bytes : 0;
        s.grid_x = (width + kDenoiseTileW - 1) / kDenoiseTileW;
        s.grid_y = (height + kDenoiseTileH - 1) / kDenoiseTileH;
        pl.lds_iterations += s.lds;
    }
    return pl;
}

const char* svgf_check_arrays(const SvgfPlan& pl, bool sums_f32, uintptr_t sums, size_t sums_bytes, uintptr_t features,
                              size_t features_bytes, uintptr_t moments, size_t moments_bytes, uintptr_t counts,
                              size_t counts_bytes, uintptr_t out, size_t out_bytes) {
    const size_t need_sums = sums_f32 ? pl.sums_bytes_f32 : pl.sums_bytes_f64;
    if (sums_bytes < need_sums) return "d_sums is smaller than H x W x 3 values";
    if (features_bytes < pl.features_bytes) return "d_features is smaller than H x W x 8 doubles";
    if (moments_bytes < pl.moments_bytes) return "d_moments is smaller than H x W x 2 doubles";
    if (counts && counts_bytes < pl.counts_bytes) return "d_counts is smaller than H x W uint32";
    if (out_bytes < pl.out_bytes) return "d_out is smaller than H x W x 3 doubles";
    if (sums % 16 || features % 16 || moments % 16 || counts % 16 || out % 16)
        return "a device pointer is not 16-byte aligned";
    auto overlaps = [&](uintptr_t a, size_t n) { return n && pl.out_bytes && a < out + pl.out_bytes && out < a + n; };
    if (overlaps(sums, need_sums) || overlaps(features, pl.features_bytes) || overlaps(moments, pl.moments_bytes) ||
        (counts && overlaps(counts, pl.counts_bytes)))
        return "d_out overlaps an input";
    return "";
}

}  // namespace rtw
