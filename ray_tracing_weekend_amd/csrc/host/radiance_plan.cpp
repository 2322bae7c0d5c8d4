// radiance_plan.cpp -- see radiance_plan.hpp
#include "radiance_plan.hpp"

#include "../path_kernels.h"   // record_align

namespace rtw {

RadianceSizes radiance_sizes(bool f64, uint64_t n, uint32_t n_samples) {
    const size_t esz = f64 ? sizeof(double) : sizeof(float);
    const uint64_t rows = n * (uint64_t)n_samples;
    RadianceSizes s;
    s.rays = {(size_t)(n * 6 * esz), record_align(6 * esz)};
    s.radiance = {(size_t)(n * 3 * sizeof(double)), record_align(3 * sizeof(double))};
    s.rng = {(size_t)(n * 4 * sizeof(uint64_t)), 16u};
    s.colours = {(size_t)(rows * 3 * esz), record_align(3 * esz)};
    s.segments = {(size_t)(rows * sizeof(uint32_t)), (uint32_t)sizeof(uint32_t)};
    return s;
}

namespace {

bool misaligned(const void* p, uint32_t align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }

}  // namespace

int radiance_check(const RadianceArgs& a, bool f64, const char** text) {
    const char* why = nullptr;
    if (a.n && !a.rays) why = "rays is NULL";
    else if (a.n && !a.radiance) why = "radiance is NULL";
    else if (a.n && !a.background) why = "background is NULL";
    else if (a.n_samples == 0) why = "n_samples is 0";
    else if (a.rng && a.n_samples != 1) why = "rng holds one start state per ray: n_samples must be 1";
    else if ((uint64_t)a.first_sample + a.n_samples > kRadianceMaxSampleEnd)
        why = "first_sample + n_samples is over 2^32";
    else if (a.n > kRadianceMaxRays) why = "more than 2^40 rays in one query";
    else if (a.n > kRadianceMaxPairs / a.n_samples) why = "more than 2^62 (ray, sample) pairs in one query";
    else if ((a.colours || a.segments) && a.n * (uint64_t)a.n_samples > kRadianceMaxRecordPairs)
        why = "more than 2^32 sample records in one query";
    if (!why && a.device && a.n) {
        const RadianceSizes s = radiance_sizes(f64, a.n, a.n_samples);
        if (a.rays_bytes < s.rays.bytes) why = "d_rays is smaller than n x 6 values";
        else if (a.radiance_bytes < s.radiance.bytes) why = "d_radiance is smaller than n x 3 doubles";
        else if (a.rng && a.rng_bytes < s.rng.bytes) why = "d_rng is smaller than n x 4 uint64";
        else if (a.colours && a.colours_bytes < s.colours.bytes)
            why = "d_colours is smaller than n x n_samples x 3 values";
        else if (a.segments && a.segments_bytes < s.segments.bytes)
            why = "d_segments is smaller than n x n_samples uint32";
        else if (misaligned(a.rays, s.rays.align) || misaligned(a.radiance, s.radiance.align) ||
                 misaligned(a.rng, s.rng.align) || misaligned(a.colours, s.colours.align) ||
                 misaligned(a.segments, s.segments.align))
            why = "a device buffer is not aligned for its rows (rays: 16 B in f64, 8 B in f32; radiance: 8 B; "
                  "rng: 16 B; colours: 8 B in f64, 4 B in f32; segments: 4 B)";
    }
    if (text) *text = why ? why : "";
    return why ? RTW_E_INVALID : RTW_OK;
}

RadiancePlan plan_radiance(const QueryPlan& q, bool f64) {
    RadiancePlan r;
    r.lds = radiance_lds(q.hit_lds, q.light_path, q.light_stack);
    r.light_off = q.light_path == kLightBvh ? (uint32_t)direct_light_off(q.hit_lds) : 0u;
    if (r.lds > kLdsLimit) {
        r.err = RTW_E_UNSUPPORTED;
        r.err_text = "the radiance kernel's LDS (the closest hit's and the light BVH's stacks) exceeds the device's";
    } else if (!radiance_kernel_exists(f64, q.world, q.robust != 0)) {
        r.err = RTW_E_UNSUPPORTED;
        r.err_text = "no radiance kernel for this scene and tuning";
    }
    return r;
}

}  // namespace rtw
