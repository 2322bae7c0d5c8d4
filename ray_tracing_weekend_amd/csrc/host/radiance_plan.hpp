// radiance_plan.hpp -- what rtw_radiance_rays checks and launches, without a HIP
// call: the sizes and alignments of its five arrays, the refusals of its
// arguments in their order, the limits, the loop bound of a lane, and the launch
// of radiance_kernel on a query plan (query_plan.hpp: the closest hit's bytes,
// then the light BVH's stacks).  tests/native/radiance_plan_check.cpp holds the
// tables.
#pragma once

#include "../radiance_kernels.h"
#include "query_plan.hpp"

namespace rtw {

// The limits of one call: rays, (ray, sample) pairs, pairs when a record is asked
// for (a record row index is 32 bits' worth of rows), and the sample indices
// (first_sample + n_samples may reach 2^32, not pass it).
constexpr uint64_t kRadianceMaxRays = (uint64_t)1 << 40;
constexpr uint64_t kRadianceMaxPairs = (uint64_t)1 << 62;
constexpr uint64_t kRadianceMaxRecordPairs = (uint64_t)1 << 32;
constexpr uint64_t kRadianceMaxSampleEnd = (uint64_t)1 << 32;

// One array of the query: bytes for n rays and S samples, and the alignment a
// device buffer must start on (the kernel's widest access to a row).
struct RadianceArray {
    size_t bytes = 0;
    uint32_t align = 1;
};
struct RadianceSizes {
    RadianceArray rays;       // n x 6 of the context's precision
    RadianceArray radiance;   // n x 3 f64 in both precisions
    RadianceArray rng;        // n x 4 uint64
    RadianceArray colours;    // n * S x 3 of the context's precision
    RadianceArray segments;   // n * S uint32
};
RadianceSizes radiance_sizes(bool f64, uint64_t n, uint32_t n_samples);

// The caller's arguments, as both entries see them; the *_bytes are the device
// form's (the host form passes none: `device` false).
struct RadianceArgs {
    const void* rays = nullptr;
    uint64_t n = 0;
    uint32_t first_sample = 0, n_samples = 0;
    const void* background = nullptr;
    const void* rng = nullptr;
    const void* radiance = nullptr;
    const void* colours = nullptr;
    const void* segments = nullptr;
    bool device = false;
    size_t rays_bytes = 0, rng_bytes = 0, radiance_bytes = 0, colours_bytes = 0, segments_bytes = 0;
};
// RTW_OK, or RTW_E_INVALID with *text set.  Checked in this order: rays, radiance
// or background NULL with n > 0, n_samples == 0, rng with n_samples != 1,
// first_sample + n_samples over 2^32, more than 2^40 rays, more than 2^62 (ray,
// sample) pairs, more than 2^32 pairs when a record is asked for; then, in the
// device form, a short buffer (rays, radiance, rng, colours, segments) and a
// misaligned one.  max_depth is free (0: every colour is 0 + 0).  n == 0 passes
// once the scalar arguments do.
int radiance_check(const RadianceArgs& a, bool f64, const char** text);

// The launch of radiance_kernel on the queries' plan.
struct RadiancePlan {
    size_t lds = kQueryLdsMin;      // dynamic LDS (radiance_kernels.h radiance_lds)
    uint32_t light_off = 0;         // RParams::light_off
    int err = RTW_OK;
    const char* err_text = "";
};
RadiancePlan plan_radiance(const QueryPlan& q, bool f64);

}  // namespace rtw
