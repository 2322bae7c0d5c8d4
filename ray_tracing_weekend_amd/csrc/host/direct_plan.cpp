// direct_plan.cpp -- see direct_plan.hpp
#include "direct_plan.hpp"

#include <cmath>

#include "../path_kernels.h"   // record_align

namespace rtw {

DirectSizes direct_sizes(bool f64, uint64_t n, uint32_t n_samples) {
    const size_t esz = f64 ? sizeof(double) : sizeof(float);
    const uint64_t rows = n * (uint64_t)n_samples;
    DirectSizes s;
    s.points = {(size_t)(n * 6 * esz), record_align(6 * esz)};
    s.direct = {(size_t)(n * 3 * sizeof(double)), record_align(3 * sizeof(double))};
    s.samples = {(size_t)(rows * kDirectSampleValues * esz), 16u};
    s.sample_ids = {(size_t)(rows * kDirectIdValues * sizeof(int32_t)), 16u};
    return s;
}

namespace {

bool misaligned(const void* p, uint32_t align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }

}  // namespace

int direct_check(const DirectArgs& a, bool f64, uint32_t n_list, const char** text) {
    const char* why = nullptr;
    if (a.n && !a.points) why = "points is NULL";
    else if (a.n && !a.direct) why = "direct is NULL";
    else if (!(a.t_min >= 0.0) || !std::isfinite(a.t_min)) why = "t_min must be finite and >= 0";
    else if (a.n_samples == 0) why = "n_samples is 0";
    else if (n_list == 0)
        why = "rtw_direct_light: the light list is empty (the reference panics, hittable_list.rs:417)";
    else if (a.n > (uint64_t)1 << 40) why = "more than 2^40 points in one query";
    else if ((a.samples || a.sample_ids) && a.n * (uint64_t)a.n_samples > (uint64_t)1 << 32)
        why = "more than 2^32 sample records in one query";
    if (!why && a.device && a.n) {
        const DirectSizes s = direct_sizes(f64, a.n, a.n_samples);
        if (a.points_bytes < s.points.bytes) why = "d_points is smaller than n x 6 values";
        else if (a.direct_bytes < s.direct.bytes) why = "d_direct is smaller than n x 3 doubles";
        else if (a.samples && a.samples_bytes < s.samples.bytes) why = "d_samples is smaller than n x n_samples x 12 values";
        else if (a.sample_ids && a.sample_ids_bytes < s.sample_ids.bytes)
            why = "d_sample_ids is smaller than n x n_samples x 4 int32";
        else if (misaligned(a.points, s.points.align) || misaligned(a.direct, s.direct.align) ||
                 misaligned(a.samples, s.samples.align) || misaligned(a.sample_ids, s.sample_ids.align))
            why = "a device buffer is not aligned for its rows (points: 16 B in f64, 8 B in f32; direct: 8 B; "
                  "samples, sample_ids: 16 B)";
    }
    if (text) *text = why ? why : "";
    return why ? RTW_E_INVALID : RTW_OK;
}

DirectPlan plan_direct(const QueryPlan& q, bool f64) {
    DirectPlan d;
    d.lds = direct_lds(q.hit_lds, q.light_path, q.light_stack);
    d.light_off = q.light_path == kLightBvh ? (uint32_t)direct_light_off(q.hit_lds) : 0u;
    if (d.lds > kLdsLimit) {
        d.err = RTW_E_UNSUPPORTED;
        d.err_text = "the direct-light kernel's LDS (the closest hit's and the light BVH's stacks) exceeds the device's";
    } else if (!direct_kernel_exists(f64, q.world, q.robust != 0)) {
        d.err = RTW_E_UNSUPPORTED;
        d.err_text = "no direct-light kernel for this scene and tuning";
    }
    return d;
}

}  // namespace rtw
