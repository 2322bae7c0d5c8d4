// ambient_plan.cpp -- see ambient_plan.hpp
#include "ambient_plan.hpp"

#include <cmath>

#include "../path_kernels.h"   // record_align

namespace rtw {

AmbientSizes ambient_sizes(bool f64, uint64_t n, uint32_t n_samples) {
    const size_t esz = f64 ? sizeof(double) : sizeof(float);
    const uint64_t rows = n * (uint64_t)n_samples;
    AmbientSizes s;
    s.points = {(size_t)(n * 6 * esz), record_align(6 * esz)};
    s.open = {(size_t)(n * sizeof(uint32_t)), (uint32_t)sizeof(uint32_t)};
    s.directions = {(size_t)(rows * 3 * esz), record_align(3 * esz)};
    s.occluded = {(size_t)rows, 1u};
    return s;
}

namespace {

bool misaligned(const void* p, uint32_t align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }

}  // namespace

int ambient_check(const AmbientArgs& a, bool f64, const char** text) {
    const char* why = nullptr;
    if (a.n && !a.points) why = "points is NULL";
    else if (a.n && !a.open) why = "open is NULL";
    else if (!(a.t_min >= 0.0) || !std::isfinite(a.t_min)) why = "t_min must be finite and >= 0";
    else if (a.n_samples == 0) why = "n_samples is 0";
    else if (a.n > kAmbientMaxPoints) why = "more than 2^40 points in one query";
    else if (a.n > kAmbientMaxPairs / a.n_samples) why = "more than 2^62 (point, sample) pairs in one query";
    else if ((a.directions || a.occluded) && a.n * (uint64_t)a.n_samples > kAmbientMaxRecordPairs)
        why = "more than 2^32 sample records in one query";
    if (!why && a.device && a.n) {
        const AmbientSizes s = ambient_sizes(f64, a.n, a.n_samples);
        if (a.points_bytes < s.points.bytes) why = "d_points is smaller than n x 6 values";
        else if (a.open_bytes < s.open.bytes) why = "d_open is smaller than n uint32";
        else if (a.directions && a.directions_bytes < s.directions.bytes)
            why = "d_directions is smaller than n x n_samples x 3 values";
        else if (a.occluded && a.occluded_bytes < s.occluded.bytes)
            why = "d_occluded is smaller than n x n_samples bytes";
        else if (misaligned(a.points, s.points.align) || misaligned(a.open, s.open.align) ||
                 misaligned(a.directions, s.directions.align))
            why = "a device buffer is not aligned for its rows (points: 16 B in f64, 8 B in f32; open: 4 B; "
                  "directions: 8 B in f64, 4 B in f32)";
    }
    if (text) *text = why ? why : "";
    return why ? RTW_E_INVALID : RTW_OK;
}

AmbientPlan plan_ambient(const QueryPlan& q, bool f64) {
    AmbientPlan a;
    a.lds = q.hit_lds;
    if (!ambient_kernel_exists(f64, q.world, q.robust != 0)) {
        a.err = RTW_E_UNSUPPORTED;
        a.err_text = "no ambient-occlusion kernel for this scene and tuning";
    }
    return a;
}

}  // namespace rtw
