// ambient_plan.hpp -- what rtw_ambient_occlusion checks and launches, without a
// HIP call: the sizes and alignments of its four arrays, the refusals of its
// arguments in their order, the limits, and the launch of ambient_kernel on a
// query plan (query_plan.hpp: the closest hit's LDS unchanged).
// tests/native/ambient_plan_check.cpp holds the tables.
#pragma once

#include "../ambient_kernels.h"
#include "query_plan.hpp"

namespace rtw {

// The limits of one call: points, (point, sample) pairs, and pairs when a record
// is asked for (a record row index is 32 bits' worth of rows).
constexpr uint64_t kAmbientMaxPoints = (uint64_t)1 << 40;
constexpr uint64_t kAmbientMaxPairs = (uint64_t)1 << 62;
constexpr uint64_t kAmbientMaxRecordPairs = (uint64_t)1 << 32;

// One array of the query: bytes for n points and S samples, and the alignment a
// device buffer must start on (the kernel's widest access to a row).
struct AmbientArray {
    size_t bytes = 0;
    uint32_t align = 1;
};
struct AmbientSizes {
    AmbientArray points;       // n x 6 of the context's precision
    AmbientArray open;         // n uint32
    AmbientArray directions;   // n * S x 3 of the context's precision
    AmbientArray occluded;     // n * S bytes
};
AmbientSizes ambient_sizes(bool f64, uint64_t n, uint32_t n_samples);

// The caller's arguments, as both entries see them; the *_bytes are the device
// form's (the host form passes none: `device` false).
struct AmbientArgs {
    const void* points = nullptr;
    uint64_t n = 0;
    uint32_t n_samples = 0;
    double t_min = 0.0;
    const void* open = nullptr;
    const void* directions = nullptr;
    const void* occluded = nullptr;
    bool device = false;
    size_t points_bytes = 0, open_bytes = 0, directions_bytes = 0, occluded_bytes = 0;
};
// RTW_OK, or RTW_E_INVALID with *text set.  Checked in this order: points NULL
// with n > 0, open NULL with n > 0, a t_min that is not finite and >= 0,
// n_samples == 0, more than 2^40 points, more than 2^62 pairs, more than 2^32
// pairs when a record is asked for; then, in the device form, a short buffer
// (points, open, directions, occluded) and a misaligned one.  t_max is not
// checked: NaN or below t_min is an empty range, and every pair is open.  An
// empty light list is fine; n == 0 passes once the scalar arguments do.
int ambient_check(const AmbientArgs& a, bool f64, const char** text);

// The launch of ambient_kernel on the queries' plan.
struct AmbientPlan {
    size_t lds = kQueryLdsMin;      // dynamic LDS: QueryPlan::hit_lds, unchanged
    int err = RTW_OK;
    const char* err_text = "";
};
AmbientPlan plan_ambient(const QueryPlan& q, bool f64);

}  // namespace rtw
