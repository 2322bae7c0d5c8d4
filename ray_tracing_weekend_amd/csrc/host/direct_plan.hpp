// direct_plan.hpp -- what rtw_direct_light checks and launches, without a HIP
// call: the sizes and alignments of its four arrays, the refusals of its
// arguments, and the dynamic LDS of direct_light_kernel on a query plan
// (query_plan.hpp: the closest hit's bytes, then the light BVH's stacks).
// tests/native/direct_plan_check.cpp holds the tables.
#pragma once

#include "../direct_kernels.h"
#include "query_plan.hpp"

namespace rtw {

// One array of the query: bytes for n points and S samples, and the alignment a
// device buffer must start on (the kernel's widest access to a row).
struct DirectArray {
    size_t bytes = 0;
    uint32_t align = 1;
};
struct DirectSizes {
    DirectArray points;       // n x 6 of the context's precision
    DirectArray direct;       // n x 3 f64 in both precisions
    DirectArray samples;      // n * S x 12 of the context's precision
    DirectArray sample_ids;   // n * S x 4 int32
};
DirectSizes direct_sizes(bool f64, uint64_t n, uint32_t n_samples);

// The caller's arguments, as both entries see them; the *_bytes are the device
// form's (the host form passes none: `device` false).
struct DirectArgs {
    const void* points = nullptr;
    uint64_t n = 0;
    uint32_t n_samples = 0;
    double t_min = 0.0;
    const void* direct = nullptr;
    const void* samples = nullptr;
    const void* sample_ids = nullptr;
    bool device = false;
    size_t points_bytes = 0, direct_bytes = 0, samples_bytes = 0, sample_ids_bytes = 0;
};
// RTW_OK, or RTW_E_INVALID with *text set: a NULL array with n > 0 (the two
// optional ones excepted), a bad t_min, n_samples == 0, an empty light list, more
// than 2^40 points, n * S over 2^32 when records are asked for, a short or
// misaligned device buffer.  Checked in that order; n == 0 passes once the
// scalar arguments do.
int direct_check(const DirectArgs& a, bool f64, uint32_t n_list, const char** text);

// The launch of direct_light_kernel on the queries' plan.
struct DirectPlan {
    size_t lds = kQueryLdsMin;      // dynamic LDS (direct_kernels.h direct_lds)
    uint32_t light_off = 0;         // DParams::light_off
    int err = RTW_OK;
    const char* err_text = "";
};
DirectPlan plan_direct(const QueryPlan& q, bool f64);

}  // namespace rtw
