// wavefront_plan.hpp -- what rtw_render_wavefront runs: the samples of a batch,
// the paths and the bytes of every buffer of the driver's state, and the record
// sizes and the overlap rule rtw_path_advance checks its arrays by.  Host only,
// no HIP call, so that the CPU can check it (tests/native/wavefront_plan_check.cpp);
// capi_wavefront.cpp allocates and launches.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../../include/rtw.h"

namespace rtw {

// batch = 0: as many samples as keep a round at or below this many paths
constexpr uint64_t kWavefrontPaths = (uint64_t)1 << 22;
// a slot is a uint32: a batch's paths and a colour array's slots
constexpr uint64_t kWavefrontMaxSlots = (uint64_t)1 << 32;

// the records of a path state and of a round, in bytes, for values of `elem` bytes
struct PathRecords {
    size_t rays, rng, vec3, slot, event, hits, ids;
};
constexpr PathRecords path_records(size_t elem) {
    return PathRecords{6 * elem, 4 * sizeof(uint64_t), 3 * elem, sizeof(uint32_t), sizeof(int32_t), 9 * elem,
                       4 * sizeof(int32_t)};
}

struct WavefrontPlan {
    int err = RTW_OK;
    const char* err_text = "";
    uint64_t pixels = 0;              // W * H
    uint32_t batch = 0;               // B: the samples of a full batch (0: nothing to run)
    uint32_t batches = 0;             // ceil(n_samples / B)
    uint32_t last_batch = 0;          // the samples of the last one
    uint64_t paths = 0;               // B * W * H: the slots of the colour array
    // the driver's state: two path states (ping-pong), one round, the colours, the sums' staging
    size_t rays_bytes = 0, rng_bytes = 0, vec3_bytes = 0, slot_bytes = 0;   // of ONE state's arrays
    size_t state_bytes = 0;           // rays + rng + mult + res + slot of one state
    size_t hits_bytes = 0, ids_bytes = 0, event_bytes = 0;                  // the round's (next: rays_bytes,
    size_t round_bytes = 0;           // weight / emitted: vec3_bytes): hits + ids + next + weight + emitted + event
    size_t colour_bytes = 0;
    size_t sums_bytes = 0;            // W * H * 3 f64
    size_t total_bytes = 0;           // 2 states + round + colour (the sums are the caller's, or staged)
};

// batch 0: B = clamp(kWavefrontPaths / (W * H), 1, n_samples); else B = min(batch, n_samples).
// elem: 4 (RTW_F32) or 8.  Refused: an empty image, more than 2^32 paths in a batch.
WavefrontPlan plan_wavefront(uint32_t width, uint32_t height, uint32_t n_samples, uint32_t batch, size_t elem);

// [a, a + a_bytes) and [b, b + b_bytes) share a byte (an empty range shares none)
inline bool ranges_overlap(uintptr_t a, size_t a_bytes, uintptr_t b, size_t b_bytes) {
    return a_bytes && b_bytes && a < b + b_bytes && b < a + a_bytes;
}

// The arrays of one rtw_path_advance: "" when they can be used, else what is
// wrong.  Addresses as integers (nothing is dereferenced).  in[3]: mult, res,
// slot; round[5]: event, weight, emitted, next, rng; out[5]: rays, rng, mult,
// res, slot.  bytes: each array's size, or 0 for "as large as n records" (the
// host form).  align: check the device forms' record alignment.
struct PathArray {
    uintptr_t at;
    size_t bytes;
};
const char* advance_check_arrays(uint64_t n, size_t elem, const PathArray (&in)[3], const PathArray (&round)[5],
                                 const PathArray (&out)[5], PathArray colour, uint64_t colour_slots, bool device);

}  // namespace rtw
