// wavefront_plan.cpp -- see wavefront_plan.hpp.
#include "wavefront_plan.hpp"

#include <algorithm>

namespace rtw {

WavefrontPlan plan_wavefront(uint32_t width, uint32_t height, uint32_t n_samples, uint32_t batch, size_t elem) {
    WavefrontPlan pl;
    pl.pixels = (uint64_t)width * height;
    if (pl.pixels == 0) {
        pl.err = RTW_E_INVALID;
        pl.err_text = "the image has no pixels";
        return pl;
    }
    pl.sums_bytes = (size_t)pl.pixels * 3 * sizeof(double);
    if (n_samples == 0) return pl;   // nothing to run, nothing to allocate
    const uint64_t fit = std::max<uint64_t>(kWavefrontPaths / pl.pixels, 1);
    const uint64_t b = std::min<uint64_t>(batch ? batch : fit, n_samples);
    if (b * pl.pixels > kWavefrontMaxSlots) {
        pl.err = RTW_E_INVALID;
        pl.err_text = "a batch of more than 2^32 paths (batch x W x H): a slot is a uint32";
        return pl;
    }
    pl.batch = (uint32_t)b;
    pl.batches = (uint32_t)((n_samples + b - 1) / b);
    pl.last_batch = (uint32_t)(n_samples - (uint64_t)(pl.batches - 1) * b);
    pl.paths = b * pl.pixels;
    const PathRecords rec = path_records(elem);
    const size_t n = (size_t)pl.paths;
    pl.rays_bytes = n * rec.rays;
    pl.rng_bytes = n * rec.rng;
    pl.vec3_bytes = n * rec.vec3;
    pl.slot_bytes = n * rec.slot;
    pl.state_bytes = pl.rays_bytes + pl.rng_bytes + 2 * pl.vec3_bytes + pl.slot_bytes;
    pl.hits_bytes = n * rec.hits;
    pl.ids_bytes = n * rec.ids;
    pl.event_bytes = n * rec.event;
    pl.round_bytes = pl.hits_bytes + pl.ids_bytes + pl.rays_bytes + 2 * pl.vec3_bytes + pl.event_bytes;
    pl.colour_bytes = pl.vec3_bytes;
    pl.total_bytes = 2 * pl.state_bytes + pl.round_bytes + pl.colour_bytes;
    return pl;
}

namespace {

// the largest power of two dividing the record's size, 16 at the most (path_kernels.h record_align)
size_t record_alignment(size_t bytes) { return bytes % 16 == 0 ? 16 : bytes % 8 == 0 ? 8 : 4; }

}  // namespace

const char* advance_check_arrays(uint64_t n, size_t elem, const PathArray (&in)[3], const PathArray (&round)[5],
                                 const PathArray (&out)[5], PathArray colour, uint64_t colour_slots, bool device) {
    if (n > kWavefrontMaxSlots) return "more than 2^32 paths in one advance: a slot is a uint32";
    if (colour_slots > kWavefrontMaxSlots) return "more than 2^32 colour slots: a slot is a uint32";
    if (n == 0) return "";
    const PathRecords rec = path_records(elem);
    const size_t in_rec[3] = {rec.vec3, rec.vec3, rec.slot};
    const size_t round_rec[5] = {rec.event, rec.vec3, rec.vec3, rec.rays, rec.rng};
    const size_t out_rec[5] = {rec.rays, rec.rng, rec.vec3, rec.vec3, rec.slot};
    struct Span {
        uintptr_t at;
        size_t bytes;
    };
    Span reads[8], writes[5];
    auto one = [&](const PathArray& a, size_t record, Span& s) -> const char* {
        if (!a.at) return "an array is NULL";
        const size_t need = (size_t)n * record;
        if (device && a.bytes < need) return "a buffer is smaller than n records";
        if (device && a.at % record_alignment(record)) return "a device buffer is not aligned for its records (rtw.h)";
        s = Span{a.at, need};
        return nullptr;
    };
    for (int k = 0; k < 3; ++k)
        if (const char* e = one(in[k], in_rec[k], reads[k])) return e;
    for (int k = 0; k < 5; ++k)
        if (const char* e = one(round[k], round_rec[k], reads[3 + k])) return e;
    for (int k = 0; k < 5; ++k)
        if (const char* e = one(out[k], out_rec[k], writes[k])) return e;
    const size_t colour_need = (size_t)colour_slots * rec.vec3;
    if (colour_slots) {
        if (!colour.at) return "colour is NULL";
        if (device && colour.bytes < colour_need) return "colour is smaller than its slots";
        if (device && colour.at % record_alignment(rec.vec3)) return "a device buffer is not aligned for its records (rtw.h)";
    }
    // the step is out of place: what it writes shares no byte with what it reads, nor with itself
    for (int w = 0; w < 5; ++w) {
        for (int r = 0; r < 8; ++r)
            if (ranges_overlap(writes[w].at, writes[w].bytes, reads[r].at, reads[r].bytes))
                return "an out-state buffer overlaps an in-state or round buffer (the advance is out of place)";
        for (int v = 0; v < w; ++v)
            if (ranges_overlap(writes[w].at, writes[w].bytes, writes[v].at, writes[v].bytes))
                return "two out-state buffers overlap";
        if (colour_slots && ranges_overlap(writes[w].at, writes[w].bytes, colour.at, colour_need))
            return "an out-state buffer overlaps colour";
    }
    return "";
}

}  // namespace rtw
