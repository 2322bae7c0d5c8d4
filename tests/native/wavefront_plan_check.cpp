// wavefront_plan_check.cpp -- CPU check of what rtw_render_wavefront plans
// (host/wavefront_plan.hpp): the samples of a batch, the bytes of every buffer,
// and the array rules of rtw_path_advance.  Built and run by
// tests/test_wavefront_host.py:
//   c++ -O2 -std=c++17 -I<csrc> -I<include> wavefront_plan_check.cpp <csrc>/host/wavefront_plan.cpp
// (the test also builds it with -fsanitize=address,undefined: a host program, run alone)
#include <stdio.h>
#include <string.h>

#include "host/wavefront_plan.hpp"

static int g_wrong = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            ++g_wrong;                     \
            printf("WRONG: " __VA_ARGS__); \
            printf("\n");                  \
        }                                  \
    } while (0)

using rtw::PathArray;
using rtw::WavefrontPlan;

// the bytes of a plan, restated: per path 6 + 3 + 3 values, 4 rng words and a slot in a
// state; 9 + 6 + 3 + 3 values, 4 ids and an event in a round; 3 values of colour
static void check_bytes(const WavefrontPlan& pl, size_t elem, const char* what) {
    const size_t n = (size_t)pl.paths;
    CHECK(pl.rays_bytes == n * 6 * elem && pl.rng_bytes == n * 32 && pl.vec3_bytes == n * 3 * elem &&
              pl.slot_bytes == n * 4,
          "%s: a state's arrays", what);
    CHECK(pl.state_bytes == n * (12 * elem + 36), "%s: state_bytes %zu", what, pl.state_bytes);
    CHECK(pl.hits_bytes == n * 9 * elem && pl.ids_bytes == n * 16 && pl.event_bytes == n * 4, "%s: a round's arrays", what);
    CHECK(pl.round_bytes == n * (21 * elem + 20), "%s: round_bytes %zu", what, pl.round_bytes);
    CHECK(pl.colour_bytes == n * 3 * elem, "%s: colour_bytes", what);
    CHECK(pl.total_bytes == n * (48 * elem + 92), "%s: total_bytes %zu", what, pl.total_bytes);
    CHECK(pl.sums_bytes == (size_t)pl.pixels * 24, "%s: sums_bytes", what);
    if (pl.batch) {
        CHECK((uint64_t)(pl.batches - 1) * pl.batch + pl.last_batch > 0 && pl.last_batch >= 1 && pl.last_batch <= pl.batch,
              "%s: the batches", what);
    }
}

static void plans() {
    for (size_t elem : {(size_t)4, (size_t)8}) {
        // one pixel: 2^22 samples would fit a round, the window has 5
        WavefrontPlan a = rtw::plan_wavefront(1, 1, 5, 0, elem);
        CHECK(!a.err && a.pixels == 1 && a.batch == 5 && a.batches == 1 && a.last_batch == 5 && a.paths == 5, "1 x 1");
        check_bytes(a, elem, "1 x 1");
        WavefrontPlan a2 = rtw::plan_wavefront(1, 1, 0xFFFFFFFFu, 0, elem);
        CHECK(!a2.err && a2.batch == (1u << 22) && a2.batches == 1024 && a2.last_batch == (1u << 22) - 1, "1 x 1, 2^32 - 1 samples");
        // 40 x 24, 4 samples, 3 a batch: 3 + 1
        WavefrontPlan b = rtw::plan_wavefront(40, 24, 4, 3, elem);
        CHECK(!b.err && b.batch == 3 && b.batches == 2 && b.last_batch == 1 && b.paths == 3 * 960, "40 x 24 batch 3");
        check_bytes(b, elem, "40 x 24 batch 3");
        CHECK(b.total_bytes == (elem == 8 ? 476u : 284u) * 2880u, "the header's bytes a path");
        // ... and the planner's own choice: all 4 fit
        WavefrontPlan b0 = rtw::plan_wavefront(40, 24, 4, 0, elem);
        CHECK(!b0.err && b0.batch == 4 && b0.batches == 1 && b0.last_batch == 4 && b0.paths == 3840, "40 x 24 batch 0");
        // a batch beyond the window is the window
        WavefrontPlan c = rtw::plan_wavefront(40, 24, 4, 9, elem);
        CHECK(!c.err && c.batch == 4 && c.batches == 1 && c.last_batch == 4 && c.paths == 3840, "batch > n_samples");
        check_bytes(c, elem, "batch > n_samples");
        // more pixels than 2^22: one sample at a time
        WavefrontPlan d = rtw::plan_wavefront(4096, 1025, 4, 0, elem);
        CHECK(!d.err && d.batch == 1 && d.batches == 4 && d.last_batch == 1 && d.paths == 4096ull * 1025, "W x H > 2^22");
        check_bytes(d, elem, "W x H > 2^22");
        // exactly 2^22 / 3 pixels and a remainder: floor
        WavefrontPlan d2 = rtw::plan_wavefront(1200, 800, 64, 0, elem);
        CHECK(!d2.err && d2.batch == 4 && d2.batches == 16 && d2.last_batch == 4, "1200 x 800");
        WavefrontPlan d3 = rtw::plan_wavefront(256, 160, 4, 0, elem);
        CHECK(!d3.err && d3.batch == 4 && d3.batches == 1, "256 x 160 x 4");
        // no samples: nothing to run, nothing to allocate, the sums still have their size
        WavefrontPlan e = rtw::plan_wavefront(40, 24, 0, 3, elem);
        CHECK(!e.err && e.batch == 0 && e.batches == 0 && e.last_batch == 0 && e.paths == 0 && e.total_bytes == 0 &&
                  e.sums_bytes == 960 * 24,
              "n_samples 0");
        // refused: no pixels; a batch of more than 2^32 paths
        CHECK(rtw::plan_wavefront(0, 24, 4, 0, elem).err == RTW_E_INVALID, "W = 0");
        CHECK(rtw::plan_wavefront(40, 0, 4, 0, elem).err == RTW_E_INVALID, "H = 0");
        CHECK(rtw::plan_wavefront(65535, 65535, 4, 2, elem).err == RTW_E_INVALID, "2 x 65535^2 paths");
        CHECK(rtw::plan_wavefront(65535, 65535, 4, 1, elem).err == RTW_OK, "65535^2 paths");
        CHECK(rtw::plan_wavefront(65535, 65535, 4, 0, elem).batch == 1, "65535^2 paths, batch 0");
    }
}

// the arrays of an advance as addresses in one imaginary buffer, `gap` bytes apart
struct Arrays {
    PathArray in[3], round[5], out[5], colour;
};
static Arrays laid_out(uint64_t n, size_t elem, uint64_t colour_slots) {
    const rtw::PathRecords r = rtw::path_records(elem);
    const size_t recs[14] = {r.vec3, r.vec3, r.slot, r.event, r.vec3, r.vec3, r.rays, r.rng, r.rays, r.rng, r.vec3, r.vec3, r.slot,
                             0};
    Arrays a;
    uintptr_t at = 0x10000;
    PathArray* all[14] = {&a.in[0], &a.in[1], &a.in[2], &a.round[0], &a.round[1], &a.round[2], &a.round[3], &a.round[4],
                          &a.out[0], &a.out[1], &a.out[2], &a.out[3], &a.out[4], &a.colour};
    for (int k = 0; k < 14; ++k) {
        const size_t bytes = k == 13 ? (size_t)colour_slots * r.vec3 : (size_t)n * recs[k];
        *all[k] = PathArray{at, bytes};
        at += (bytes + 15) / 16 * 16;
    }
    return a;
}
static const char* check(const Arrays& a, uint64_t n, size_t elem, uint64_t slots, bool device) {
    return rtw::advance_check_arrays(n, elem, a.in, a.round, a.out, a.colour, slots, device);
}

static void arrays() {
    for (size_t elem : {(size_t)4, (size_t)8}) {
        const uint64_t n = 1000, slots = 1200;
        const Arrays ok = laid_out(n, elem, slots);
        for (bool device : {false, true}) CHECK(!*check(ok, n, elem, slots, device), "a good set of arrays: %s", check(ok, n, elem, slots, device));
        CHECK(!*check(ok, 0, elem, slots, true), "n = 0");
        // every out-state array against every in-state and round array, against colour and the other out arrays
        for (int w = 0; w < 5; ++w) {
            for (int r = 0; r < 8; ++r) {
                Arrays bad = ok;
                const PathArray& victim = r < 3 ? ok.in[r] : ok.round[r - 3];
                bad.out[w].at = victim.at + (victim.bytes / 32) * 16;   // (16-aligned, inside the victim)
                CHECK(strstr(check(bad, n, elem, slots, true), "overlaps"), "out %d inside read %d", w, r);
                CHECK(strstr(check(bad, n, elem, slots, false), "overlaps"), "out %d inside read %d (host)", w, r);
            }
            Arrays bad = ok;
            bad.out[w].at = ok.colour.at;
            CHECK(strstr(check(bad, n, elem, slots, true), "overlaps colour"), "out %d on colour", w);
            bad = ok;
            bad.out[w].at = ok.out[(w + 1) % 5].at;
            CHECK(strstr(check(bad, n, elem, slots, true), "overlap"), "out %d on out %d", w, (w + 1) % 5);
        }
        // touching is not overlapping (the good set's arrays touch: n x every record is a multiple of 16)
        CHECK(ok.out[0].at == ok.round[4].at + ok.round[4].bytes, "the good set's arrays touch");
        CHECK(!rtw::ranges_overlap(100, 10, 110, 10) && rtw::ranges_overlap(100, 11, 110, 10) &&
                  !rtw::ranges_overlap(100, 0, 90, 100) && rtw::ranges_overlap(90, 100, 100, 1),
              "ranges_overlap");
        // short, NULL, misaligned (device only), too many
        for (int k = 0; k < 13; ++k) {
            Arrays bad = ok;
            PathArray& a = k < 3 ? bad.in[k] : k < 8 ? bad.round[k - 3] : bad.out[k - 8];
            a.bytes -= 1;
            CHECK(strstr(check(bad, n, elem, slots, true), "smaller"), "array %d one byte short", k);
            CHECK(!*check(bad, n, elem, slots, false), "array %d: the host form has no sizes", k);
            a = (k < 3 ? ok.in[k] : k < 8 ? ok.round[k - 3] : ok.out[k - 8]);
            a.at += 2;
            CHECK(strstr(check(bad, n, elem, slots, true), "aligned"), "array %d misaligned", k);
            a.at = 0;
            CHECK(strstr(check(bad, n, elem, slots, true), "NULL"), "array %d NULL", k);
            CHECK(strstr(check(bad, n, elem, slots, false), "NULL"), "array %d NULL (host)", k);
        }
        // a row slice is aligned: one record further on
        Arrays slice = ok;
        const rtw::PathRecords r = rtw::path_records(elem);
        slice.round[1].at += r.vec3, slice.round[1].bytes += r.vec3;
        slice.in[2].at += r.slot, slice.in[2].bytes += r.slot;
        CHECK(!*check(slice, n - 1, elem, slots, true), "row slices: %s", check(slice, n - 1, elem, slots, true));
        Arrays bad = ok;
        bad.colour.bytes -= 1;
        CHECK(strstr(check(bad, n, elem, slots, true), "colour is smaller"), "colour short");
        bad.colour.at = 0;
        CHECK(strstr(check(bad, n, elem, slots, true), "colour is NULL"), "colour NULL");
        CHECK(!*check(bad, n, elem, 0, true), "no colour slots, no colour array");
        CHECK(strstr(check(ok, (1ull << 32) + 1, elem, slots, false), "2^32"), "n > 2^32");
        CHECK(strstr(check(ok, n, elem, (1ull << 32) + 1, false), "2^32"), "slots > 2^32");
    }
}

int main() {
    plans();
    arrays();
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
