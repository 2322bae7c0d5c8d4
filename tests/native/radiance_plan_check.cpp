// radiance_plan_check.cpp -- CPU check of what rtw_radiance_rays checks and
// launches (host/radiance_plan.hpp) on the plan of the other ray queries
// (host/query_plan.cpp), in the style of ambient_plan_check.cpp.  Built and run by
// tests/test_radiance_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> radiance_plan_check.cpp \
//       <csrc>/host/{radiance_plan,query_plan,render_plan,stage_scene,bvh,rtw_host}.cpp -o radiance_plan_check
//
// The size and alignment table of the five arrays, the refusals in their order, the
// limits (rays, pairs, record pairs, sample indices), the loop bound of a lane, and
// a sweep of the tuning keys over the scene families: every plan names a
// radiance_kernel that exists, with direct_light_kernel's LDS layout.
//
// `radiance_plan_check kernels` only prints the kernel table, one
// "radiance <f32|f64> <world> <robust>" line each.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <tuple>

#include "host/query_plan.hpp"
#include "host/radiance_plan.hpp"
#include "host/rtw_host.hpp"
#include "host/stage_scene.hpp"
#include "radiance_kernels.h"

// host/rtw_host.cpp's Camera::render drives a device through these; nothing here renders
extern "C" {
rtw_ctx* rtw_create(int, int) { abort(); }
int rtw_create_mask_ex(uint64_t, int, rtw_ctx**) { abort(); }
int rtw_visible_devices(void) { abort(); }
int rtw_set_accel(rtw_ctx*, int) { abort(); }
int rtw_render(rtw_ctx*, const rtw_camera*, const rtw_scene*, uint64_t, double*, rtw_stats*) { abort(); }
const char* rtw_last_error(const rtw_ctx*) { abort(); }
void rtw_destroy(rtw_ctx*) { abort(); }
}

static int g_wrong = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++g_wrong;                   \
            printf("WRONG: " __VA_ARGS__); \
            printf("\n");                \
        }                                \
    } while (0)

static int print_kernels() {
    int n = 0;
    for (int f64 = 0; f64 < 2; ++f64)
        for (int robust = 0; robust < 2; ++robust)
            for (int world = -1; world <= rtw::kWorldBvhLds + 1; ++world)
                if (rtw::radiance_kernel_exists(f64 != 0, world, robust != 0)) {
                    CHECK(rtw::hit_kernel_exists(f64 != 0, world, robust != 0), "not a closest-hit kernel");
                    printf("radiance %s %d %d\n", f64 ? "f64" : "f32", world, robust);
                    ++n;
                }
    printf("%d kernels\n", n);
    return g_wrong ? 1 : 0;
}

static void sizes_and_refusals() {
    // the table: bytes for n = 5 rays, S = 3 samples, and the alignments
    const rtw::RadianceSizes d = rtw::radiance_sizes(true, 5, 3), f = rtw::radiance_sizes(false, 5, 3);
    CHECK(d.rays.bytes == 5 * 48 && d.rays.align == 16, "f64 rays %zu / %u", d.rays.bytes, d.rays.align);
    CHECK(f.rays.bytes == 5 * 24 && f.rays.align == 8, "f32 rays %zu / %u", f.rays.bytes, f.rays.align);
    CHECK(d.radiance.bytes == 5 * 24 && d.radiance.align == 8 && f.radiance.bytes == 5 * 24 && f.radiance.align == 8,
          "radiance is n x 3 f64 in both precisions");
    CHECK(d.rng.bytes == 5 * 32 && d.rng.align == 16 && f.rng.bytes == 5 * 32 && f.rng.align == 16, "rng");
    CHECK(d.colours.bytes == 15 * 24 && d.colours.align == 8, "f64 colours %zu / %u", d.colours.bytes, d.colours.align);
    CHECK(f.colours.bytes == 15 * 12 && f.colours.align == 4, "f32 colours %zu / %u", f.colours.bytes, f.colours.align);
    CHECK(d.segments.bytes == 15 * 4 && d.segments.align == 4 && f.segments.bytes == 15 * 4 && f.segments.align == 4,
          "segments");
    CHECK(rtw::kQueryRadiance == 10, "the stats value");
    CHECK(rtw::kRadianceMaxRays == (uint64_t)1 << 40 && rtw::kRadianceMaxPairs == (uint64_t)1 << 62 &&
              rtw::kRadianceMaxRecordPairs == (uint64_t)1 << 32 && rtw::kRadianceMaxSampleEnd == (uint64_t)1 << 32,
          "the limits");
    // the loop bound of a lane: S * max(max_depth, 1), in 64 bits
    CHECK(rtw::radiance_trip_bound(3, 8) == 24 && rtw::radiance_trip_bound(3, 0) == 3 &&
              rtw::radiance_trip_bound(1, 1) == 1 &&
              rtw::radiance_trip_bound(0xffffffffu, 0xffffffffu) == 0xfffffffe00000001ull,
          "the trip bound");

    alignas(16) static unsigned char buf[8192];
    static const double bg[3] = {0.5, 0.7, 1.0};
    const char* text = nullptr;
    rtw::RadianceArgs ok;
    ok.rays = buf, ok.n = 5, ok.n_samples = 3, ok.background = bg, ok.radiance = buf + 1024;
    CHECK(rtw::radiance_check(ok, true, &text) == RTW_OK && !*text, "a good host call: %s", text);
    auto refused = [&](rtw::RadianceArgs a, bool f64, const char* needle, const char* what) {
        const char* t = "";
        const int rc = rtw::radiance_check(a, f64, &t);
        CHECK(rc == RTW_E_INVALID && strstr(t, needle), "%s: rc %d, \"%s\"", what, rc, t);
    };
    rtw::RadianceArgs a = ok;
    a.rays = nullptr;
    refused(a, true, "rays is NULL", "NULL rays");
    a = ok, a.radiance = nullptr;
    refused(a, true, "radiance is NULL", "NULL radiance");
    a = ok, a.background = nullptr;
    refused(a, true, "background is NULL", "NULL background");
    a = ok, a.n_samples = 0;
    refused(a, true, "n_samples is 0", "n_samples == 0");
    a = ok, a.rng = buf + 2048;
    refused(a, true, "n_samples must be 1", "rng with S = 3");
    a.n_samples = 1;
    CHECK(rtw::radiance_check(a, true, &text) == RTW_OK, "rng with S = 1: %s", text);
    a = ok, a.first_sample = 0xfffffffeu, a.n_samples = 2;
    CHECK(rtw::radiance_check(a, true, &text) == RTW_OK, "samples up to 2^32 - 1: %s", text);
    a.n_samples = 3;
    refused(a, true, "first_sample + n_samples", "a sample index of 2^32");
    a = ok, a.n = ((uint64_t)1 << 40) + 1;
    refused(a, true, "2^40", "n over 2^40");
    // the order: each refusal comes before the ones after it
    a = ok, a.rays = nullptr, a.radiance = nullptr, a.background = nullptr, a.n_samples = 0;
    refused(a, true, "rays is NULL", "rays before radiance");
    a.rays = buf;
    refused(a, true, "radiance is NULL", "radiance before background");
    a.radiance = buf + 1024;
    refused(a, true, "background is NULL", "background before n_samples");
    a.background = bg;
    refused(a, true, "n_samples is 0", "n_samples next");
    a = ok, a.rng = buf + 2048, a.first_sample = 0xffffffffu, a.n_samples = 2, a.n = ((uint64_t)1 << 40) + 1;
    refused(a, true, "n_samples must be 1", "rng before the sample range");
    a.rng = nullptr;
    refused(a, true, "first_sample + n_samples", "the sample range before 2^40");
    a.first_sample = 0, a.n_samples = 0xffffffffu, a.colours = buf;
    refused(a, true, "2^40", "2^40 before the pair limits");
    // n = 0: the NULL arrays pass, the scalar arguments are still checked
    a = rtw::RadianceArgs{}, a.n_samples = 1;
    CHECK(rtw::radiance_check(a, true, &text) == RTW_OK, "n = 0 passes");
    a.n_samples = 0;
    refused(a, true, "n_samples is 0", "n = 0 with n_samples == 0");
    // the pair limit: n * S never wraps 64 bits
    a = ok, a.n = (uint64_t)1 << 40, a.n_samples = 0xffffffffu;
    refused(a, true, "2^62", "2^72 pairs");
    a = ok, a.n = (uint64_t)1 << 40, a.n_samples = 1u << 22;
    CHECK(rtw::radiance_check(a, true, &text) == RTW_OK, "2^62 pairs pass: %s", text);
    a.n_samples += 1;
    refused(a, true, "2^62", "2^62 + 2^40 pairs");
    a.colours = buf;
    refused(a, true, "2^62", "2^62 before 2^32");
    // the n * S limit of the records: only when one is asked for, exactly above 2^32
    a = ok, a.n = (uint64_t)1 << 31, a.n_samples = 2;
    CHECK(rtw::radiance_check(a, true, &text) == RTW_OK, "2^32 pairs without records");
    a.colours = buf;
    CHECK(rtw::radiance_check(a, true, &text) == RTW_OK, "2^32 records pass");
    a.n += 1;
    refused(a, true, "2^32", "2^32 + 2 records (colours)");
    a.colours = nullptr, a.segments = buf;
    refused(a, true, "2^32", "2^32 + 2 records (segments)");
    a.segments = nullptr;
    CHECK(rtw::radiance_check(a, true, &text) == RTW_OK, "2^32 + 2 pairs without records");

    // the device form: sizes and alignments
    for (int f64 = 0; f64 < 2; ++f64) {
        const rtw::RadianceSizes s = rtw::radiance_sizes(f64 != 0, 5, 1);
        rtw::RadianceArgs dv = ok;
        dv.device = true;
        dv.n_samples = 1;
        dv.rng = buf + 2048, dv.colours = buf + 4096, dv.segments = buf + 6144;
        dv.rays_bytes = s.rays.bytes, dv.radiance_bytes = s.radiance.bytes, dv.rng_bytes = s.rng.bytes;
        dv.colours_bytes = s.colours.bytes, dv.segments_bytes = s.segments.bytes;
        CHECK(rtw::radiance_check(dv, f64 != 0, &text) == RTW_OK, "a good device call: %s", text);
        a = dv, a.rays_bytes -= 1;
        refused(a, f64 != 0, "d_rays", "short rays");
        a = dv, a.radiance_bytes -= 1;
        refused(a, f64 != 0, "d_radiance", "short radiance");
        a = dv, a.rng_bytes -= 1;
        refused(a, f64 != 0, "d_rng", "short rng");
        a = dv, a.colours_bytes -= 1;
        refused(a, f64 != 0, "d_colours", "short colours");
        a = dv, a.segments_bytes -= 1;
        refused(a, f64 != 0, "d_segments", "short segments");
        a = dv, a.rays_bytes = a.radiance_bytes = a.rng_bytes = a.colours_bytes = a.segments_bytes = 0;
        refused(a, f64 != 0, "d_rays", "rays first of the short buffers");
        a.rays_bytes = s.rays.bytes;
        refused(a, f64 != 0, "d_radiance", "then radiance");
        a.radiance_bytes = s.radiance.bytes;
        refused(a, f64 != 0, "d_rng", "then rng");
        a.rng_bytes = s.rng.bytes;
        refused(a, f64 != 0, "d_colours", "then colours");
        // the optional arrays absent: their sizes are not looked at
        a = dv, a.rng = a.colours = a.segments = nullptr, a.rng_bytes = a.colours_bytes = a.segments_bytes = 0;
        CHECK(rtw::radiance_check(a, f64 != 0, &text) == RTW_OK, "no rng, no records: %s", text);
        a = dv, a.rays = buf + 8;
        if (f64) refused(a, true, "aligned", "f64 rays 8 B off");
        else CHECK(rtw::radiance_check(a, false, &text) == RTW_OK, "f32 rays on 8 B: %s", text);
        a = dv, a.rays = buf + 4;
        refused(a, f64 != 0, "aligned", "rays 4 B off");
        a = dv, a.radiance = buf + 1024 + 8;
        CHECK(rtw::radiance_check(a, f64 != 0, &text) == RTW_OK, "radiance on 8 B: %s", text);
        a = dv, a.radiance = buf + 1024 + 4;
        refused(a, f64 != 0, "aligned", "radiance 4 B off");
        a = dv, a.rng = buf + 2048 + 8;
        refused(a, f64 != 0, "aligned", "rng 8 B off");
        a = dv, a.colours = buf + 4096 + 4;
        if (f64) refused(a, true, "aligned", "f64 colours 4 B off");
        else CHECK(rtw::radiance_check(a, false, &text) == RTW_OK, "f32 colours on 4 B: %s", text);
        a = dv, a.colours = buf + 4096 + 2;
        refused(a, f64 != 0, "aligned", "colours 2 B off");
        a = dv, a.segments = buf + 6144 + 2;
        refused(a, f64 != 0, "aligned", "segments 2 B off");
    }
}

template <typename R>
static void sweep(const char* name, const rtw_scene& s, int* n_plans, int* n_light_bvh) {
    rtw::RenderKnobs k;
    for (int light_grid : {(int)k.light_grid, 0}) {
        k.light_grid = light_grid;
        rtw::DevScene<R> ds{};   // as rtw_set_scene stages it
        const uint32_t leaf = rtw::auto_leaf(k.bvh_leaf, s.n_spheres, sizeof(R) == 8);
        const double grid = s.n_lights >= k.light_bvh_min ? k.light_grid / 16.0 : 0.0;
        rtw::stage_scene<R>(&s, &ds, 0, leaf, k.light_leaf ? k.light_leaf : 4u, grid);
        const rtw::SceneScale scale = rtw::scene_scale(&s, ds);
        for (int accel : {RTW_ACCEL_AUTO, RTW_ACCEL_BRUTE, RTW_ACCEL_BVH})
            for (int bvh_kind : {0, 1, 2, 3})
                for (int robust : {0, 1, 2}) {
                    k.accel = accel;
                    k.bvh_kind = bvh_kind;
                    k.robust = robust;
                    const rtw::QueryPlan q = rtw::plan_query<R>(k, ds, scale);
                    if (q.err != RTW_OK) continue;
                    const rtw::RadiancePlan r = rtw::plan_radiance(q, sizeof(R) == 8);
                    ++*n_plans;
                    const char* pr = sizeof(R) == 4 ? "f32" : "f64";
                    CHECK(r.err == RTW_OK, "%s %s: world %d: %s", name, pr, q.world, r.err_text);
                    CHECK(rtw::radiance_kernel_exists(sizeof(R) == 8, q.world, q.robust != 0),
                          "%s %s: no radiance_kernel <%d, %u>", name, pr, q.world, q.robust);
                    // direct_light_kernel's layout: the closest hit's bytes, then the light BVH's stacks
                    const bool lbvh = q.light_path == rtw::kLightBvh;
                    *n_light_bvh += lbvh ? 1 : 0;
                    CHECK(r.lds == rtw::direct_lds(q.hit_lds, q.light_path, q.light_stack) && r.lds <= rtw::kLdsLimit &&
                              r.lds >= rtw::kQueryLdsMin,
                          "%s %s: LDS %zu, hit %zu", name, pr, r.lds, q.hit_lds);
                    if (lbvh)
                        CHECK(r.light_off % 16 == 0 && r.light_off >= q.hit_lds &&
                                  r.lds == r.light_off + rtw::query_light_lds(rtw::kLightBvh, q.light_stack),
                              "%s %s: the light BVH's stacks at %u of %zu", name, pr, r.light_off, r.lds);
                    else
                        CHECK(r.light_off == 0 && r.lds == q.hit_lds, "%s %s: no light stacks", name, pr);
                }
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "kernels")) return print_kernels();
    sizes_and_refusals();
    rtw::QueryPlan odd;
    CHECK(rtw::plan_radiance(odd, true).err == RTW_OK && rtw::plan_radiance(odd, false).err == RTW_OK, "the default plan");
    odd.robust = 1;
    CHECK(rtw::plan_radiance(odd, true).err == RTW_E_UNSUPPORTED, "no robust f64 kernel");
    CHECK(rtw::plan_radiance(odd, false).err == RTW_OK, "a robust f32 kernel");
    odd = rtw::QueryPlan{};
    odd.hit_lds = rtw::kLdsLimit;
    odd.light_path = rtw::kLightBvh;
    CHECK(rtw::plan_radiance(odd, true).err == RTW_E_UNSUPPORTED, "LDS beyond the device's is refused");

    const auto simple_t = rtw::scenes::simple(0x5EED0001, 11);
    const rtw::FlatScene simple_f = rtw::flatten(std::get<0>(simple_t), std::get<1>(simple_t));
    const rtw_scene simple = simple_f.view();
    rtw_scene l64 = simple;      // the first 64 spheres as the light list: the grid, or the light BVH
    l64.lights = simple.spheres;
    l64.n_lights = 64;
    l64.light_kinds = nullptr;
    rtw_scene s63 = simple;
    s63.n_spheres = 63;
    const auto box_t = rtw::scenes::cornell_box();
    const rtw::FlatScene box_f = rtw::flatten(std::get<0>(box_t), std::get<1>(box_t));
    const rtw_scene box = box_f.view();
    int n_plans = 0, n_light_bvh = 0;
    const std::pair<const char*, const rtw_scene*> scenes[] = {
        {"simple", &simple}, {"63 spheres", &s63}, {"64 lights", &l64}, {"cornell_box", &box}};
    for (const auto& sc : scenes) {
        sweep<float>(sc.first, *sc.second, &n_plans, &n_light_bvh);
        sweep<double>(sc.first, *sc.second, &n_plans, &n_light_bvh);
    }
    printf("sweep: %d plans, %d on the light BVH\n", n_plans, n_light_bvh);
    CHECK(n_plans == 4 * 2 * 2 * 3 * 4 * 3, "sweep: %d plans without an error", n_plans);
    CHECK(n_light_bvh > 0, "no plan of the sweep walks the light BVH");
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
