// ambient_plan_check.cpp -- CPU check of what rtw_ambient_occlusion checks and
// launches (host/ambient_plan.hpp) on the plan of the other ray queries
// (host/query_plan.cpp), in the style of direct_plan_check.cpp.  Built and run by
// tests/test_ambient_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> ambient_plan_check.cpp \
//       <csrc>/host/{ambient_plan,query_plan,render_plan,stage_scene,bvh,rtw_host}.cpp -o ambient_plan_check
//
// The size and alignment table of the four arrays, the refusals in their order, the
// limits (points, pairs, record pairs), and a sweep of the tuning keys over the
// scene families: every plan names an ambient_kernel that exists, with the
// closest-hit query's LDS unchanged.
//
// `ambient_plan_check kernels` only prints the kernel table, one
// "ambient <f32|f64> <world> <robust>" line each.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <tuple>

#include "ambient_kernels.h"
#include "host/ambient_plan.hpp"
#include "host/query_plan.hpp"
#include "host/rtw_host.hpp"
#include "host/stage_scene.hpp"

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
                if (rtw::ambient_kernel_exists(f64 != 0, world, robust != 0)) {
                    CHECK(rtw::occlusion_kernel_exists(f64 != 0, world, robust != 0), "not an any-hit kernel");
                    printf("ambient %s %d %d\n", f64 ? "f64" : "f32", world, robust);
                    ++n;
                }
    printf("%d kernels\n", n);
    return g_wrong ? 1 : 0;
}

static void sizes_and_refusals() {
    // the table: bytes for n = 5 points, S = 3 samples, and the alignments
    const rtw::AmbientSizes d = rtw::ambient_sizes(true, 5, 3), f = rtw::ambient_sizes(false, 5, 3);
    CHECK(d.points.bytes == 5 * 48 && d.points.align == 16, "f64 points %zu / %u", d.points.bytes, d.points.align);
    CHECK(f.points.bytes == 5 * 24 && f.points.align == 8, "f32 points %zu / %u", f.points.bytes, f.points.align);
    CHECK(d.open.bytes == 5 * 4 && d.open.align == 4 && f.open.bytes == 5 * 4 && f.open.align == 4,
          "open is n uint32 in both precisions");
    CHECK(d.directions.bytes == 15 * 24 && d.directions.align == 8, "f64 directions %zu / %u", d.directions.bytes,
          d.directions.align);
    CHECK(f.directions.bytes == 15 * 12 && f.directions.align == 4, "f32 directions %zu / %u", f.directions.bytes,
          f.directions.align);
    CHECK(d.occluded.bytes == 15 && d.occluded.align == 1 && f.occluded.bytes == 15 && f.occluded.align == 1, "occluded");
    CHECK(rtw::kQueryAmbient == 9, "the stats value");
    CHECK(rtw::kAmbientMaxPoints == (uint64_t)1 << 40 && rtw::kAmbientMaxPairs == (uint64_t)1 << 62 &&
              rtw::kAmbientMaxRecordPairs == (uint64_t)1 << 32, "the limits");

    alignas(16) static unsigned char buf[4096];
    const char* text = nullptr;
    rtw::AmbientArgs ok;
    ok.points = buf, ok.n = 5, ok.n_samples = 3, ok.t_min = 1e-9, ok.open = buf + 1024;
    CHECK(rtw::ambient_check(ok, true, &text) == RTW_OK && !*text, "a good host call: %s", text);
    auto refused = [&](rtw::AmbientArgs a, bool f64, const char* needle, const char* what) {
        const char* t = "";
        const int rc = rtw::ambient_check(a, f64, &t);
        CHECK(rc == RTW_E_INVALID && strstr(t, needle), "%s: rc %d, \"%s\"", what, rc, t);
    };
    rtw::AmbientArgs a = ok;
    a.points = nullptr;
    refused(a, true, "points is NULL", "NULL points");
    a = ok, a.open = nullptr;
    refused(a, true, "open is NULL", "NULL open");
    for (double t : {-1.0, (double)NAN, (double)INFINITY}) {
        a = ok, a.t_min = t;
        refused(a, true, "t_min", "a bad t_min");
    }
    a = ok, a.n_samples = 0;
    refused(a, true, "n_samples", "n_samples == 0");
    a = ok, a.n = ((uint64_t)1 << 40) + 1;
    refused(a, true, "2^40", "n over 2^40");
    // the order: each refusal comes before the ones after it
    a = ok, a.points = nullptr, a.open = nullptr, a.t_min = -1.0, a.n_samples = 0;
    refused(a, true, "points is NULL", "points before open");
    a.points = buf;
    refused(a, true, "open is NULL", "open before t_min");
    a.open = buf + 1024;
    refused(a, true, "t_min", "t_min before n_samples");
    a.t_min = 0.0;
    refused(a, true, "n_samples", "n_samples last of the four");
    a = ok, a.n = ((uint64_t)1 << 40) + 1, a.n_samples = 0xffffffffu, a.directions = buf;
    refused(a, true, "2^40", "2^40 before the pair limits");
    // n = 0: the NULL arrays pass, the scalar arguments are still checked
    a = rtw::AmbientArgs{}, a.n_samples = 1;
    CHECK(rtw::ambient_check(a, true, &text) == RTW_OK, "n = 0 passes");
    a.n_samples = 0;
    refused(a, true, "n_samples", "n = 0 with n_samples == 0");
    // the pair limit: n * S never wraps 64 bits (2^40 points x 2^32 - 1 samples would)
    a = ok, a.n = (uint64_t)1 << 40, a.n_samples = 0xffffffffu;
    refused(a, true, "2^62", "2^72 pairs");
    a = ok, a.n = (uint64_t)1 << 40, a.n_samples = 1u << 22;
    CHECK(rtw::ambient_check(a, true, &text) == RTW_OK, "2^62 pairs pass: %s", text);
    a.n_samples += 1;
    refused(a, true, "2^62", "2^62 + 2^40 pairs");
    a.directions = buf;
    refused(a, true, "2^62", "2^62 before 2^32");
    // the n * S limit of the records: only when one is asked for, exactly above 2^32
    a = ok, a.n = (uint64_t)1 << 31, a.n_samples = 2;
    CHECK(rtw::ambient_check(a, true, &text) == RTW_OK, "2^32 pairs without records");
    a.directions = buf;
    CHECK(rtw::ambient_check(a, true, &text) == RTW_OK, "2^32 records pass");
    a.n += 1;
    refused(a, true, "2^32", "2^32 + 2 records (directions)");
    a.directions = nullptr, a.occluded = buf;
    refused(a, true, "2^32", "2^32 + 2 records (occluded)");
    a.occluded = nullptr;
    CHECK(rtw::ambient_check(a, true, &text) == RTW_OK, "2^32 + 2 pairs without records");

    // the device form: sizes and alignments
    for (int f64 = 0; f64 < 2; ++f64) {
        const rtw::AmbientSizes s = rtw::ambient_sizes(f64 != 0, 5, 3);
        rtw::AmbientArgs dv = ok;
        dv.device = true;
        dv.directions = buf + 2048, dv.occluded = buf + 3585;   // (bytes: any address)
        dv.points_bytes = s.points.bytes, dv.open_bytes = s.open.bytes;
        dv.directions_bytes = s.directions.bytes, dv.occluded_bytes = s.occluded.bytes;
        CHECK(rtw::ambient_check(dv, f64 != 0, &text) == RTW_OK, "a good device call: %s", text);
        a = dv, a.points_bytes -= 1;
        refused(a, f64 != 0, "d_points", "short points");
        a = dv, a.open_bytes -= 1;
        refused(a, f64 != 0, "d_open", "short open");
        a = dv, a.directions_bytes -= 1;
        refused(a, f64 != 0, "d_directions", "short directions");
        a = dv, a.occluded_bytes -= 1;
        refused(a, f64 != 0, "d_occluded", "short occluded");
        a = dv, a.points_bytes = 0, a.open_bytes = 0, a.directions_bytes = 0, a.occluded_bytes = 0;
        refused(a, f64 != 0, "d_points", "points first of the short buffers");
        a.points_bytes = s.points.bytes;
        refused(a, f64 != 0, "d_open", "then open");
        a.open_bytes = s.open.bytes;
        refused(a, f64 != 0, "d_directions", "then directions");
        // the optional arrays absent: their sizes are not looked at
        a = dv, a.directions = nullptr, a.occluded = nullptr, a.directions_bytes = 0, a.occluded_bytes = 0;
        CHECK(rtw::ambient_check(a, f64 != 0, &text) == RTW_OK, "no records: %s", text);
        a = dv, a.points = buf + 8;
        if (f64) refused(a, true, "aligned", "f64 points 8 B off");
        else CHECK(rtw::ambient_check(a, false, &text) == RTW_OK, "f32 points on 8 B: %s", text);
        a = dv, a.points = buf + 4;
        refused(a, f64 != 0, "aligned", "points 4 B off");
        a = dv, a.open = buf + 1024 + 4;
        CHECK(rtw::ambient_check(a, f64 != 0, &text) == RTW_OK, "open on 4 B: %s", text);
        a = dv, a.open = buf + 1024 + 2;
        refused(a, f64 != 0, "aligned", "open 2 B off");
        a = dv, a.directions = buf + 2048 + 4;
        if (f64) refused(a, true, "aligned", "f64 directions 4 B off");
        else CHECK(rtw::ambient_check(a, false, &text) == RTW_OK, "f32 directions on 4 B: %s", text);
        a = dv, a.directions = buf + 2048 + 2;
        refused(a, f64 != 0, "aligned", "directions 2 B off");
    }
}

template <typename R>
static void sweep(const char* name, const rtw_scene& s, int* n_plans) {
    rtw::RenderKnobs k;
    rtw::DevScene<R> ds{};   // as rtw_set_scene stages it
    const uint32_t leaf = rtw::auto_leaf(k.bvh_leaf, s.n_spheres, sizeof(R) == 8);
    const double grid = s.n_lights >= k.light_bvh_min ? k.light_grid / 16.0 : 0.0;
    rtw::stage_scene<R>(&s, &ds, 0, leaf, k.light_leaf ? k.light_leaf : 4u, grid);
    const rtw::SceneScale scale = rtw::scene_scale(&s, ds);
    for (int accel : {RTW_ACCEL_AUTO, RTW_ACCEL_BRUTE, RTW_ACCEL_BVH})
        for (int bvh_kind : {0, 1, 2, 3})
            for (int robust : {0, 1, 2})
                for (int world_pref : {0, 1}) {
                    k.accel = accel;
                    k.bvh_kind = bvh_kind;
                    k.robust = robust;
                    k.world_pref = world_pref;
                    const rtw::QueryPlan q = rtw::plan_query<R>(k, ds, scale);
                    if (q.err != RTW_OK) continue;
                    const rtw::AmbientPlan a = rtw::plan_ambient(q, sizeof(R) == 8);
                    ++*n_plans;
                    const char* pr = sizeof(R) == 4 ? "f32" : "f64";
                    CHECK(a.err == RTW_OK, "%s %s: world %d: %s", name, pr, q.world, a.err_text);
                    CHECK(rtw::ambient_kernel_exists(sizeof(R) == 8, q.world, q.robust != 0),
                          "%s %s: no ambient_kernel <%d, %u>", name, pr, q.world, q.robust);
                    // the closest hit's bytes, unchanged
                    CHECK(a.lds == q.hit_lds && a.lds <= rtw::kLdsLimit && a.lds >= rtw::kQueryLdsMin,
                          "%s %s: LDS %zu, hit %zu", name, pr, a.lds, q.hit_lds);
                }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "kernels")) return print_kernels();
    sizes_and_refusals();
    rtw::QueryPlan odd;
    CHECK(rtw::plan_ambient(odd, true).err == RTW_OK && rtw::plan_ambient(odd, false).err == RTW_OK, "the default plan");
    odd.robust = 1;
    CHECK(rtw::plan_ambient(odd, true).err == RTW_E_UNSUPPORTED, "no robust f64 kernel");
    CHECK(rtw::plan_ambient(odd, false).err == RTW_OK, "a robust f32 kernel");

    const auto simple_t = rtw::scenes::simple(0x5EED0001, 11);
    const rtw::FlatScene simple_f = rtw::flatten(std::get<0>(simple_t), std::get<1>(simple_t));
    const rtw_scene simple = simple_f.view();
    rtw_scene nolights = simple;   // an empty light list is fine here
    nolights.lights = nullptr;
    nolights.n_lights = 0;
    nolights.light_kinds = nullptr;
    rtw_scene s63 = simple;
    s63.n_spheres = 63;
    const auto box_t = rtw::scenes::cornell_box();
    const rtw::FlatScene box_f = rtw::flatten(std::get<0>(box_t), std::get<1>(box_t));
    const rtw_scene box = box_f.view();
    int n_plans = 0;
    const std::pair<const char*, const rtw_scene*> scenes[] = {
        {"simple", &simple}, {"63 spheres", &s63}, {"no lights", &nolights}, {"cornell_box", &box}};
    for (const auto& sc : scenes) {
        sweep<float>(sc.first, *sc.second, &n_plans);
        sweep<double>(sc.first, *sc.second, &n_plans);
    }
    printf("sweep: %d plans\n", n_plans);
    CHECK(n_plans == 4 * 2 * 3 * 4 * 3 * 2, "sweep: %d plans without an error", n_plans);
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
