// direct_plan_check.cpp -- CPU check of what rtw_direct_light checks and launches
// (host/direct_plan.hpp) on the plan of the other ray queries (host/query_plan.cpp),
// in the style of nee_plan_check.cpp.  Built and run by tests/test_direct_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> direct_plan_check.cpp \
//       <csrc>/host/{direct_plan,query_plan,render_plan,stage_scene,bvh,rtw_host}.cpp -o direct_plan_check
//
// The size and alignment table of the four arrays, the refusals in their order, the
// n * S limit of the records, and a sweep of the tuning keys over the scene
// families: every plan names a direct_light_kernel that exists, with the
// closest-hit query's LDS at its offsets and the light BVH's stacks behind it.
//
// `direct_plan_check kernels` only prints the kernel table, one
// "direct <f32|f64> <world> <robust>" line each.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <tuple>

#include "direct_kernels.h"
#include "host/direct_plan.hpp"
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
                if (rtw::direct_kernel_exists(f64 != 0, world, robust != 0)) {
                    printf("direct %s %d %d\n", f64 ? "f64" : "f32", world, robust);
                    ++n;
                }
    printf("%d kernels\n", n);
    return 0;
}

static void sizes_and_refusals() {
    // the table: bytes for n = 5 points, S = 3 samples, and the alignments
    const rtw::DirectSizes d = rtw::direct_sizes(true, 5, 3), f = rtw::direct_sizes(false, 5, 3);
    CHECK(d.points.bytes == 5 * 48 && d.points.align == 16, "f64 points %zu / %u", d.points.bytes, d.points.align);
    CHECK(f.points.bytes == 5 * 24 && f.points.align == 8, "f32 points %zu / %u", f.points.bytes, f.points.align);
    CHECK(d.direct.bytes == 5 * 24 && d.direct.align == 8 && f.direct.bytes == 5 * 24 && f.direct.align == 8,
          "direct is n x 3 f64 in both precisions");
    CHECK(d.samples.bytes == 15 * 96 && d.samples.align == 16 && f.samples.bytes == 15 * 48 && f.samples.align == 16,
          "samples %zu / %zu", d.samples.bytes, f.samples.bytes);
    CHECK(d.sample_ids.bytes == 15 * 16 && d.sample_ids.align == 16 && f.sample_ids.bytes == 15 * 16 &&
              f.sample_ids.align == 16, "sample_ids");
    CHECK(rtw::kDirectSampleValues == 12 && rtw::kDirectIdValues == 4 && rtw::kQueryDirectLight == 8, "the constants");

    alignas(16) static unsigned char buf[4096];
    const char* text = nullptr;
    rtw::DirectArgs ok;
    ok.points = buf, ok.n = 5, ok.n_samples = 3, ok.t_min = 1e-9, ok.direct = buf + 1024;
    CHECK(rtw::direct_check(ok, true, 2, &text) == RTW_OK && !*text, "a good host call: %s", text);
    auto refused = [&](rtw::DirectArgs a, bool f64, uint32_t n_list, const char* needle, const char* what) {
        const char* t = "";
        const int rc = rtw::direct_check(a, f64, n_list, &t);
        CHECK(rc == RTW_E_INVALID && strstr(t, needle), "%s: rc %d, \"%s\"", what, rc, t);
    };
    rtw::DirectArgs a = ok;
    a.points = nullptr;
    refused(a, true, 2, "points is NULL", "NULL points");
    a = ok, a.direct = nullptr;
    refused(a, true, 2, "direct is NULL", "NULL direct");
    for (double t : {-1.0, (double)NAN, (double)INFINITY}) {
        a = ok, a.t_min = t;
        refused(a, true, 2, "t_min", "a bad t_min");
    }
    a = ok, a.n_samples = 0;
    refused(a, true, 2, "n_samples", "n_samples == 0");
    refused(ok, true, 0, "empty", "an empty light list");
    a = ok, a.n = ((uint64_t)1 << 40) + 1;
    refused(a, true, 2, "2^40", "n over 2^40");
    // n = 0: the NULL arrays pass, the scalar arguments are still checked
    a = rtw::DirectArgs{}, a.n_samples = 1;
    CHECK(rtw::direct_check(a, true, 2, &text) == RTW_OK, "n = 0 passes");
    a.n_samples = 0;
    refused(a, true, 2, "n_samples", "n = 0 with n_samples == 0");
    a.n_samples = 1;
    refused(a, true, 0, "empty", "n = 0 with an empty list");
    // the n * S limit: only when records are asked for, exactly above 2^32
    a = ok, a.n = (uint64_t)1 << 31, a.n_samples = 2;
    CHECK(rtw::direct_check(a, true, 2, &text) == RTW_OK, "2^32 pairs without records");
    a.samples = buf;
    CHECK(rtw::direct_check(a, true, 2, &text) == RTW_OK, "2^32 records pass");
    a.n += 1;
    refused(a, true, 2, "2^32", "2^32 + 2 records (samples)");
    a.samples = nullptr, a.sample_ids = buf;
    refused(a, true, 2, "2^32", "2^32 + 2 records (sample_ids)");
    a.sample_ids = nullptr;
    CHECK(rtw::direct_check(a, true, 2, &text) == RTW_OK, "2^32 + 2 pairs without records");

    // the device form: sizes and alignments
    for (int f64 = 0; f64 < 2; ++f64) {
        const rtw::DirectSizes s = rtw::direct_sizes(f64 != 0, 5, 3);
        rtw::DirectArgs dv = ok;
        dv.device = true;
        dv.samples = buf + 2048, dv.sample_ids = buf + 3584;
        dv.points_bytes = s.points.bytes, dv.direct_bytes = s.direct.bytes;
        dv.samples_bytes = s.samples.bytes, dv.sample_ids_bytes = s.sample_ids.bytes;
        CHECK(rtw::direct_check(dv, f64 != 0, 2, &text) == RTW_OK, "a good device call: %s", text);
        a = dv, a.points_bytes -= 1;
        refused(a, f64 != 0, 2, "d_points", "short points");
        a = dv, a.direct_bytes -= 1;
        refused(a, f64 != 0, 2, "d_direct", "short direct");
        a = dv, a.samples_bytes -= 1;
        refused(a, f64 != 0, 2, "d_samples", "short samples");
        a = dv, a.sample_ids_bytes -= 1;
        refused(a, f64 != 0, 2, "d_sample_ids", "short sample_ids");
        // the optional arrays absent: their sizes are not looked at
        a = dv, a.samples = nullptr, a.sample_ids = nullptr, a.samples_bytes = 0, a.sample_ids_bytes = 0;
        CHECK(rtw::direct_check(a, f64 != 0, 2, &text) == RTW_OK, "no records: %s", text);
        a = dv, a.points = buf + 8;
        if (f64) refused(a, true, 2, "aligned", "f64 points 8 B off");
        else CHECK(rtw::direct_check(a, false, 2, &text) == RTW_OK, "f32 points on 8 B: %s", text);
        a = dv, a.points = buf + 4;
        refused(a, f64 != 0, 2, "aligned", "points 4 B off");
        a = dv, a.direct = buf + 1024 + 8;
        CHECK(rtw::direct_check(a, f64 != 0, 2, &text) == RTW_OK, "direct on 8 B: %s", text);
        a = dv, a.direct = buf + 1024 + 4;
        refused(a, f64 != 0, 2, "aligned", "direct 4 B off");
        a = dv, a.samples = buf + 2048 + 8;
        refused(a, f64 != 0, 2, "aligned", "samples 8 B off");
        a = dv, a.sample_ids = buf + 3584 + 8;
        refused(a, f64 != 0, 2, "aligned", "sample_ids 8 B off");
    }
}

template <typename R>
static void sweep(const char* name, const rtw_scene& s, int* n_plans, int* n_light_bvh) {
    for (uint32_t light_grid : {8u, 0u})
        for (uint32_t light_bvh_min : {64u, 1000u}) {
            rtw::RenderKnobs k;
            k.light_grid = light_grid;
            k.light_bvh_min = light_bvh_min;
            rtw::DevScene<R> ds{};   // as rtw_set_scene stages it (only the light keys change the staging)
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
                            const rtw::DirectPlan d = rtw::plan_direct(q, sizeof(R) == 8);
                            ++*n_plans;
                            const char* pr = sizeof(R) == 4 ? "f32" : "f64";
                            CHECK(d.err == RTW_OK, "%s %s: world %d: %s", name, pr, q.world, d.err_text);
                            CHECK(rtw::direct_kernel_exists(sizeof(R) == 8, q.world, q.robust != 0),
                                  "%s %s: no direct_light_kernel <%d, %u>", name, pr, q.world, q.robust);
                            // the closest hit's bytes at its offsets, the light BVH's stacks behind them
                            if (q.light_path == rtw::kLightBvh) {
                                ++*n_light_bvh;
                                CHECK(d.light_off >= q.hit_lds && d.light_off % 16 == 0 && d.light_off < q.hit_lds + 16 &&
                                          d.lds == d.light_off + (size_t)rtw::kQueryBlock * q.light_stack * sizeof(int32_t),
                                      "%s %s: light BVH stacks at %u of %zu (hit %zu)", name, pr, d.light_off, d.lds,
                                      q.hit_lds);
                            } else {
                                CHECK(d.light_off == 0 && d.lds == q.hit_lds, "%s %s: LDS %zu, hit %zu", name, pr, d.lds,
                                      q.hit_lds);
                            }
                            CHECK(d.lds <= rtw::kLdsLimit && d.lds >= rtw::kQueryLdsMin, "%s %s: LDS %zu", name, pr,
                                  d.lds);
                        }
        }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "kernels")) return print_kernels();
    sizes_and_refusals();
    // a plan whose LDS does not fit is refused, not launched
    rtw::QueryPlan big;
    big.world = rtw::kWorldBvhLds;
    big.hit_lds = rtw::kLdsLimit - 64;
    big.light_path = rtw::kLightBvh;
    big.light_stack = 8;
    CHECK(rtw::plan_direct(big, true).err == RTW_E_UNSUPPORTED, "an LDS over the limit is refused");
    big.light_path = rtw::kLightGrid;
    CHECK(rtw::plan_direct(big, true).err == RTW_OK, "the same world without the light BVH fits");
    CHECK(rtw::plan_direct(big, false).err == RTW_OK && rtw::plan_direct(rtw::QueryPlan{}, true).err == RTW_OK,
          "the default plan");
    big.robust = 1;
    CHECK(rtw::plan_direct(big, true).err == RTW_E_UNSUPPORTED, "no robust f64 kernel");

    const auto simple_t = rtw::scenes::simple(0x5EED0001, 11);
    const rtw::FlatScene simple_f = rtw::flatten(std::get<0>(simple_t), std::get<1>(simple_t));
    const rtw_scene simple = simple_f.view();
    rtw_scene lights64 = simple;
    lights64.lights = simple.spheres;
    lights64.n_lights = 64;
    lights64.light_kinds = nullptr;
    rtw_scene s63 = simple;
    s63.n_spheres = 63;
    const auto box_t = rtw::scenes::cornell_box();
    const rtw::FlatScene box_f = rtw::flatten(std::get<0>(box_t), std::get<1>(box_t));
    const rtw_scene box = box_f.view();
    int n_plans = 0, n_light_bvh = 0;
    const std::pair<const char*, const rtw_scene*> scenes[] = {
        {"simple", &simple}, {"63 spheres", &s63}, {"64 lights", &lights64}, {"cornell_box", &box}};
    for (const auto& sc : scenes) {
        sweep<float>(sc.first, *sc.second, &n_plans, &n_light_bvh);
        sweep<double>(sc.first, *sc.second, &n_plans, &n_light_bvh);
    }
    printf("sweep: %d plans, %d with the light BVH\n", n_plans, n_light_bvh);
    CHECK(n_plans == 4 * 2 * 2 * 2 * 3 * 4 * 3 * 2, "sweep: %d plans without an error", n_plans);
    CHECK(n_light_bvh > 0, "no plan walks the light BVH");
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
