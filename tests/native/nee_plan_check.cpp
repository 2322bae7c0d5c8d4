// nee_plan_check.cpp -- CPU check of what the any-hit and light-sample queries
// launch (nee_kernels.h) on the plan of the other ray queries (host/query_plan.cpp),
// in the style of query_plan_check.cpp.  Built and run by tests/test_nee_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> nee_plan_check.cpp \
//       <csrc>/host/{query_plan,render_plan,stage_scene,bvh,rtw_host}.cpp -o nee_plan_check
//
// A sweep of the tuning keys over the scene families: every plan names an
// occlusion_kernel and a light_sample_kernel that exist, with the closest-hit
// query's world and LDS (the any-hit stages the same bytes) and the light pdf's
// path and stack.
//
// `nee_plan_check kernels` only prints the kernel table, one
// "occlusion <f32|f64> <world> <robust>" or "sample <f32|f64> <path> <robust>" line each.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <tuple>

#include "host/query_plan.hpp"
#include "host/rtw_host.hpp"
#include "host/stage_scene.hpp"
#include "nee_kernels.h"

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
        for (int robust = 0; robust < 2; ++robust) {
            for (int world = -1; world <= rtw::kWorldBvhLds + 1; ++world)
                if (rtw::occlusion_kernel_exists(f64 != 0, world, robust != 0)) {
                    printf("occlusion %s %d %d\n", f64 ? "f64" : "f32", world, robust);
                    ++n;
                }
            for (int path = -1; path <= rtw::kLightPaths; ++path)
                if (rtw::light_sample_kernel_exists(f64 != 0, path, robust != 0)) {
                    printf("sample %s %d %d\n", f64 ? "f64" : "f32", path, robust);
                    ++n;
                }
        }
    printf("%d kernels\n", n);
    return 0;
}

template <typename R>
static void sweep(const char* name, const rtw_scene& s, int* n_plans) {
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
                            ++*n_plans;
                            const char* pr = sizeof(R) == 4 ? "f32" : "f64";
                            CHECK(rtw::occlusion_kernel_exists(sizeof(R) == 8, q.world, q.robust != 0),
                                  "%s %s: no occlusion_kernel <%d, %u>", name, pr, q.world, q.robust);
                            CHECK(rtw::light_sample_kernel_exists(sizeof(R) == 8, q.light_path, q.robust != 0),
                                  "%s %s: no light_sample_kernel <%d, %u>", name, pr, q.light_path, q.robust);
                            // the any-hit stages the closest-hit query's bytes at its offsets
                            CHECK(q.hit_lds == rtw::query_hit_lds<R>(q.world, q.stack, ds.n_nodes, ds.n_sph) &&
                                      q.hit_lds <= rtw::kLdsLimit && q.hit_lds >= rtw::kQueryLdsMin,
                                  "%s %s: world %d LDS %zu", name, pr, q.world, q.hit_lds);
                            CHECK(q.light_lds == rtw::query_light_lds(q.light_path, q.light_stack) &&
                                      q.light_lds >= rtw::kQueryLdsMin, "%s %s: light LDS %zu", name, pr, q.light_lds);
                        }
        }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "kernels")) return print_kernels();
    CHECK(rtw::kQueryAnyHit == 2 && rtw::kQueryLightSample == 3, "rtw_query_stats.is_light_pdf values");
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
    int n_plans = 0;
    const std::pair<const char*, const rtw_scene*> scenes[] = {
        {"simple", &simple}, {"63 spheres", &s63}, {"64 lights", &lights64}, {"cornell_box", &box}};
    for (const auto& sc : scenes) {
        sweep<float>(sc.first, *sc.second, &n_plans);
        sweep<double>(sc.first, *sc.second, &n_plans);
    }
    printf("sweep: %d plans\n", n_plans);
    CHECK(n_plans == 4 * 2 * 2 * 2 * 3 * 4 * 3 * 2, "sweep: %d plans without an error", n_plans);
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
