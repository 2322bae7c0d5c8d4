// path_plan_check.cpp -- CPU check of what the path queries launch
// (path_kernels.h, host/path_params.hpp) on the plan of the other ray queries
// (host/query_plan.cpp), in the style of nee_plan_check.cpp.  Built and run by
// tests/test_path_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> path_plan_check.cpp \
//       <csrc>/host/{query_plan,render_plan,stage_scene,bvh,rtw_host}.cpp -o path_plan_check
// (the test also builds it with -fsanitize=address,undefined: a host program, run alone)
//
// A sweep of the tuning keys over the scene families: every plan names a
// shade_rays_kernel that exists, on the light pdf's path, stack and LDS, and
// the kernel parameters built from it (shade_params / camera_ray_params) carry
// the plan and the camera as a render's kernel sees it.
//
// `path_plan_check kernels` only prints the kernel table, one
// "camera <f32|f64>" or "shade <f32|f64> <path> <robust>" line each.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <tuple>

#include "host/path_params.hpp"
#include "host/query_plan.hpp"
#include "host/rtw_host.hpp"
#include "host/stage_scene.hpp"
#include "path_kernels.h"

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
    for (int f64 = 0; f64 < 2; ++f64) {
        if (rtw::camera_rays_kernel_exists(f64 != 0)) {
            printf("camera %s\n", f64 ? "f64" : "f32");
            ++n;
        }
        for (int robust = 0; robust < 2; ++robust)
            for (int path = -1; path <= rtw::kLightPaths; ++path)
                if (rtw::shade_rays_kernel_exists(f64 != 0, path, robust != 0)) {
                    printf("shade %s %d %d\n", f64 ? "f64" : "f32", path, robust);
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
            // (the blob holds what the DevScene's pointers point to: kept while they are read)
            const std::vector<unsigned char> blob =
                rtw::stage_scene<R>(&s, &ds, 0, leaf, k.light_leaf ? k.light_leaf : 4u, grid);
            const rtw::SceneScale scale = rtw::scene_scale(&s, ds);
            for (int accel : {RTW_ACCEL_AUTO, RTW_ACCEL_BRUTE, RTW_ACCEL_BVH})
                for (int robust : {0, 1, 2}) {
                    k.accel = accel;
                    k.robust = robust;
                    const rtw::QueryPlan q = rtw::plan_query<R>(k, ds, scale);
                    if (q.err != RTW_OK) continue;
                    ++*n_plans;
                    const char* pr = sizeof(R) == 4 ? "f32" : "f64";
                    const rtw::ShadeLaunch sl = rtw::shade_launch(q);
                    CHECK(rtw::shade_rays_kernel_exists(sizeof(R) == 8, sl.path, sl.robust),
                          "%s %s: no shade_rays_kernel <%d, %d>", name, pr, sl.path, (int)sl.robust);
                    CHECK(sl.path == q.light_path && sl.robust == (q.robust != 0), "%s %s: launch is not the plan's", name, pr);
                    CHECK(sl.lds == rtw::query_light_lds(q.light_path, q.light_stack) && sl.lds >= rtw::kQueryLdsMin &&
                              sl.lds <= rtw::kLdsLimit, "%s %s: light LDS %zu", name, pr, sl.lds);
                    CHECK((sl.path == rtw::kLightMixed) == (ds.lref != nullptr), "%s %s: mixed path %d", name, pr, sl.path);
                    const rtw::SParams<R> p = rtw::shade_params<R>(ds, q, 1000);
                    CHECK(p.n == 1000 && p.stack == q.light_stack && p.sc.robust == q.robust &&
                              p.sc.n_list == ds.n_list && p.sc.lights == ds.lights && p.sc.mat_p == ds.mat_p,
                          "%s %s: shade_params", name, pr);
                    CHECK(!p.rays && !p.hits && !p.ids && !p.rng && !p.next && !p.weight && !p.emitted && !p.event &&
                              !p.pdfs && !p.counters, "%s %s: shade_params leaves the buffers to the caller", name, pr);
                    // the light BVH's stack fits the LDS the launch asks for
                    if (sl.path == rtw::kLightBvh)
                        CHECK((size_t)rtw::kQueryBlock * p.stack * sizeof(int32_t) <= sl.lds, "%s %s: stack %u", name, pr,
                              p.stack);
                }
        }
}

template <typename R>
static void camera_checks(const rtw::CameraBuilder& b, bool defocus) {
    const rtw_camera cam = b.build().raw();
    const rtw::CParams<R> p = rtw::camera_ray_params<R>(cam, 7, 3, 5, 100);
    const char* pr = sizeof(R) == 4 ? "f32" : "f64";
    CHECK(p.W == cam.image_width && p.n_pixels == (uint64_t)cam.image_width * cam.image_height, "%s: image", pr);
    CHECK(p.seed == 7 && p.sample == 3 && p.first_pixel == 5 && p.n == 100, "%s: stream key", pr);
    CHECK(p.defocus == (defocus ? 1u : 0u), "%s: defocus %u", pr, p.defocus);
    for (int a = 0; a < 3; ++a)
        CHECK(p.center[a] == (R)cam.center[a] && p.p00[a] == (R)cam.pixel00_loc[a] && p.du[a] == (R)cam.pixel_delta_u[a] &&
                  p.dv[a] == (R)cam.pixel_delta_v[a] && p.disk_u[a] == (R)cam.defocus_disk_u[a] &&
                  p.disk_v[a] == (R)cam.defocus_disk_v[a], "%s: camera axis %d", pr, a);
    // Uniform::new_inclusive(-0.5, 0.5): the largest draw lands on 0.5 or below
    const double max_rand = 1.0 - 2.220446049250313080847e-16;
    CHECK((double)p.u_scale * max_rand + -0.5 <= 0.5 || sizeof(R) == 4, "%s: u_scale", pr);
    CHECK(!p.pixels && !p.rays && !p.rng && !p.counters, "%s: camera_ray_params leaves the buffers to the caller", pr);
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "kernels")) return print_kernels();
    CHECK(rtw::kQueryCameraRays == 4 && rtw::kQueryShade == 5, "rtw_query_stats.is_light_pdf values");
    CHECK(rtw::kEventMiss == RTW_EVENT_MISS && rtw::kEventAbsorbed == RTW_EVENT_ABSORBED &&
              rtw::kEventReflect == RTW_EVENT_REFLECT && rtw::kEventScatter == RTW_EVENT_SCATTER, "RTW_EVENT_*");
    // the record accesses: the widest the strides allow from a 16-byte aligned base
    CHECK(rtw::record_align(6 * 8) == 16 && rtw::record_align(9 * 8) == 8 && rtw::record_align(3 * 8) == 8 &&
              rtw::record_align(6 * 4) == 8 && rtw::record_align(9 * 4) == 4 && rtw::record_align(3 * 4) == 4 &&
              rtw::record_align(4 * 8) == 16 && rtw::record_align(4 * 4) == 16, "record_align");
    const auto simple_t = rtw::scenes::simple(0x5EED0001, 11);
    const rtw::FlatScene simple_f = rtw::flatten(std::get<0>(simple_t), std::get<1>(simple_t));
    const rtw_scene simple = simple_f.view();
    rtw_scene lights64 = simple;
    lights64.lights = simple.spheres;
    lights64.n_lights = 64;
    lights64.light_kinds = nullptr;
    const auto box_t = rtw::scenes::cornell_box();
    const rtw::FlatScene box_f = rtw::flatten(std::get<0>(box_t), std::get<1>(box_t));
    const rtw_scene box = box_f.view();
    int n_plans = 0;
    const std::pair<const char*, const rtw_scene*> scenes[] = {
        {"simple", &simple}, {"64 lights", &lights64}, {"cornell_box", &box}};
    for (const auto& sc : scenes) {
        sweep<float>(sc.first, *sc.second, &n_plans);
        sweep<double>(sc.first, *sc.second, &n_plans);
    }
    printf("sweep: %d plans\n", n_plans);
    CHECK(n_plans == 3 * 2 * 2 * 2 * 3 * 3, "sweep: %d plans without an error", n_plans);
    rtw::CameraBuilder b = std::get<2>(simple_t);
    camera_checks<float>(b.with_image_width(40).with_image_height(24), false);
    camera_checks<double>(b, false);
    camera_checks<double>(b.with_defocus_angle(2.0).with_focus_dist(10.0), true);
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
