// features_plan_check.cpp -- CPU check of the feature pass's plan: plan_query
// (host/query_plan.cpp) with the camera's center.  Built and run by
// tests/test_features_host.py like query_plan_check.cpp:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> features_plan_check.cpp \
//       <csrc>/host/{query_plan,render_plan,stage_scene,bvh,rtw_host}.cpp -o features_plan_check
//
// For every tuning of a sweep the pass's world and f32 test form are the render
// plan's for the same camera -- also for a camera far from the scene, where
// knob robust = 2 resolves otherwise than from the origin -- its stack and LDS
// are the query's, and the plan names a kernel of the table.
//
// `features_plan_check kernels` only prints the kernel table (features_kernels.h:
// the launcher instantiates what hit_kernel_exists names), one
// "features <f32|f64> <world> <robust>" line each.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <tuple>

#include "features_kernels.h"
#include "host/query_plan.hpp"
#include "host/rtw_host.hpp"
#include "host/stage_scene.hpp"
#include "host/tiles.hpp"

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

template <typename R>
static void sweep(const char* name, const rtw_scene& s, const rtw_camera& cam, int* n_plans, int* n_robust) {
    rtw::RenderKnobs k;
    rtw::DevScene<R> ds{};
    const uint32_t leaf = rtw::auto_leaf(k.bvh_leaf, s.n_spheres, sizeof(R) == 8);
    rtw::stage_scene<R>(&s, &ds, 0, leaf, 4u, 0.0);
    const rtw::SceneScale scale = rtw::scene_scale(&s, ds);
    const uint32_t nt = rtw::tiles_for_rank(cam.image_width, cam.image_height, 0, 1);
    for (int accel : {RTW_ACCEL_AUTO, RTW_ACCEL_BRUTE, RTW_ACCEL_BVH})
        for (int bvh_kind : {0, 1, 2, 3})
            for (int robust : {0, 1, 2})
                for (int world_pref : {0, 1})
                    for (size_t bvh_lds_max : {(size_t)0, (size_t)1}) {
                        k.accel = accel;
                        k.bvh_kind = bvh_kind;
                        k.robust = robust;
                        k.world_pref = world_pref;
                        k.bvh_lds_max = bvh_lds_max;
                        const rtw::RenderPlan p = rtw::plan_render<R>(k, ds, cam, nt, 1, scale);
                        const rtw::QueryPlan f = rtw::plan_query<R>(k, ds, scale, cam.center);
                        const rtw::QueryPlan q = rtw::plan_query<R>(k, ds, scale);
                        char what[160];
                        snprintf(what, sizeof what, "%s %s: accel %d bvh_kind %d robust %d lds %d bvh_lds_max %zu", name,
                                 sizeof(R) == 4 ? "f32" : "f64", accel, bvh_kind, robust, world_pref, bvh_lds_max);
                        CHECK((p.err != RTW_OK) == (f.err != RTW_OK), "%s: render error %d, features error %d", what,
                              p.err, f.err);
                        if (p.err != RTW_OK || f.err != RTW_OK) continue;
                        ++*n_plans;
                        CHECK(f.world == p.world && f.accel == p.accel, "%s: the pass runs world %d, the render %d", what,
                              f.world, p.world);
                        CHECK(f.robust == (sizeof(R) == 4 ? p.robust : 0u), "%s: test form %u, the render's %u", what,
                              f.robust, p.robust);
                        CHECK(f.stack == q.stack && f.hit_lds == q.hit_lds && f.hit_lds <= rtw::kLdsLimit,
                              "%s: stack %u lds %zu, the query's %u %zu", what, f.stack, f.hit_lds, q.stack, q.hit_lds);
                        CHECK(rtw::hit_kernel_exists(sizeof(R) == 8, f.world, f.robust != 0),
                              "%s: plans <%d, %u>, which does not exist", what, f.world, f.robust);
                        if (f.robust != q.robust) ++*n_robust;
                    }
}

static int print_kernels() {
    int n = 0;
    for (int f64 = 0; f64 < 2; ++f64)
        for (int robust = 0; robust < 2; ++robust)
            for (int world = -1; world <= rtw::kWorldBvhLds + 1; ++world)
                if (rtw::hit_kernel_exists(f64 != 0, world, robust != 0)) {
                    printf("features %s %d %d\n", f64 ? "f64" : "f32", world, robust);
                    ++n;
                }
    printf("%d kernels\n", n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "kernels")) return print_kernels();
    static_assert(rtw::kFeatureChannels == 8 && rtw::kFeatureNextTile == rtw::kQueryCounters,
                  "8 channels; the tile counter follows the query counters");

    const auto simple_t = rtw::scenes::simple(0x5EED0001, 11);
    const rtw::FlatScene simple_f = rtw::flatten(std::get<0>(simple_t), std::get<1>(simple_t));
    const rtw_scene simple = simple_f.view();
    rtw::CameraBuilder near_b = std::get<2>(simple_t);
    const rtw_camera near_cam =
        near_b.with_image_width(16).with_image_height(16).with_samples_per_pixel(4).with_max_depth(5).build().raw();
    // the same scene from far away: f32 rays lose the small spheres' digits, and knob
    // robust = 2 turns the closest-approach tests on for this camera, not for the origin
    rtw::CameraBuilder far_b = std::get<2>(simple_t);
    const rtw_camera far_cam = far_b.with_lookfrom({13.0e5, 2.0e5, 3.0e5})
                                   .with_image_width(16)
                                   .with_image_height(16)
                                   .with_samples_per_pixel(4)
                                   .with_max_depth(5)
                                   .build()
                                   .raw();
    int n_plans = 0, n_near = 0, n_far = 0;
    sweep<float>("simple", simple, near_cam, &n_plans, &n_near);
    sweep<double>("simple", simple, near_cam, &n_plans, &n_near);
    sweep<float>("simple far", simple, far_cam, &n_plans, &n_far);
    sweep<double>("simple far", simple, far_cam, &n_plans, &n_far);
    printf("sweep: %d plans, the camera changes the test form in %d (near) and %d (far)\n", n_plans, n_near, n_far);
    CHECK(n_plans == 4 * 3 * 4 * 3 * 2 * 2, "sweep: %d plans without an error", n_plans);
    CHECK(n_near == 0, "the near camera resolves robust as the origin does");
    CHECK(n_far > 0, "the far camera never changed the test form: the case is vacuous");
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
