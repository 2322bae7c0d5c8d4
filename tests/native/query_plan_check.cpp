// query_plan_check.cpp -- CPU check of the ray queries' plan (host/query_plan.cpp)
// on scenes staged by host/stage_scene.cpp, in the style of plan_check.cpp.
// Built and run by tests/test_query_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> query_plan_check.cpp \
//       <csrc>/host/{query_plan,render_plan,stage_scene,bvh,rtw_host}.cpp -o query_plan_check
//
// Known answers: the world, stack, LDS and light path of the scene families of
// plan_check.cpp (simple, 63 / 64 spheres, 64 lights with the grid and with the
// light BVH, textured, cuboid, emissive).  The LDS figures are query_kernels.h's
// layout evaluated by hand from the staged counts plan_check.cpp pins:
//   world 5: 4 * (stack * 256 + steal) + nodes * 64 + spheres * 16 + pad8(spheres) * 4
//            (steal = 576 f32 / 1344 f64 B per wave)
//     simple f32: 4 * (9 * 256 + 576) + 156 * 64 + 484 * 16 + 488 * 4 = 31200
//     simple f64: 4 * (9 * 256 + 1344) + 9984 + 7744 + 1952 = 34272
//   world 3 / 2: 4 * (9 * 256 + steal) = 11520 / 14592; world 4: 4 * (14 * 256 + steal) = 16640 / 19712
//   world 1: spheres * sizeof(R4<R>), at least 64; world 0: 64 (the counters' block)
// Then a sweep of the tuning keys over the scenes: the query's world is
// plan_render's for the same knobs, its LDS is within the device's and never
// more than the render's for a tree in LDS, and every plan names kernels that
// exist (query_kernels.h).  The feature pass's parameters (feature_params) are
// held to the camera a render pass sees (render_pass.hpp pass_params), with
// defocus and without.
//
// `query_plan_check kernels` only prints the kernel table, one
// "hit <f32|f64> <world> <robust>" or "light <f32|f64> <path> <robust>" line each.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <tuple>

#include "host/camera_params.hpp"
#include "host/query_plan.hpp"
#include "host/render_pass.hpp"
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
struct Staged {
    rtw::DevScene<R> ds{};
    rtw::SceneScale scale;
};

// as rtw_set_scene stages it
template <typename R>
static Staged<R> stage(const rtw_scene& s, const rtw::RenderKnobs& k) {
    Staged<R> st;
    const uint32_t leaf = rtw::auto_leaf(k.bvh_leaf, s.n_spheres, sizeof(R) == 8);
    const double grid = s.n_lights >= k.light_bvh_min ? k.light_grid / 16.0 : 0.0;
    rtw::stage_scene<R>(&s, &st.ds, 0, leaf, k.light_leaf ? k.light_leaf : 4u, grid);
    st.scale = rtw::scene_scale(&s, st.ds);
    return st;
}

static rtw_camera small_camera(const rtw::CameraBuilder& b0) {
    rtw::CameraBuilder b = b0;
    return b.with_image_width(16).with_image_height(16).with_samples_per_pixel(4).with_max_depth(5).build().raw();
}

static rtw_scene cut(rtw_scene s, uint32_t n) {
    s.n_spheres = n;
    return s;
}

struct Expect {
    int world;
    uint32_t stack;
    size_t hit_lds;
    int light_path;
    uint32_t light_stack;
    size_t light_lds;
};

template <typename R>
static void check_plan(const char* name, const rtw_scene& s, const rtw::RenderKnobs& k, const Expect& e) {
    const Staged<R> st = stage<R>(s, k);
    const rtw::QueryPlan q = rtw::plan_query<R>(k, st.ds, st.scale);
    const char* pr = sizeof(R) == 4 ? "f32" : "f64";
    printf("query plan %-18s %s: world %d robust %u stack %u lds %zu light path %d stack %u lds %zu\n", name, pr,
           q.world, q.robust, q.stack, q.hit_lds, q.light_path, q.light_stack, q.light_lds);
    CHECK(q.err == RTW_OK, "%s %s: error %d %s", name, pr, q.err, q.err_text);
    CHECK(q.world == e.world && q.stack == e.stack && q.hit_lds == e.hit_lds,
          "%s %s: world %d stack %u lds %zu, expected %d %u %zu", name, pr, q.world, q.stack, q.hit_lds, e.world,
          e.stack, e.hit_lds);
    CHECK(q.light_path == e.light_path && q.light_stack == e.light_stack && q.light_lds == e.light_lds,
          "%s %s: light path %d stack %u lds %zu, expected %d %u %zu", name, pr, q.light_path, q.light_stack,
          q.light_lds, e.light_path, e.light_stack, e.light_lds);
}

template <typename R>
static void sweep(const char* name, const rtw_scene& s, const rtw_camera& cam, int* n_plans) {
    for (uint32_t light_grid : {8u, 0u})
        for (uint32_t light_bvh_min : {64u, 1000u}) {
            rtw::RenderKnobs k;
            k.light_grid = light_grid;
            k.light_bvh_min = light_bvh_min;
            const Staged<R> st = stage<R>(s, k);   // (only the light keys change the staging)
            const uint32_t nt = rtw::tiles_for_rank(cam.image_width, cam.image_height, 0, 1);
            for (int accel : {RTW_ACCEL_AUTO, RTW_ACCEL_BRUTE, RTW_ACCEL_BVH})
                for (int bvh_kind : {0, 1, 2, 3})
                    for (int robust : {0, 1, 2})
                        for (int world_pref : {0, 1})
                            for (size_t bvh_lds_max : {(size_t)0, (size_t)1, rtw::kLdsLimit}) {
                                k.accel = accel;
                                k.bvh_kind = bvh_kind;
                                k.robust = robust;
                                k.world_pref = world_pref;
                                k.bvh_lds_max = bvh_lds_max;
                                const rtw::RenderPlan p = rtw::plan_render<R>(k, st.ds, cam, nt, 1, st.scale);
                                const rtw::QueryPlan q = rtw::plan_query<R>(k, st.ds, st.scale);
                                char what[160];
                                snprintf(what, sizeof what,
                                         "%s %s: accel %d bvh_kind %d robust %d lds %d bvh_lds_max %zu light_grid %u "
                                         "light_bvh_min %u", name, sizeof(R) == 4 ? "f32" : "f64", accel, bvh_kind,
                                         robust, world_pref, bvh_lds_max, light_grid, light_bvh_min);
                                CHECK((p.err != RTW_OK) == (q.err != RTW_OK), "%s: render error %d, query error %d", what,
                                      p.err, q.err);
                                if (p.err != RTW_OK || q.err != RTW_OK) continue;
                                ++*n_plans;
                                CHECK(q.world == p.world && q.accel == p.accel, "%s: the query runs world %d, the render %d",
                                      what, q.world, p.world);
                                CHECK(q.hit_lds <= rtw::kLdsLimit && q.light_lds <= rtw::kLdsLimit && q.hit_lds >= 64 &&
                                          q.light_lds >= 64, "%s: LDS %zu / %zu", what, q.hit_lds, q.light_lds);
                                if (q.world == rtw::kWorldBvhLds)
                                    CHECK(q.hit_lds <= p.launch_lds, "%s: the query stages %zu B, the render %zu", what,
                                          q.hit_lds, p.launch_lds);
                                if (bvh_lds_max == 1 && p.accel == RTW_ACCEL_BVH && bvh_kind == 3)
                                    CHECK(q.world == rtw::kWorldBvhWW, "%s: a tree too big for LDS runs world %d", what,
                                          q.world);
                                CHECK(q.stack >= 1 && q.stack <= rtw::kBvhStack && q.light_stack >= 1 &&
                                          q.light_stack <= rtw::kBvhStack, "%s: stacks %u / %u", what, q.stack,
                                      q.light_stack);
                                const int want_path = st.ds.lref ? rtw::kLightMixed
                                                                 : (p.light_bvh == 2 ? rtw::kLightGrid
                                                                    : p.light_bvh == 1 ? rtw::kLightBvh : rtw::kLightLinear);
                                CHECK(q.light_path == want_path, "%s: light path %d, the render's %d", what, q.light_path,
                                      want_path);
                                CHECK(rtw::hit_kernel_exists(sizeof(R) == 8, q.world, q.robust != 0) &&
                                          rtw::light_kernel_exists(sizeof(R) == 8, q.light_path, q.robust != 0),
                                      "%s: plans hit <%d, %u> / light <%d, %u>, which do not exist", what, q.world,
                                      q.robust, q.light_path, q.robust);
                                CHECK(sizeof(R) == 4 || q.robust == 0, "%s: f64 with robust", what);
                            }
        }
}

// host/camera_params.hpp: a render pass (KParams of render_pass.hpp pass_params)
// and a feature pass (FParams of feature_params) see the same camera, with
// defocus and without
template <typename R>
static void check_camera_fill(const char* name, const rtw_camera& cam, const rtw::DevScene<R>& sc) {
    // the two entry points: a render pass's parameters and a feature pass's
    const rtw::KParams<R> k = rtw::pass_params<R>(sc, cam, 99, 0, 1, rtw::RenderKnobs(), rtw::RenderPlan(),
                                                  rtw::one_shot_pass(cam));
    rtw::QueryPlan q;
    q.stack = 7;
    q.robust = sizeof(R) == 4 ? 1u : 0u;
    const rtw::FParams<R> f = rtw::feature_params<R>(sc, cam, 99, 3, 5, q);
    const char* pr = sizeof(R) == 4 ? "f32" : "f64";
    bool same = k.u_scale == f.u_scale && k.defocus == f.defocus;
    for (int a = 0; a < 3; ++a)
        same = same && k.center[a] == f.center[a] && k.p00[a] == f.p00[a] && k.du[a] == f.du[a] && k.dv[a] == f.dv[a] &&
               k.disk_u[a] == f.disk_u[a] && k.disk_v[a] == f.disk_v[a] && k.bg[a] == f.bg[a];
    CHECK(same, "%s %s: KParams and FParams differ in a camera field", name, pr);
    CHECK(f.center[0] == (R)cam.center[0] && f.p00[1] == (R)cam.pixel00_loc[1] && f.du[0] == (R)cam.pixel_delta_u[0] &&
              f.dv[1] == (R)cam.pixel_delta_v[1] && f.disk_u[0] == (R)cam.defocus_disk_u[0] &&
              f.disk_v[1] == (R)cam.defocus_disk_v[1] && f.bg[2] == (R)cam.background[2],
          "%s %s: a camera field is not the camera's", name, pr);
    // Uniform::new_inclusive(-0.5, 0.5): the largest scale whose top sample stays <= 0.5
    const double max_rand = 1.0 - 2.220446049250313080847e-16;
    CHECK((double)f.u_scale * max_rand + -0.5 <= 0.5 && f.u_scale >= (R)1 && f.u_scale <= (R)(1.0 + 1e-6),
          "%s %s: u_scale %.17g", name, pr, (double)f.u_scale);
    CHECK(f.defocus == (cam.defocus_angle > 2.220446049250313080847e-16 ? 1u : 0u), "%s %s: defocus %u", name, pr,
          f.defocus);
    CHECK(f.seed == 99 && f.W == cam.image_width && f.H == cam.image_height && f.first == 3 && f.end == 8 &&
              f.tiles_x == rtw::tiles_across(f.W) && f.n_tiles == f.tiles_x * rtw::tiles_across(f.H) && f.stack == 7 &&
              f.sc.robust == q.robust && f.sc.n_sph == sc.n_sph && !f.counts && !f.features && !f.ids && !f.counters,
          "%s %s: the pass's own fields", name, pr);
}

static int print_kernels() {
    int n = 0;
    for (int f64 = 0; f64 < 2; ++f64)
        for (int robust = 0; robust < 2; ++robust) {
            for (int world = -1; world <= rtw::kWorldBvhLds + 1; ++world)
                if (rtw::hit_kernel_exists(f64 != 0, world, robust != 0)) {
                    printf("hit %s %d %d\n", f64 ? "f64" : "f32", world, robust);
                    ++n;
                }
            for (int path = -1; path <= rtw::kLightPaths; ++path)
                if (rtw::light_kernel_exists(f64 != 0, path, robust != 0)) {
                    printf("light %s %d %d\n", f64 ? "f64" : "f32", path, robust);
                    ++n;
                }
        }
    printf("%d kernels\n", n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "kernels")) return print_kernels();

    const auto simple_t = rtw::scenes::simple(0x5EED0001, 11);
    const rtw::FlatScene simple_f = rtw::flatten(std::get<0>(simple_t), std::get<1>(simple_t));
    const rtw_scene simple = simple_f.view();
    const rtw_camera cam = small_camera(std::get<2>(simple_t));
    // 64 / 63 lights: the scene's first spheres as its light list
    rtw_scene lights64 = simple;
    lights64.lights = simple.spheres;
    lights64.n_lights = 64;
    lights64.light_kinds = nullptr;
    rtw_scene lights63 = lights64;
    lights63.n_lights = 63;
    const auto tex_t = rtw::scenes::checkered_spheres();
    const rtw::FlatScene tex_f = rtw::flatten(std::get<0>(tex_t), std::get<1>(tex_t));
    const rtw_scene tex = tex_f.view();
    const rtw_camera tex_cam = small_camera(std::get<2>(tex_t));
    const auto box_t = rtw::scenes::cornell_box();
    const rtw::FlatScene box_f = rtw::flatten(std::get<0>(box_t), std::get<1>(box_t));
    const rtw_scene box = box_f.view();
    const rtw_camera box_cam = small_camera(std::get<2>(box_t));
    rtw::HittableList glow_w, glow_l;
    glow_w.add(rtw::Sphere{{0, 0, -1}, 0.5, rtw::Material::lambertian({0.5, 0.5, 0.5})});
    glow_w.add(rtw::Sphere{{0, 1.5, -1}, 0.5, rtw::Material::diffuse_light({4, 4, 4})});
    glow_l.add(rtw::Sphere{{0, 1.5, -1}, 0.5, rtw::Material::diffuse_light({4, 4, 4})});
    const rtw::FlatScene glow_f = rtw::flatten(glow_w, glow_l);
    const rtw_scene glow = glow_f.view();
    const rtw_camera glow_cam = small_camera(rtw::CameraBuilder());
    const rtw_scene s63 = cut(simple, 63), s64 = cut(simple, 64);

    auto knob = [](const char* key, uint32_t v) {
        rtw::RenderKnobs k;
        const std::string s = key;
        if (s == "lds") k.world_pref = (int)v;
        else if (s == "bvh_kind") k.bvh_kind = (int)v;
        else if (s == "bvh_lds_max") k.bvh_lds_max = v;
        else if (s == "light_grid") k.light_grid = v;
        else if (s == "light_bvh_min") k.light_bvh_min = v;
        else if (s == "accel") k.accel = (int)v;
        else if (s != "") abort();
        return k;
    };
    const int LIN = rtw::kLightLinear, LBV = rtw::kLightBvh, LGR = rtw::kLightGrid, MIX = rtw::kLightMixed;
    struct Case {
        const char* name;
        const rtw_scene* scene;
        rtw::RenderKnobs k;
        Expect f32, f64;
    };
    // {world, stack, hit_lds, light path, light stack, light_lds}
    const Case cases[] = {
        {"defaults", &simple, knob("", 0), {5, 9, 31200, LIN, 1, 64}, {5, 9, 34272, LIN, 1, 64}},
        {"bvh_kind 0", &simple, knob("bvh_kind", 0), {2, 9, 11520, LIN, 1, 64}, {2, 9, 14592, LIN, 1, 64}},
        {"bvh_kind 1", &simple, knob("bvh_kind", 1), {3, 9, 11520, LIN, 1, 64}, {3, 9, 14592, LIN, 1, 64}},
        {"bvh_kind 2", &simple, knob("bvh_kind", 2), {4, 14, 16640, LIN, 1, 64}, {4, 14, 19712, LIN, 1, 64}},
        // a tree too big for the LDS allowed: the while-while world from L1 / L2
        {"bvh_lds_max 1", &simple, knob("bvh_lds_max", 1), {3, 9, 11520, LIN, 1, 64}, {3, 9, 14592, LIN, 1, 64}},
        {"brute", &simple, knob("accel", RTW_ACCEL_BRUTE), {1, 1, 484 * 16, LIN, 1, 64}, {1, 1, 484 * 32, LIN, 1, 64}},
        {"63 spheres", &s63, knob("", 0), {1, 1, 63 * 16, LIN, 1, 64}, {1, 1, 63 * 32, LIN, 1, 64}},
        {"63 spheres lds 0", &s63, knob("lds", 0), {0, 1, 64, LIN, 1, 64}, {0, 1, 64, LIN, 1, 64}},
        // 64 spheres: 21 nodes, depth 5: 4 * (5 * 256 + steal) + 21 * 64 + 64 * 16 + 64 * 4
        {"64 spheres", &s64, knob("", 0), {5, 5, 10048, LIN, 1, 64}, {5, 5, 13120, LIN, 1, 64}},
        // the light path flips at 63 / 64 lights, and with light_grid 0 (light BVH, depth 5: 6 entries
        // per lane, 256 * 6 * 4 B); the render's light grid pushes the tree out of LDS (world 3)
        {"63 lights", &lights63, knob("", 0), {5, 9, 31200, LIN, 1, 64}, {5, 9, 34272, LIN, 1, 64}},
        {"64 lights grid 8", &lights64, knob("light_grid", 8), {3, 9, 11520, LGR, 1, 64}, {3, 9, 14592, LGR, 1, 64}},
        {"64 lights grid 0", &lights64, knob("light_grid", 0), {5, 9, 31200, LBV, 6, 6144}, {5, 9, 34272, LBV, 6, 6144}},
        {"64 lights linear", &lights64, knob("light_bvh_min", 65), {5, 9, 31200, LIN, 1, 64}, {5, 9, 34272, LIN, 1, 64}},
        {"64 lights brute", &lights64, knob("accel", RTW_ACCEL_BRUTE), {1, 1, 484 * 16, LIN, 1, 64}, {1, 1, 484 * 32, LIN, 1, 64}},
        // 2 spheres, 1 node
        {"textured", &tex, knob("", 0), {1, 1, 64, LIN, 1, 64}, {1, 1, 64, LIN, 1, 64}},
        {"cornell_box", &box, knob("", 0), {1, 1, 64, MIX, 1, 64}, {1, 1, 64, MIX, 1, 64}},
        {"emissive sphere", &glow, knob("", 0), {1, 1, 64, LIN, 1, 64}, {1, 1, 64, LIN, 1, 64}},
    };
    for (const Case& c : cases) {
        check_plan<float>(c.name, *c.scene, c.k, c.f32);
        check_plan<double>(c.name, *c.scene, c.k, c.f64);
    }
    // the f32 test form: the tuning key, or by the scene's scale seen from the origin
    {
        rtw::RenderKnobs k;
        k.robust = 1;
        const Staged<float> a = stage<float>(simple, k);
        const Staged<double> b = stage<double>(simple, k);
        CHECK(rtw::plan_query<float>(k, a.ds, a.scale).robust == 1 && rtw::plan_query<double>(k, b.ds, b.scale).robust == 0,
              "robust 1: f32 on, f64 never");
        k.robust = 2;
        const Staged<float> t = stage<float>(tex, k);
        CHECK(rtw::plan_query<float>(k, a.ds, a.scale).robust == 0, "simple: robust by scale");
        printf("textured extent %g min radius %g -> robust %u\n", t.scale.extent, t.scale.min_radius,
               rtw::plan_query<float>(k, t.ds, t.scale).robust);
    }
    // a BVH deeper than the kernels' traversal stack is refused as the render refuses it
    {
        const rtw::RenderKnobs k;
        Staged<float> a = stage<float>(simple, k);
        a.ds.bvh_depth = rtw::kBvhStack + 1;
        const rtw::QueryPlan q = rtw::plan_query<float>(k, a.ds, a.scale);
        CHECK(q.err == RTW_E_UNSUPPORTED, "deep BVH: error %d '%s'", q.err, q.err_text);
    }
    {
        rtw::CameraBuilder b = std::get<2>(simple_t);
        const rtw_camera sharp = small_camera(b.with_defocus_angle(0.0));
        const rtw_camera blurred = small_camera(b.with_defocus_angle(0.6).with_focus_dist(10.0));
        CHECK(sharp.defocus_angle == 0.0 && blurred.defocus_angle > 0.0 &&
                  (blurred.defocus_disk_u[0] != 0.0 || blurred.defocus_disk_u[1] != 0.0 || blurred.defocus_disk_u[2] != 0.0),
              "the two cameras: one without defocus, one with a defocus disk");
        const rtw::RenderKnobs k;
        const Staged<float> a = stage<float>(simple, k);
        const Staged<double> b64 = stage<double>(simple, k);
        check_camera_fill<float>("sharp", sharp, a.ds);
        check_camera_fill<double>("sharp", sharp, b64.ds);
        check_camera_fill<float>("defocus", blurred, a.ds);
        check_camera_fill<double>("defocus", blurred, b64.ds);
    }
    {
        int n_plans = 0;
        const std::tuple<const char*, const rtw_scene*, const rtw_camera*> scenes[] = {
            {"simple", &simple, &cam},       {"63 spheres", &s63, &cam},      {"64 spheres", &s64, &cam},
            {"64 lights", &lights64, &cam},  {"63 lights", &lights63, &cam},  {"textured", &tex, &tex_cam},
            {"cornell_box", &box, &box_cam}, {"emissive sphere", &glow, &glow_cam}};
        for (const auto& sc : scenes) {
            sweep<float>(std::get<0>(sc), *std::get<1>(sc), *std::get<2>(sc), &n_plans);
            sweep<double>(std::get<0>(sc), *std::get<1>(sc), *std::get<2>(sc), &n_plans);
        }
        printf("sweep: %d plans\n", n_plans);
        CHECK(n_plans == 8 * 2 * 2 * 2 * 3 * 4 * 3 * 2 * 3, "sweep: %d plans without an error", n_plans);
    }
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
