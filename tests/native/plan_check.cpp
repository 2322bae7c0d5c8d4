// plan_check.cpp -- CPU check of the render plan and the longest-tiles-first
// task list (host/render_plan.cpp) on scenes staged by host/stage_scene.cpp.
// Built and run by tests/test_render_plan_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> plan_check.cpp \
//       <csrc>/host/{render_plan,stage_scene,bvh,rtw_host}.cpp -o plan_check
//
// Task lists: every (tile, chunk) exactly once, a tile's entries in increasing
// chunk order, 1..4095 chunks per entry, first chunk < 2^20, tiles by
// non-increasing cost (ties: lower index).
//
// Plans: known answers.  accel / bvh_width / world / chunk are what the
// library before the split into host units reported through rtw_get_stats for
// the same scene and tuning on an MI355X (16 x 16 pixels, 4 spp, depth 5);
// stack / launch_lds are not visible through the ABI: they are that library's
// formula evaluated by hand from the staged scenes' counts, which main()
// pins first.  opts (the kernel's option bits) are the rules of the launcher
// the plan's choice replaced, evaluated by hand per case (below); for the scene
// families of tests/test_gpu_parity.py's variant test they are also what that
// library reported through rtw_last_kernel.
//
// Then a sweep of the tuning keys over the scenes: every plan without an error
// names a kernel variant that exists (rtw_kernels.h variant_exists).
//
// `plan_check variants` only prints the table of variants, one
// "variant <f32|f64> <world> <opts>" line each (tests/test_capi_host.py holds
// it against the library's symbols).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "host/render_plan.hpp"
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

// ---------------------------------------------------------------- task lists
static void check_task_list(const std::vector<uint32_t>& cost, uint32_t n_chunks, uint32_t fixed_group,
                            uint32_t guide_div) {
    rtw::RenderKnobs k;
    k.guide_div = guide_div;
    const std::vector<uint32_t> tab = rtw::build_task_list(cost, n_chunks, fixed_group, rtw::kAutoTasks, k);
    const uint32_t nt = (uint32_t)cost.size();
    char name[96];
    snprintf(name, sizeof name, "tiles %u chunks %u group %u guide_div %u", nt, n_chunks, fixed_group, guide_div);
    CHECK(tab.size() % 2 == 0, "%s: odd table", name);
    std::vector<uint32_t> next(nt, 0);       // the next chunk each tile expects
    std::vector<uint32_t> tile_order;        // tiles in the order they first appear
    for (size_t e = 0; e + 1 < tab.size(); e += 2) {
        const uint32_t tile = tab[e], first = tab[e + 1] & 0xFFFFFu, count = tab[e + 1] >> 20;
        if (tile >= nt) {
            CHECK(false, "%s: tile %u out of range", name, tile);
            return;
        }
        CHECK(count >= 1 && count <= 4095, "%s: entry %zu has %u chunks", name, e / 2, count);
        CHECK(first == next[tile], "%s: tile %u entry starts at chunk %u, expected %u", name, tile, first, next[tile]);
        CHECK((uint64_t)first + count <= n_chunks, "%s: tile %u runs past its chunks", name, tile);
        if (tile_order.empty() || tile_order.back() != tile) tile_order.push_back(tile);
        next[tile] = first + count;
    }
    for (uint32_t t = 0; t < nt; ++t) CHECK(next[t] == n_chunks, "%s: tile %u covered to %u", name, t, next[t]);
    CHECK(tile_order.size() == nt, "%s: %zu tile runs for %u tiles", name, tile_order.size(), nt);
    for (size_t q = 1; q < tile_order.size(); ++q) {
        const uint32_t a = tile_order[q - 1], b = tile_order[q];
        CHECK(cost[a] > cost[b] || (cost[a] == cost[b] && a < b), "%s: tile %u (cost %u) before tile %u (cost %u)",
              name, a, cost[a], b, cost[b]);
    }
}

static void check_task_lists() {
    std::mt19937 rng(20240607);
    for (uint32_t nt : {1u, 2u, 7u, 64u})
        for (uint32_t n_chunks : {1u, 5u, 33u, 4096u, 5000u})
            for (uint32_t fixed_group : {0u, 1u, 4096u})
                for (uint32_t guide_div : {0u, 16384u}) {
                    // random costs with zeros and ties (a few distinct values, one large)
                    std::vector<uint32_t> cost(nt);
                    for (uint32_t& c : cost) {
                        const uint32_t r = rng() % 8;
                        c = r == 0 ? 0u : (r < 6 ? r * 100u : rng() % 100000u);
                    }
                    if (nt > 2) cost[nt / 2] = cost[0];   // a tie for sure
                    check_task_list(cost, n_chunks, fixed_group, guide_div);
                }
}

// --------------------------------------------------------------------- plans
struct Expect {
    const char* name;
    int accel;
    uint32_t bvh_width;
    int world, opts;
    uint32_t chunk, stack;
    size_t launch_lds;
};

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

template <typename R>
static rtw::RenderPlan plan_of(const rtw_scene& s, const rtw_camera& cam, const rtw::RenderKnobs& k) {
    const Staged<R> st = stage<R>(s, k);
    const uint32_t nt = rtw::tiles_for_rank(cam.image_width, cam.image_height, 0, 1);
    const uint32_t chunk = rtw::plan_chunk<R>(k, cam.samples_per_pixel, nt, 0);
    return rtw::plan_render<R>(k, st.ds, cam, nt, chunk, st.scale);
}

template <typename R>
static void check_plan(const rtw_scene& s, const rtw_camera& cam, const rtw::RenderKnobs& k, const Expect& e) {
    const rtw::RenderPlan p = plan_of<R>(s, cam, k);
    const char* pr = sizeof(R) == 4 ? "f32" : "f64";
    printf("plan %-20s %s: accel %d width %u world %d opts %d chunk %u stack %u lds %zu light_bvh %u\n", e.name, pr,
           p.accel, p.bvh_width, p.world, p.opts, p.chunk, p.stack, p.launch_lds, p.light_bvh);
    CHECK(p.err == RTW_OK, "%s %s: error %d %s", e.name, pr, p.err, p.err_text);
    CHECK(p.accel == e.accel && p.bvh_width == e.bvh_width && p.world == e.world && p.chunk == e.chunk,
          "%s %s: accel %d width %u world %d chunk %u, expected %d %u %d %u", e.name, pr, p.accel, p.bvh_width,
          p.world, p.chunk, e.accel, e.bvh_width, e.world, e.chunk);
    CHECK(p.opts == e.opts, "%s %s: opts %d, expected %d", e.name, pr, p.opts, e.opts);
    CHECK(p.stack == e.stack && p.launch_lds == e.launch_lds, "%s %s: stack %u lds %zu, expected %u %zu", e.name, pr,
          p.stack, p.launch_lds, e.stack, e.launch_lds);
}

static rtw::RenderKnobs knob(const char* key, uint32_t v) {
    rtw::RenderKnobs k;
    const std::string s = key;
    if (s == "lds") k.world_pref = (int)v;
    else if (s == "bvh_kind") k.bvh_kind = (int)v;
    else if (s == "bvh_lds_max") k.bvh_lds_max = v;
    else if (s == "light_grid") k.light_grid = v;
    else if (s == "hit64") k.hit64 = v;
    else if (s == "robust") k.robust = (int)v;
    else if (s == "accel") k.accel = (int)v;
    else if (s != "") abort();
    return k;
}

// the first n spheres of a scene
static rtw_scene cut(rtw_scene s, uint32_t n) {
    s.n_spheres = n;
    return s;
}

template <typename R>
static void sweep_plans(const char* name, const rtw_scene& s, const rtw_camera& cam, int* n_plans) {
    for (uint32_t light_grid : {8u, 0u}) {
        rtw::RenderKnobs k;
        k.light_grid = light_grid;
        const Staged<R> st = stage<R>(s, k);   // (only the light grid's key changes the staging)
        const uint32_t nt = rtw::tiles_for_rank(cam.image_width, cam.image_height, 0, 1);
        for (int accel : {RTW_ACCEL_AUTO, RTW_ACCEL_BRUTE, RTW_ACCEL_BVH})
            for (int bvh_kind : {0, 1, 2, 3})
                for (uint32_t hit64 : {0u, 1u})
                    for (int robust : {0, 1, 2})
                        for (int world_pref : {0, 1})
                            for (size_t bvh_lds_max : {(size_t)0, (size_t)1}) {
                                k.accel = accel;
                                k.bvh_kind = bvh_kind;
                                k.hit64 = hit64;
                                k.robust = robust;
                                k.world_pref = world_pref;
                                k.bvh_lds_max = bvh_lds_max;
                                const rtw::RenderPlan p = rtw::plan_render<R>(k, st.ds, cam, nt, 1, st.scale);
                                if (p.err != RTW_OK) continue;
                                ++*n_plans;
                                CHECK(rtw::dev::variant_exists(sizeof(R) == 8, p.world, p.opts),
                                      "%s %s: accel %d bvh_kind %d hit64 %u robust %d lds %d bvh_lds_max %zu light_grid "
                                      "%u plans world %d opts %d, which does not exist", name,
                                      sizeof(R) == 4 ? "f32" : "f64", accel, bvh_kind, hit64, robust, world_pref,
                                      bvh_lds_max, light_grid, p.world, p.opts);
                            }
    }
}

static int print_variants() {
    int n = 0;
    for (int f64 = 0; f64 < 2; ++f64)
        for (int world = -1; world <= rtw::kWorldBvhLds + 1; ++world)
            for (int opts = 0; opts < 64; ++opts)
                if (rtw::dev::variant_exists(f64 != 0, world, opts)) {
                    printf("variant %s %d %d\n", f64 ? "f64" : "f32", world, opts);
                    ++n;
                }
    printf("%d variants\n", n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "variants")) return print_variants();
    check_task_lists();

    const auto simple_t = rtw::scenes::simple(0x5EED0001, 11);
    const rtw::FlatScene simple_f = rtw::flatten(std::get<0>(simple_t), std::get<1>(simple_t));
    const rtw_scene simple = simple_f.view();
    const rtw_camera cam = small_camera(std::get<2>(simple_t));
    // 64 lights: the scene's first 64 spheres as its light list
    rtw_scene lights64 = simple;
    lights64.lights = simple.spheres;
    lights64.n_lights = 64;
    lights64.light_kinds = nullptr;
    const auto tex_t = rtw::scenes::checkered_spheres();
    const rtw::FlatScene tex_f = rtw::flatten(std::get<0>(tex_t), std::get<1>(tex_t));
    const rtw_scene tex = tex_f.view();
    const rtw_camera tex_cam = small_camera(std::get<2>(tex_t));
    const auto box_t = rtw::scenes::cornell_box();
    const rtw::FlatScene box_f = rtw::flatten(std::get<0>(box_t), std::get<1>(box_t));
    const rtw_scene box = box_f.view();
    const rtw_camera box_cam = small_camera(std::get<2>(box_t));
    // spheres only, one of them a DiffuseLight: no quad, cuboid or mixed light list
    rtw::HittableList glow_w, glow_l;
    glow_w.add(rtw::Sphere{{0, 0, -1}, 0.5, rtw::Material::lambertian({0.5, 0.5, 0.5})});
    glow_w.add(rtw::Sphere{{0, 1.5, -1}, 0.5, rtw::Material::diffuse_light({4, 4, 4})});
    glow_l.add(rtw::Sphere{{0, 1.5, -1}, 0.5, rtw::Material::diffuse_light({4, 4, 4})});
    const rtw::FlatScene glow_f = rtw::flatten(glow_w, glow_l);
    const rtw_scene glow = glow_f.view();
    const rtw_camera glow_cam = small_camera(rtw::CameraBuilder());

    // the staged scenes' counts the hand-evaluated stack / launch_lds rest on
    {
        const rtw::RenderKnobs k;
        const Staged<float> a = stage<float>(simple, k);
        const Staged<double> b = stage<double>(simple, k);
        const Staged<float> c = stage<float>(lights64, k);
        const Staged<float> d = stage<float>(lights64, knob("light_grid", 0));
        const Staged<float> e = stage<float>(tex, k);
        const Staged<float> f = stage<float>(cut(simple, 64), k);
        const Staged<double> g = stage<double>(cut(simple, 64), k);
        printf("facts simple: spheres %u lights %u nodes %u depth %u bvh4_stack %u (f64 nodes %u depth %u stack %u)\n",
               a.ds.n_sph, a.ds.n_lights, a.ds.n_nodes, a.ds.bvh_depth, a.ds.bvh4_stack, b.ds.n_nodes, b.ds.bvh_depth,
               b.ds.bvh4_stack);
        printf("facts lights64: lg_on %u lbvh_depth %u (grid 0: lg_on %u lbvh_depth %u)\n", c.ds.lg_on,
               c.ds.lbvh_depth, d.ds.lg_on, d.ds.lbvh_depth);
        printf("facts textured: spheres %u lights %u nodes %u depth %u bvh4_stack %u; simple[:64]: nodes %u depth %u "
               "(f64 %u %u)\n", e.ds.n_sph, e.ds.n_lights, e.ds.n_nodes, e.ds.bvh_depth, e.ds.bvh4_stack, f.ds.n_nodes,
               f.ds.bvh_depth, g.ds.n_nodes, g.ds.bvh_depth);
        CHECK(a.ds.n_sph == 484 && a.ds.n_lights == 19 && a.ds.n_nodes == 156 && a.ds.bvh_depth == 9 &&
                  a.ds.bvh4_stack == 13 && b.ds.n_nodes == 156 && b.ds.bvh_depth == 9 && b.ds.bvh4_stack == 13,
              "scenes::simple stages differently");
        CHECK(c.ds.lg_on == 1 && d.ds.lg_on == 0 && d.ds.lbvh_depth == 5, "the 64-light scene stages differently");
        CHECK(e.ds.n_sph == 2 && e.ds.n_lights == 1 && e.ds.n_nodes == 1 && e.ds.bvh_depth == 1 &&
                  e.ds.bvh4_stack == 0 && e.ds.mat_tex != nullptr, "checkered_spheres stages differently");
        const Staged<float> h = stage<float>(box, k);
        const Staged<float> i = stage<float>(glow, k);
        printf("facts cornell_box: spheres %u lights %u quads %u boxes %u light quads %u; glow: spheres %u lights %u "
               "emissive %u\n", h.ds.n_sph, h.ds.n_lights, h.ds.n_quads, h.ds.n_boxes, h.ds.n_lquads, i.ds.n_sph,
               i.ds.n_lights, i.ds.emissive);
        CHECK(h.ds.n_sph == 1 && h.ds.n_lights == 1 && h.ds.n_quads == 6 && h.ds.n_boxes == 1 && h.ds.n_lquads == 1 &&
                  h.ds.lref != nullptr && !h.ds.mat_tex, "cornell_box stages differently");
        CHECK(i.ds.n_sph == 2 && i.ds.n_lights == 1 && i.ds.emissive == 1 && !i.ds.n_quads && !i.ds.n_boxes &&
                  !i.ds.lref && !i.ds.mat_tex, "the emissive sphere scene stages differently");
        CHECK(f.ds.n_nodes == 21 && f.ds.bvh_depth == 5 && g.ds.n_nodes == 21 && g.ds.bvh_depth == 5,
              "the 64-sphere scene stages differently");
    }

    // {name, accel, bvh_width, world, opts, chunk | stack, launch_lds}; the hand evaluation, per precision R
    // (s4 = sizeof(R4<R>): 16 / 32; steal = 576 / 1344 B per wave; 4 waves per workgroup, f64 `wide` 16):
    //   opts (1 robust, 2 light BVH / grid, 4 textures, 8 quads / cuboids / emitters, 16 f64 hit points):
    //     textured scene 4 + 8; else 8 with a quad, cuboid, mixed light list or DiffuseLight;
    //     f32: + 1 when `robust` (tuning 1, or 2 and (far / smallest radius)^2 * 5.96e-8 > 1e-3, far = the
    //       larger of the spheres' extent and the camera's distance from the origin:
    //       simple and its cuts (15 / 0.2)^2 -> 3.4e-4: off; checkered_spheres (40 / 0.1)^2 -> 9.5e-3: on;
    //       cornell_box (891 / 90)^2, the emissive spheres (2 / 0.5)^2: off);
    //     + 2 with a light BVH / grid (BVH worlds only); f32: + 16 with tuning hit64 unless 8 is set
    //   stack: brute worlds kBvhStack = 32; BVH worlds the tree depth (9), bvh4_stack + 1 (14), or
    //     the light grid walk's 21 (f32) / 42 (f64) words
    //   launch_lds, the dynamic LDS the launch passes:
    //     world 0: 0 (nothing staged)
    //     world 1: (spheres + lights) * s4
    //     worlds 2, 3, 4: traversal_lds = 4 * (stack * 256 + steal [+ 16 with a light BVH / grid]).  (Before the
    //       launcher became a table these plans carried world 1's value, which the launcher ignored: it passed
    //       this one.)
    //       stack 9:  f32 4 * (2304 + 576) = 11520           f64 4 * (2304 + 1344) = 14592
    //       stack 14: f32 4 * (3584 + 576) = 16640           f64 4 * (3584 + 1344) = 19712
    //       stack 1:  f32 4 * (256 + 576) = 3328             f64 4 * (256 + 1344) = 6400
    //       light grid: f32 4 * (21 * 256 + 576 + 16) = 23872, f64 4 * (42 * 256 + 1344 + 16) = 48448
    //   world 5 (LDS):     waves * (stack * 256 + steal [+ 16 with a light BVH / grid]) [+ 32 + 2 * spheres * 32, wide]
    //                      + nodes * 64 + spheres * 16 + pad8(spheres) * 4 [+ 32, f64] + lights * s4
    //                      + (f32: pad2(lights) * 16; f64: lights * 16)
    //     simple f32: 4 * (9 * 256 + 576) + 156 * 64 + 484 * 16 + 488 * 4 + 19 * 16 + 20 * 16 = 31824
    //     simple f64: 16 * (9 * 256 + 1344) + 32 + 2 * 484 * 32 + 9984 + 7744 + 1952 + 32 + 19 * 32 + 19 * 16 = 110000
    //     64 lights, light BVH, f32: 4 * (2304 + 576 + 16) + 9984 + 7744 + 1952 + 1024 + 1024 = 33312
    //     64 lights, light BVH, f64: 4 * (2304 + 1344 + 16) + 9984 + 7744 + 1952 + 32 + 2048 + 1024 = 37440
    //     64 lights, light grid: 45600 > 36 KiB (f32), 71232 > 52 KiB (f64): the tree stays in L1 / L2
    //     64 spheres f32: 4 * (5 * 256 + 576) + 21 * 64 + 1024 + 256 + 304 + 320 = 10672
    //     64 spheres f64: 16 * (1280 + 1344) + 32 + 4096 + 1344 + 1024 + 256 + 32 + 608 + 304 = 49680
    //     textured (2 spheres, 1 node, 1 light; not wide): f32 3328 + 64 + 32 + 32 + 16 + 32 = 3504
    //                                                      f64 6400 + 64 + 32 + 32 + 32 + 32 + 16 = 6608
    struct Case {
        const rtw_scene* scene;
        const rtw_camera* cam;
        rtw::RenderKnobs k;
        Expect f32, f64;
    };
    const int BR = RTW_ACCEL_BRUTE, BV = RTW_ACCEL_BVH;
    auto tex_k = [&](int kind) {
        rtw::RenderKnobs k = knob("bvh_kind", (uint32_t)kind);
        k.accel = BV;
        return k;
    };
    const rtw_scene s63 = cut(simple, 63), s64 = cut(simple, 64);
    const Case cases[] = {
        {&simple, &cam, knob("", 0), {"defaults", BV, 2, 5, 16, 1, 9, 31824}, {"defaults", BV, 2, 5, 0, 1, 9, 110000}},
        {&simple, &cam, knob("lds", 0), {"lds 0", BV, 2, 5, 16, 1, 9, 31824}, {"lds 0", BV, 2, 5, 0, 1, 9, 110000}},
        {&s63, &cam, knob("lds", 0), {"63 spheres lds 0", BR, 0, 0, 16, 1, 32, 0}, {"63 spheres lds 0", BR, 0, 0, 0, 1, 32, 0}},
        {&simple, &cam, knob("bvh_kind", 0), {"bvh_kind 0", BV, 2, 2, 16, 1, 9, 11520}, {"bvh_kind 0", BV, 2, 2, 0, 1, 9, 14592}},
        {&simple, &cam, knob("bvh_kind", 1), {"bvh_kind 1", BV, 2, 3, 16, 1, 9, 11520}, {"bvh_kind 1", BV, 2, 3, 0, 1, 9, 14592}},
        {&simple, &cam, knob("bvh_kind", 2), {"bvh_kind 2", BV, 4, 4, 16, 1, 14, 16640}, {"bvh_kind 2", BV, 4, 4, 0, 1, 14, 19712}},
        {&simple, &cam, knob("bvh_lds_max", 1), {"bvh_lds_max 1", BV, 2, 3, 16, 1, 9, 11520}, {"bvh_lds_max 1", BV, 2, 3, 0, 1, 9, 14592}},
        {&lights64, &cam, knob("light_grid", 8), {"64 lights grid 8", BV, 2, 3, 18, 1, 21, 23872}, {"64 lights grid 8", BV, 2, 3, 2, 1, 42, 48448}},
        {&lights64, &cam, knob("light_grid", 0), {"64 lights grid 0", BV, 2, 5, 18, 1, 9, 33312}, {"64 lights grid 0", BV, 2, 5, 2, 1, 9, 37440}},
        // forced brute force: no light BVH / grid, world 1 with (484 + 64) * s4
        {&lights64, &cam, knob("accel", (uint32_t)BR), {"64 lights brute", BR, 0, 1, 16, 1, 32, 8768}, {"64 lights brute", BR, 0, 1, 0, 1, 32, 17536}},
        // textured: kinds 0 and 2 have no textured kernel and take the while-while world
        {&tex, &tex_cam, tex_k(0), {"textured kind 0", BV, 2, 3, 13, 1, 1, 3328}, {"textured kind 0", BV, 2, 3, 12, 1, 1, 6400}},
        {&tex, &tex_cam, tex_k(1), {"textured kind 1", BV, 2, 3, 13, 1, 1, 3328}, {"textured kind 1", BV, 2, 3, 12, 1, 1, 6400}},
        {&tex, &tex_cam, tex_k(2), {"textured kind 2", BV, 2, 3, 13, 1, 1, 3328}, {"textured kind 2", BV, 2, 3, 12, 1, 1, 6400}},
        {&tex, &tex_cam, tex_k(3), {"textured kind 3", BV, 2, 5, 13, 1, 1, 3504}, {"textured kind 3", BV, 2, 5, 12, 1, 1, 6608}},
        {&s63, &cam, knob("", 0), {"63 spheres", BR, 0, 1, 16, 1, 32, 1312}, {"63 spheres", BR, 0, 1, 0, 1, 32, 2624}},
        {&s64, &cam, knob("", 0), {"64 spheres", BV, 2, 5, 16, 1, 5, 10672}, {"64 spheres", BV, 2, 5, 0, 1, 5, 49680}},
        // the f32 option bits of a sphere + plane scene
        {&simple, &cam, knob("hit64", 0), {"hit64 0", BV, 2, 5, 0, 1, 9, 31824}, {"hit64 0", BV, 2, 5, 0, 1, 9, 110000}},
        {&simple, &cam, knob("hit64", 1), {"hit64 1", BV, 2, 5, 16, 1, 9, 31824}, {"hit64 1", BV, 2, 5, 0, 1, 9, 110000}},
        {&simple, &cam, knob("robust", 0), {"robust 0", BV, 2, 5, 16, 1, 9, 31824}, {"robust 0", BV, 2, 5, 0, 1, 9, 110000}},
        {&simple, &cam, knob("robust", 1), {"robust 1", BV, 2, 5, 17, 1, 9, 31824}, {"robust 1", BV, 2, 5, 0, 1, 9, 110000}},
        // quads and a cuboid (1 sphere, 1 sphere light: brute force in LDS, 2 * s4), and a DiffuseLight
        // alone (2 spheres, 1 light: 3 * s4): the kernels with the quad / cuboid code, no f64 hit points
        {&box, &box_cam, knob("", 0), {"cornell_box", BR, 0, 1, 8, 1, 32, 32}, {"cornell_box", BR, 0, 1, 8, 1, 32, 64}},
        {&glow, &glow_cam, knob("", 0), {"emissive sphere", BR, 0, 1, 8, 1, 32, 48}, {"emissive sphere", BR, 0, 1, 8, 1, 32, 96}},
    };
    for (const Case& c : cases) {
        check_plan<float>(*c.scene, *c.cam, c.k, c.f32);
        check_plan<double>(*c.scene, *c.cam, c.k, c.f64);
    }
    // the light pdf's path of the 64-light cases: the grid (2), the light BVH (1)
    CHECK(plan_of<float>(lights64, cam, knob("light_grid", 8)).light_bvh == 2 &&
              plan_of<double>(lights64, cam, knob("light_grid", 0)).light_bvh == 1, "64 lights: light_bvh");

    // a BVH deeper than the kernels' traversal stack
    {
        const rtw::RenderKnobs k;
        Staged<float> a = stage<float>(simple, k);
        Staged<double> b = stage<double>(simple, k);
        a.ds.bvh_depth = b.ds.bvh_depth = rtw::kBvhStack + 1;
        const rtw::RenderPlan pa = rtw::plan_render<float>(k, a.ds, cam, 4, 1, a.scale);
        const rtw::RenderPlan pb = rtw::plan_render<double>(k, b.ds, cam, 4, 1, b.scale);
        for (const rtw::RenderPlan* p : {&pa, &pb})
            CHECK(p->err == RTW_E_UNSUPPORTED && !strcmp(p->err_text, "BVH deeper than the kernel's traversal stack"),
                  "deep BVH: error %d '%s'", p->err, p->err_text);
    }
    // every plan names a kernel that exists
    {
        int n_plans = 0;
        const std::tuple<const char*, const rtw_scene*, const rtw_camera*> scenes[] = {
            {"simple", &simple, &cam},       {"63 spheres", &s63, &cam},     {"64 lights", &lights64, &cam},
            {"textured", &tex, &tex_cam},    {"cornell_box", &box, &box_cam}, {"emissive sphere", &glow, &glow_cam}};
        for (const auto& sc : scenes) {
            sweep_plans<float>(std::get<0>(sc), *std::get<1>(sc), *std::get<2>(sc), &n_plans);
            sweep_plans<double>(std::get<0>(sc), *std::get<1>(sc), *std::get<2>(sc), &n_plans);
        }
        printf("sweep: %d plans\n", n_plans);
        CHECK(n_plans == 6 * 2 * 2 * 3 * 4 * 2 * 3 * 2 * 2, "sweep: %d plans without an error", n_plans);
    }
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
