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
// pins first.
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
    int world;
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
    printf("plan %-16s %s: accel %d width %u world %d chunk %u stack %u lds %zu light_bvh %u\n", e.name, pr, p.accel,
           p.bvh_width, p.world, p.chunk, p.stack, p.launch_lds, p.light_bvh);
    CHECK(p.err == RTW_OK, "%s %s: error %d %s", e.name, pr, p.err, p.err_text);
    CHECK(p.accel == e.accel && p.bvh_width == e.bvh_width && p.world == e.world && p.chunk == e.chunk,
          "%s %s: accel %d width %u world %d chunk %u, expected %d %u %d %u", e.name, pr, p.accel, p.bvh_width,
          p.world, p.chunk, e.accel, e.bvh_width, e.world, e.chunk);
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
    else if (s != "") abort();
    return k;
}

// the first n spheres of a scene
static rtw_scene cut(rtw_scene s, uint32_t n) {
    s.n_spheres = n;
    return s;
}

int main() {
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
        CHECK(e.ds.n_sph == 2 && e.ds.n_lights == 1 && e.ds.bvh_depth == 1 && e.ds.bvh4_stack == 0 &&
                  e.ds.mat_tex != nullptr, "checkered_spheres stages differently");
        CHECK(f.ds.n_nodes == 21 && f.ds.bvh_depth == 5 && g.ds.n_nodes == 21 && g.ds.bvh_depth == 5,
              "the 64-sphere scene stages differently");
    }

    // {name, accel, bvh_width, world, chunk | stack, launch_lds}; the hand evaluation, per precision R
    // (s4 = sizeof(R4<R>): 16 / 32; steal = 576 / 1344 B per wave; 4 waves per workgroup, f64 `wide` 16):
    //   brute worlds:      stack kBvhStack = 32, lds = (spheres + lights) * s4
    //   worlds 2, 3, 4:    lds as the brute worlds; stack = tree depth (9), bvh4_stack + 1 (14), or
    //                      the light grid walk's 21 (f32) / 42 (f64) words
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
    struct Case {
        const rtw_scene* scene;
        const rtw_camera* cam;
        rtw::RenderKnobs k;
        Expect f32, f64;
    };
    rtw::RenderKnobs tex_k = knob("bvh_kind", 2);
    tex_k.accel = RTW_ACCEL_BVH;
    const rtw_scene s63 = cut(simple, 63), s64 = cut(simple, 64);
    const int BR = RTW_ACCEL_BRUTE, BV = RTW_ACCEL_BVH;
    const Case cases[] = {
        {&simple, &cam, knob("", 0), {"defaults", BV, 2, 5, 1, 9, 31824}, {"defaults", BV, 2, 5, 1, 9, 110000}},
        {&simple, &cam, knob("lds", 0), {"lds 0", BV, 2, 5, 1, 9, 31824}, {"lds 0", BV, 2, 5, 1, 9, 110000}},
        {&s63, &cam, knob("lds", 0), {"63 spheres lds 0", BR, 0, 0, 1, 32, 1312}, {"63 spheres lds 0", BR, 0, 0, 1, 32, 2624}},
        {&simple, &cam, knob("bvh_kind", 0), {"bvh_kind 0", BV, 2, 2, 1, 9, 8048}, {"bvh_kind 0", BV, 2, 2, 1, 9, 16096}},
        {&simple, &cam, knob("bvh_kind", 1), {"bvh_kind 1", BV, 2, 3, 1, 9, 8048}, {"bvh_kind 1", BV, 2, 3, 1, 9, 16096}},
        {&simple, &cam, knob("bvh_kind", 2), {"bvh_kind 2", BV, 4, 4, 1, 14, 8048}, {"bvh_kind 2", BV, 4, 4, 1, 14, 16096}},
        {&simple, &cam, knob("bvh_lds_max", 1), {"bvh_lds_max 1", BV, 2, 3, 1, 9, 8048}, {"bvh_lds_max 1", BV, 2, 3, 1, 9, 16096}},
        {&lights64, &cam, knob("light_grid", 8), {"64 lights grid 8", BV, 2, 3, 1, 21, 8768}, {"64 lights grid 8", BV, 2, 3, 1, 42, 17536}},
        {&lights64, &cam, knob("light_grid", 0), {"64 lights grid 0", BV, 2, 5, 1, 9, 33312}, {"64 lights grid 0", BV, 2, 5, 1, 9, 37440}},
        {&tex, &tex_cam, tex_k, {"textured kind 2", BV, 2, 3, 1, 1, 48}, {"textured kind 2", BV, 2, 3, 1, 1, 96}},
        {&s63, &cam, knob("", 0), {"63 spheres", BR, 0, 1, 1, 32, 1312}, {"63 spheres", BR, 0, 1, 1, 32, 2624}},
        {&s64, &cam, knob("", 0), {"64 spheres", BV, 2, 5, 1, 5, 10672}, {"64 spheres", BV, 2, 5, 1, 5, 49680}},
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
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
