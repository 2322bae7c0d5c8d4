// render_plan.cpp -- see render_plan.hpp
#include "render_plan.hpp"

#include <math.h>

#include <algorithm>
#include <cmath>

namespace rtw {

// Work decomposition: ITEM = (pixel, chunk of `chunk` samples) -- the unit
// a lane folds in sample order; TASK = (8x8 tile, group of chunks) -- one
// wavefront's dynamic item pool.  Small chunks balance the lanes of a
// wave; enough tasks keep the dispatcher fed to the end of the launch.
template <typename R>
uint32_t plan_chunk(const RenderKnobs& k, uint32_t spp, uint32_t n_local_tiles, size_t dev_total) {
    uint32_t chunk = k.chunk ? k.chunk : k.auto_chunk;
    const size_t per_chunk = (size_t)n_local_tiles * 64 * 3 * sizeof(R);
    if (!k.chunk && spp) {
        // keep the chunk sums within partial_max and half the device's memory
        // (deterministic: the chunk, and so the fold order, never depends on
        // what else holds memory): bytes = ceil(spp/chunk) * tiles * 64 * 3 * sizeof(R)
        size_t pmax = k.partial_max;
        if (dev_total) pmax = std::min(pmax, dev_total / 2);
        const size_t max_chunks = std::max<size_t>(1, pmax / std::max<size_t>(per_chunk, 1));
        while ((spp + chunk - 1) / chunk > max_chunks) ++chunk;
    }
    return std::max<uint32_t>(1, std::min<uint32_t>(chunk, std::max<uint32_t>(spp, 1)));
}

template <typename R>
WindowPlan plan_windows(const RenderKnobs& k, uint32_t spp, uint32_t n_local_tiles, size_t dev_total) {
    WindowPlan w;
    const size_t per_chunk = (size_t)n_local_tiles * 64 * 3 * sizeof(R);
    auto one_shot = [&]() {
        w.chunk = plan_chunk<R>(k, spp, n_local_tiles, dev_total);
        w.window = spp;
        w.n_windows = spp ? 1 : 0;
        w.partial_bytes = (size_t)(((uint64_t)spp + w.chunk - 1) / w.chunk) * per_chunk;
        return w;
    };
    if (k.window == 0 || spp == 0) return one_shot();
    uint64_t window = 0;
    if (k.window > 0) {
        window = (uint64_t)k.window;
    } else {
        // auto: the most chunks of the configured size that fit the budget plan_chunk keeps
        const uint32_t chunk = std::max<uint32_t>(1, k.chunk ? k.chunk : k.auto_chunk);
        size_t pmax = k.partial_max;
        if (dev_total) pmax = std::min(pmax, dev_total / 2);
        const size_t max_chunks = std::max<size_t>(1, pmax / std::max<size_t>(per_chunk, 1));
        window = (uint64_t)std::min<size_t>(max_chunks, 0xFFFFFFFFu / chunk) * chunk;
    }
    if (window >= spp) return one_shot();
    // the chunk of a window this long (auto: grows only when one window exceeds the budget)
    // (an explicit chunk stays as it is: the window is rounded up to a multiple of it)
    w.chunk = k.chunk ? k.chunk : plan_chunk<R>(k, (uint32_t)window, n_local_tiles, dev_total);
    window = (window + w.chunk - 1) / w.chunk * w.chunk;
    if (window >= spp) return one_shot();
    w.window = (uint32_t)window;
    w.n_windows = (uint32_t)(((uint64_t)spp + w.window - 1) / w.window);
    w.partial_bytes = (size_t)(w.window / w.chunk) * per_chunk;
    return w;
}

// the scene needs the kernels' quad / cuboid code (kOptPrims): quads, cuboids,
// a mixed light list or a DiffuseLight (whose emission the kernels without it,
// the Book-1 family, do not accumulate)
template <typename R>
static bool scene_has_prims(const DevScene<R>& sc) {
    return sc.n_quads || sc.n_boxes || sc.lref || sc.emissive;
}

// The world decision (render_plan.hpp plan_world): the accelerator, the world
// query and its traversal stack, the f32 test form, the light path and the
// kernel options, with the render kernel's dynamic LDS.
template <typename R>
void plan_world(const RenderKnobs& k, const DevScene<R>& sc, const double center[3], const SceneScale& scale,
                RenderPlan& p) {
    const size_t lds = (size_t)(sc.n_sph + sc.n_lights) * sizeof(R4<R>);
    p.accel = k.accel == RTW_ACCEL_AUTO ? k.auto_accel : k.accel;
    if (p.accel == RTW_ACCEL_AUTO) p.accel = sc.n_sph >= 64 ? RTW_ACCEL_BVH : RTW_ACCEL_BRUTE;
    p.world = (k.world_pref == 0 || lds > kLdsLimit) ? kWorldGlobal : kWorldLds;
    p.stack = kBvhStack;
    p.bvh_width = 0;
    p.launch_lds = lds;
    // f32 sphere/light tests: the reference's hb^2 - a c loses r^2 to
    // rounding once (distance / radius)^2 * 2^-24 is no longer small (C3/C5
    // seen from afar); the closest-approach form is then used.
    {
        const double cx = (double)(R)center[0], cy = (double)(R)center[1], cz = (double)(R)center[2];
        const double far = std::max(scale.extent, sqrt(cx * cx + cy * cy + cz * cz));
        const double rel = std::isfinite(scale.min_radius) ? (far / scale.min_radius) * (far / scale.min_radius) * 5.96e-8
                                                           : 0.0;
        p.robust = k.robust == 2 ? (rel > 1e-3 ? 1u : 0u) : (uint32_t)k.robust;
    }
    // the light pdf goes through the light BVH (same per-lane stack) for
    // longer light lists: with a BVH world only
    const uint32_t light_stack = sc.lbvh_depth + 1;
    p.light_bvh = 0;
    if (p.accel == RTW_ACCEL_BVH && sc.n_lights >= k.light_bvh_min && sc.n_lquads == 0) {
        if (sc.lg_on) p.light_bvh = 2;                          // light grid
        else if (light_stack <= kBvhStack) p.light_bvh = 1;  // light BVH
    }
    // f64 hit points: the f32 kernels of sphere + plane scenes
    p.hit64 = k.hit64 ? 1u : 0u;
    // The kernel's options (rtw_kernels.h kOpt*): textured kernels carry the
    // quad / cuboid code; the closest-approach tests and the f64 hit points are
    // f32's, the latter of the kernels without that code.
    const bool f32 = sizeof(R) == 4;
    p.opts = (sc.mat_tex ? dev::kOptTex | dev::kOptPrims : (scene_has_prims(sc) ? dev::kOptPrims : 0)) |
             (f32 && p.robust ? dev::kOptRobust : 0) | (p.light_bvh ? dev::kOptLightBvh : 0);
    if (f32 && p.hit64 && !(p.opts & dev::kOptPrims)) p.opts |= dev::kOptHit64;
    if (p.accel == RTW_ACCEL_BVH) {
        // the light grid's cooperative walk parks path state in the stack area
        // (f64: one kCoop64Slot-word slot per piece of the walk -- [count, list
        // indices] -- after the kCoopStash64-word stash: 64 pieces per round)
        const uint32_t min_stack = p.light_bvh == 1 ? light_stack
                                   : (p.light_bvh == 2 ? (sizeof(R) == 8 ? kCoopStash64 + kCoop64Slot
                                                                         : kCoopStash + 1u)
                                                       : 1u);
        // binary traversal pushes at most one entry per inner level: a leaf at
        // level `bvh_depth` has that many inner nodes above it (host/bvh.cpp)
        const uint32_t bin_stack = std::max(sc.bvh_depth, min_stack);
        // kWorldBvhLds layout: stacks + stealing area (+ light-work counters) (traversal_lds) | f32 nodes
        // (bvh32) | leaf spheres | ids (padded to 8) | lights | (f32) light pairs | (f64) the lights rounded to f32
        // wide workgroups (rtw_kernels.h kernel_wide): the f64 kernel of sphere + plane
        // scenes with a linear light list -- 16 waves share one copy, which then also
        // holds the f64 spheres twice, in leaf and in id order (32 B each, 32-B aligned)
        const bool wide = dev::kernel_wide(sizeof(R), kWorldBvhLds, p.opts);
        const uint32_t waves = block_waves(wide);
        const size_t tree_lds = traversal_lds<R>(bin_stack, p.light_bvh != 0, waves) +
                                (wide ? 32 + 2 * (size_t)sc.n_sph * sizeof(R4<double>) : 0) +
                                (size_t)sc.n_nodes * sizeof(BvhNode<float>) +
                                (size_t)sc.n_sph * sizeof(R4<float>) +
                                (size_t)((sc.n_sph + 7u) & ~7u) * sizeof(uint32_t) +
                                (sizeof(R) == 8 ? 32 : 0) +   // (f64: the light list 32-B aligned)
                                (size_t)sc.n_lights * sizeof(R4<R>) +
                                // f32: the light pairs of the packed light test; f64: the
                                // lights rounded to f32 for the pre-pass (16 B each)
                                (sizeof(R) == 4 ? (size_t)((sc.n_lights + 1u) & ~1u) * sizeof(R4<R>)
                                                : (size_t)sc.n_lights * sizeof(R4<float>));
        if (k.bvh_kind == 2 && sc.bvh4_stack + 1 <= kBvhStack) {
            p.world = kWorldBvh4;       // 4-wide, when its stack bound fits
            p.stack = std::max(sc.bvh4_stack + 1, min_stack);
            p.bvh_width = 4;
        } else if (sc.bvh_depth <= kBvhStack && min_stack <= kWalkStashMax) {
            // the tree bounds the traversal stack; the light grid's walk may ask
            // for a larger per-lane area (its LDS stash + piece slots)
            p.stack = bin_stack;
            p.bvh_width = 2;
            // (4-wave workgroups: four copies per CU; wide: one workgroup per CU, which may
            // take all of its 160 KiB -- the C2 scene needs 110, ~900 spheres fit)
            const size_t lds_max = k.bvh_lds_max ? k.bvh_lds_max
                                                 : (sizeof(R) == 4 ? 36 * 1024 : (wide ? kLdsLimit : 52 * 1024));
            if (k.bvh_kind == 3 && tree_lds <= lds_max) {
                p.world = kWorldBvhLds;
                p.launch_lds = tree_lds;
            } else {
                p.world = k.bvh_kind ? kWorldBvhWW : kWorldBvh;
            }
        } else {
            p.err = RTW_E_UNSUPPORTED;
            p.err_text = "BVH deeper than the kernel's traversal stack";
            return;
        }
    }
    // textured scenes have kernels for the brute-force and binary while-while worlds only
    if (sc.mat_tex && (p.world == kWorldBvh4 || p.world == kWorldBvh)) {
        p.world = kWorldBvhWW;
        p.bvh_width = 2;
        // Textured kernels carry kOptPrims, so their light-grid walk is the
        // per-lane one (no cooperative walk, no stash or piece slots): only the
        // light BVH's walk uses the per-lane stack
        p.stack = std::max(sc.bvh_depth, p.light_bvh == 1 ? sc.lbvh_depth + 1 : 1u);
        if (p.stack > kBvhStack) {
            p.err = RTW_E_UNSUPPORTED;
            p.err_text = "BVH deeper than the kernel's traversal stack";
            return;
        }
    }
    // The launch's dynamic LDS: the brute-force world in LDS and the tree in LDS
    // as sized above; the other BVH worlds hold their traversal stacks + stealing
    // area; the brute-force world read from global memory holds nothing.
    if (p.world == kWorldGlobal) p.launch_lds = 0;
    else if (p.world != kWorldLds && p.world != kWorldBvhLds) p.launch_lds = traversal_lds<R>(p.stack, p.light_bvh != 0);
    if (!dev::variant_exists(!f32, p.world, p.opts)) {
        p.err = RTW_E_UNSUPPORTED;
        p.err_text = "no render kernel for this scene and tuning";
    }
}

template <typename R>
RenderPlan plan_render(const RenderKnobs& k, const DevScene<R>& sc, const rtw_camera& cam, uint32_t n_local_tiles,
                       uint32_t chunk, const SceneScale& scale) {
    RenderPlan p;
    const uint32_t spp = cam.samples_per_pixel;
    p.chunk = chunk;
    p.n_chunks = spp ? (spp + chunk - 1) / chunk : 0;
    uint32_t group = k.group;
    if (group == 0) {
        // Persistent waves (default) have no per-task drain; a task boundary
        // mixes two tiles' items in the wave (less coherent), the launch's tail
        // grows with the task size.  Longest tiles first leaves cheap tiles
        // for the end, so ~2^17 tasks (~32 per resident wave): C2 split over
        // 1 / 2 / 4 / 8 ranks -> 32 / 28 / 15 / 8 chunks per task (N = 1:
        // group 32 93.7 ms vs 16 94.4, 4 104.4; an 8-way share: 8 13.2 ms vs
        // 4 13.6).  One task per wave instead pays a drain per task: ~2^17.
        constexpr uint32_t kMinAutoGroup = 4, kMaxAutoGroup = 32;
        const uint64_t target = k.target_tasks ? k.target_tasks : kAutoTasks;
        const uint64_t n_groups = n_local_tiles ? (target + n_local_tiles - 1) / n_local_tiles : 1;
        group = (uint32_t)((p.n_chunks + n_groups - 1) / std::max<uint64_t>(n_groups, 1));
        group = std::max(kMinAutoGroup, std::min(group, kMaxAutoGroup));
    }
    // at most 4096 chunks per task: the kernel divides item indices q < 64 * group
    // by the group with a multiply-high by ceil(2^32 / group), exact while 64 group^2 < 2^32
    p.group = std::max<uint32_t>(1, std::min<uint32_t>(std::min<uint32_t>(group, 4096u), std::max<uint32_t>(p.n_chunks, 1)));
    p.n_groups = p.n_chunks ? (p.n_chunks + p.group - 1) / p.group : 0;
    p.n_tasks = n_local_tiles * p.n_groups;
    plan_world<R>(k, sc, cam.center, scale, p);
    if (p.err) return p;
    // auto: walks that cross the whole grid in few pieces give the wave little to
    // share, short ones pay each piece's setup: f32, a fourteenth of the grid's
    // widest side, 4..16 cells (at the default 1/2 cell per light: C3, ~16 cells
    // wide: 4; C5, 158 wide: 11); f64, whose pieces also carry the list-order
    // merge, a seventh, 4..24 (C3 4, C5 22: C5 3249 -> 3133 ms, C3 unchanged;
    // profiles/r04_w_grid_piece_sweep.jsonl)
    const uint32_t grid_w = std::max(sc.lg_n[0], std::max(sc.lg_n[1], sc.lg_n[2]));
    // r05: the f64 walk runs in f32 too, but each piece also keeps and merges
    // candidate list indices: 16..24 cells, the longest a trip may cut (pieces
    // are sized per trip below it: C3 16 vs 11: 554 -> 546 ms at half spp; C5
    // 22; profiles/r05_piece_sweep.jsonl, r05_piece_sweep_final.jsonl)
    p.grid_piece = k.grid_piece != RenderKnobs::kGridPieceAuto
                       ? k.grid_piece
                       : (sizeof(R) == 8 ? std::max(16u, std::min(24u, grid_w / 7u))
                                         : std::max(4u, std::min(16u, grid_w / 14u)));
    // Reordering the tiles scatters the tiles in flight over the image: a tree
    // larger than an XCD's L2 (4 MiB) loses its locality (C5, 1M spheres,
    // ~100 MB: +8 %), so by default only worlds held in LDS or small enough
    // for L2 take it (C2: -4 %, C3 (10k spheres): -4 %).
    const bool on_chip = p.world == kWorldBvhLds || p.world == kWorldLds || scale.tree_bytes <= (4u << 20);
    p.lpt = (k.lpt == 2 || (k.lpt == 1 && on_chip)) && spp >= std::max(k.lpt_min_spp, 1u) && cam.max_depth &&
            n_local_tiles > 1 && p.n_chunks < (1u << 20);
    return p;
}

template uint32_t plan_chunk<float>(const RenderKnobs&, uint32_t, uint32_t, size_t);
template uint32_t plan_chunk<double>(const RenderKnobs&, uint32_t, uint32_t, size_t);
template WindowPlan plan_windows<float>(const RenderKnobs&, uint32_t, uint32_t, size_t);
template WindowPlan plan_windows<double>(const RenderKnobs&, uint32_t, uint32_t, size_t);
template void plan_world<float>(const RenderKnobs&, const DevScene<float>&, const double*, const SceneScale&,
                                RenderPlan&);
template void plan_world<double>(const RenderKnobs&, const DevScene<double>&, const double*, const SceneScale&,
                                 RenderPlan&);
template RenderPlan plan_render<float>(const RenderKnobs&, const DevScene<float>&, const rtw_camera&, uint32_t,
                                       uint32_t, const SceneScale&);
template RenderPlan plan_render<double>(const RenderKnobs&, const DevScene<double>&, const rtw_camera&, uint32_t,
                                        uint32_t, const SceneScale&);

// The task list from the pilot's tile costs: tiles longest first (ties by
// index), each cut into tasks of g chunks.  With the auto task size, g is
// sized per tile so that tasks cost about the same (total cost / target
// tasks, 1..kMaxGroup chunks): a tile whose every sample bounces max_depth
// times (a glass sphere's interior) gets 1-chunk tasks and no task outlasts
// the launch's tail; cheap tiles (sky) get long ones, fewer task switches.
// Only the order and cut of tasks change: every item is still one (pixel,
// chunk) folded in sample order by the reduce, the image is the same bit for
// bit.  Entry: {local tile, first chunk | chunks << 20}.
std::vector<uint32_t> build_task_list(const std::vector<uint32_t>& cost, uint32_t n_chunks, uint32_t fixed_group,
                                      uint64_t target, const RenderKnobs& c, const uint8_t* skip) {
    const uint32_t nt = (uint32_t)cost.size();
    std::vector<uint32_t> order;
    order.reserve(nt);
    for (uint32_t k = 0; k < nt; ++k)
        if (!skip || !skip[k]) order.push_back(k);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
    double total = 0;
    for (uint32_t k : order) total += std::max<uint32_t>(cost[k], 1);
    const double per_task = total * n_chunks / (double)std::max<uint64_t>(target, 1);   // pilot-cost units x chunks
    std::vector<uint32_t> tab;
    if (!fixed_group && c.guide_div) {
        // Guided sizes (guided self-scheduling): each task costs about the work
        // still left after it / guide_div (~ 2 x the resident waves), between
        // total / guide_floor and guide_max chunks.  The launch starts on large
        // tasks (few task switches: a wave's lanes then stay on one tile) and
        // ends on small ones, so the waves run dry together: an 8-rank C2
        // share's equal-cost 2^17 tasks left 3.4 % of its wave-time idle at the
        // end and switched tasks 32 times per wave (profiles/r06a_timeline_*).
        double remaining = total * n_chunks;
        const double floor_cost = total * n_chunks / (double)std::max<uint64_t>(c.guide_floor, 1);
        const uint32_t gmax = std::min<uint32_t>(std::max(c.guide_max, 1u), kTaskMaxChunks);
        for (uint32_t k : order) {
            const double ck = (double)std::max<uint32_t>(cost[k], 1);
            for (uint32_t cb = 0; cb < n_chunks;) {
                const double want = std::max(remaining / (double)c.guide_div, floor_cost) / ck;
                uint32_t g = (uint32_t)std::max(1.0, std::min((double)gmax, std::floor(want + 0.5)));
                g = std::min(g, n_chunks - cb);
                tab.push_back(k);
                tab.push_back(cb | (g << 20));
                cb += g;
                remaining -= g * ck;
            }
        }
    }
    for (uint32_t k : order) {
        if (!fixed_group && c.guide_div) break;
        uint32_t g = fixed_group;
        if (!g) {
            const double want = per_task / (double)std::max<uint32_t>(cost[k], 1);
            g = (uint32_t)std::max(1.0, std::min((double)std::max(c.max_group, 1u), std::floor(want + 0.5)));
        }
        // the entry holds the chunk count in 12 bits (first chunk < 2^20 in the low 20)
        g = std::min(std::min(g, n_chunks), kTaskMaxChunks);
        for (uint32_t cb = 0; cb < n_chunks; cb += g) {
            tab.push_back(k);
            tab.push_back(cb | (std::min(g, n_chunks - cb) << 20));
        }
    }
    return tab;
}

}  // namespace rtw
