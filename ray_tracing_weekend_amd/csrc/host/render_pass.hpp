// render_pass.hpp -- one pass of a render: its kind (the one-shot render, a
// sample window, a sub-pass of an adaptive render), what each kind does, and
// the kernel parameters of a pass (pass_params).  Host only, no HIP call:
// capi_render.cpp render_pass_t allocates, orders the tasks and launches.
#pragma once

#include <algorithm>

#include "camera_params.hpp"
#include "render_plan.hpp"
#include "tiles.hpp"

namespace rtw {

enum PassKind : int { kPassOneShot, kPassWindow, kPassAdaptive };

// What a kind of pass does, in one row each (kPassKinds[kind]).
struct PassKindRow {
    bool fixed_chunk;   // Pass::chunk, or an error: the passes of a render share one fold
                        // association (false: plan_chunk's, which may grow on the device)
    bool split;         // the rank's tiles follow a dealt split (false: the pass's own tiles)
    bool lpt;           // the longest-first task order applies and is kept up
    FoldKind fold;      // what follows the render kernel
    bool zero_fill;     // no sample to trace (no samples, or depth 0: every sample is 0):
                        // d_out is zeroed and nothing is launched (false: the launch
                        // without tasks -- its fold alone)
    bool cull;          // provably empty tiles get no task (host/tile_cull.hpp): the pass's
                        // own fold answers them (adaptive: the caller folds, so never)
};
constexpr PassKindRow kPassKinds[] = {
    /* kPassOneShot  */ {false, true, true, kFoldReduce, true, true},
    /* kPassWindow   */ {true, true, true, kFoldWindow, false, true},
    /* kPassAdaptive */ {true, false, false, kFoldNone, false, false},
};

// The samples [first, first + n) of every pixel of the pass's tiles.
struct Pass {
    PassKind kind = kPassOneShot;
    uint32_t first = 0, n = 0;
    uint32_t chunk = 0;       // window, adaptive: the samples per item (fixed for the render)
    bool begin = true;        // the first pass of a render: counters and stats start here
    uint32_t key_spp = 0;     // the sample count in the task-order key's camera: the render's, not
                              // the pass's, so that the windows of a render share their key
    double* accum = nullptr;  // window: the running sums the fold adds to (device memory)
    // adaptive: the n_tiles global tiles rendered (device memory, ascending; null: every
    // tile of the image), in tile order -- the caller folds the chunk sums, by list position
    const uint32_t* tile_list = nullptr;
    uint32_t n_tiles = 0;
};

// every sample of the camera
inline Pass one_shot_pass(const rtw_camera& cam) {
    Pass ps;
    ps.n = ps.key_spp = cam.samples_per_pixel;
    return ps;
}
// the window [first, first + n) at `chunk` samples per item, folded onto accum
inline Pass window_pass(uint32_t first, uint32_t n, uint32_t chunk, double* accum, bool begin, uint32_t key_spp) {
    Pass ps;
    ps.kind = kPassWindow;
    ps.first = first;
    ps.n = n;
    ps.chunk = chunk;
    ps.begin = begin;
    ps.key_spp = key_spp;
    ps.accum = accum;
    return ps;
}
// the samples [first, first + n) of the n_tiles tiles of tile_list, one per item
inline Pass adaptive_pass(uint32_t first, uint32_t n, const uint32_t* tile_list, uint32_t n_tiles) {
    Pass ps;
    ps.kind = kPassAdaptive;
    ps.first = first;
    ps.n = n;
    ps.chunk = 1;
    ps.begin = first == 0;
    ps.tile_list = tile_list;
    ps.n_tiles = n_tiles;
    return ps;
}

// the camera of the pass's task-order key
inline rtw_camera key_camera(const rtw_camera& cam, const Pass& pass) {
    rtw_camera k = cam;
    k.samples_per_pixel = pass.key_spp;
    return k;
}

// the tiles the pass renders on `rank`
inline uint32_t pass_tiles(const Pass& pass, uint32_t W, uint32_t H, uint32_t rank, uint32_t nranks) {
    return pass.kind == kPassAdaptive ? pass.n_tiles : tiles_for_rank(W, H, rank, nranks);
}

// The kernel parameters of a pass planned as `pl`: the scene, the camera (its
// sample count: the pass's), the plan's decomposition and variant facts, the
// pass's place in the render (s_base, c_base) and an adaptive pass's tile list.
// The buffers (partial, counters, a dealt split's tile_map) and the task order
// (task_table, tile_cost, ...) are the caller's: null / 0 here.
template <typename R>
KParams<R> pass_params(const DevScene<R>& sc, const rtw_camera& cam, uint64_t seed, uint32_t rank, uint32_t nranks,
                       const RenderKnobs& k, const RenderPlan& pl, const Pass& pass) {
    KParams<R> p{};
    p.sc = sc;
    p.sc.robust = pl.robust;
    fill_camera<R>(p, cam);
    p.seed = seed;
    p.W = cam.image_width;
    p.H = cam.image_height;
    p.spp = pass.n;
    p.max_depth = cam.max_depth;
    p.rank = rank;
    p.nranks = nranks;
    p.tiles_x = tiles_across(p.W);
    p.n_local_tiles = pass_tiles(pass, p.W, p.H, rank, nranks);
    p.tile_map = pass.tile_list;
    p.chunk = pl.chunk;
    p.n_chunks = pl.n_chunks;
    p.group = pl.group;
    p.n_groups = pl.n_groups;
    p.n_tasks = pl.n_tasks;
    p.s_base = pass.first;
    p.c_base = pass.first / std::max(pl.chunk, 1u);
    p.item_order = k.item_order;
    p.persist = k.persist;
    p.stack = pl.stack;
    p.light_bvh = pl.light_bvh;
    p.hit64 = pl.hit64;
    p.grid_piece = pl.grid_piece;
    return p;
}

}  // namespace rtw
