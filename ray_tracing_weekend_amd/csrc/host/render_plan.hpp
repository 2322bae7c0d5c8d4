// render_plan.hpp -- what a render launches: the tuning knobs, and the pure
// decisions that turn them, the staged scene's counts and the camera into the
// work decomposition and the kernel variant -- render_kernel<R, world, opts>
// and its dynamic LDS, decided here and nowhere else (plan_chunk /
// plan_render; render_launch.hpp only looks the variant up) -- and the
// longest-tiles-first task list (build_task_list).  Host only, no HIP call:
// the C-ABI allocates, launches and keeps the caches.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../../include/rtw.h"
#include "../rtw_kernels.h"
#include "stage_scene.hpp"

namespace rtw {

constexpr size_t kLdsLimit = 160 * 1024;
constexpr uint64_t kAutoTasks = 1u << 17;   // auto task size: about this many tasks per render
constexpr uint32_t kTaskMaxChunks = 4095;    // task-table entry {first chunk | chunks << 20}: 12 bits

// rtw_set_accel, rtw_set_chunk and the keys of rtw_set_tuning
struct RenderKnobs {
    int accel = RTW_ACCEL_AUTO;
    uint32_t chunk = 0;           // samples per item (0 = auto_chunk)
    uint32_t auto_chunk = 1;      // one sample per item: the chunk fold is then the reference's
                                  // sample-by-sample fold exactly
    // cap of the chunk-sum buffer (the auto chunk grows beyond it), at most half
    // the device's memory: 128 GiB of the 288 GB of HBM keeps every BASELINE
    // config at one sample per item -- the reference's fold order exactly (C2
    // f64: 11.5 GB, C3 f64 51 GB, a C4 f64 8-way share 102 GB).  Chunk 1 is
    // also the faster form: a chunk > 1 reads its running sum back at every
    // sample's end (C3 f64 1083 vs 1121 ms at chunk 2, a C4 share 958 vs 993
    // ms at chunk 4, profiles/r06h_ab_chunk.jsonl, r06i_ab_c4_chunk.jsonl)
    size_t partial_max = (size_t)128 << 30;
    uint32_t group = 0;           // chunks per wave task (0 = from target_tasks)
    uint64_t target_tasks = 0;   // auto chunks-per-task: about this many tasks (0: 2^19 with
                                 // persistent waves, 2^17 without), 4..32 chunks per task
    int world_pref = 1;           // 1: LDS-staged sphere list when it fits, 0: global
    int auto_accel = RTW_ACCEL_AUTO;    // RTW_ACCEL_AUTO resolves to this (AUTO: by scene size)
    int bvh_kind = 3;             // BVH traversal: 3 = binary while-while + leaf postponing on the
                                  // tree staged in LDS (falls back to 1 when it does not fit),
                                  // 1 = the same from L1/L2, 2 = 4-wide octant tree, 0 = binary
                                  // single loop
    // LDS per workgroup allowed for bvh_kind 3 (0: by precision -- f32 36 KiB, four
    // 256-thread workgroups per CU at 4 waves/SIMD; f64 52 KiB)
    size_t bvh_lds_max = 0;
    int robust = 2;                   // f32 closest-approach tests: 1 on, 0 off, 2 by scene scale
    uint32_t bvh_leaf = 0;            // spheres per BVH leaf (set before rtw_set_scene); 0 = auto:
                                      // 4, 8 for scenes of >= 100k spheres (C5: +12 %), 2 for
                                      // f64 scenes of 4096..100k (auto_leaf)
    uint32_t persist = kPersistResident;   // workgroups of persistent waves (tasks from a
                                      // counter; default: as many as are resident at once);
                                      // 0: one task per wave
    uint32_t query_grid = 0;          // queries, feature pass, wavefront rounds: at most this many
                                      // workgroups a launch (query_plan.hpp query_grid); 0: as many
                                      // as are resident at once
    uint32_t light_leaf = 0;          // light spheres per light-BVH leaf; 0 = 4
    uint32_t light_grid = 8;          // light pdf through the light grid at light_grid / 16
                                      // cells per light (set before rtw_set_scene); 0: light BVH
    uint32_t hit64 = 1;               // f32: f64 hit points (the reference's self-intersection odds)
    uint32_t item_order = 1;          // wave item pool: 1 sample-major (C2 +1.3 %, C3 +5 %, C5 +2 %), 0 pixel-major
    uint32_t lpt = 1;                 // longest tiles first: task order from a pilot render's
                                      // per-tile segment counts (cached per scene / camera / split);
                                      // 1: for worlds in LDS or within an L2, 2: always, 0: never
    uint32_t lpt_min_spp = 32;        // ... for renders of at least this many samples per pixel
    uint32_t lpt_inline = 1;          // 1: no separate pilot -- the first render of a (scene,
                                      // camera, split) runs in the plain tile order and counts the
                                      // segments of each pixel's first lpt_pilot_spp samples; the
                                      // renders after it take the task list of those counts
                                      // 0: a pilot render before the first render
    uint32_t lpt_pilot_spp = 2;       // the pilot render: samples per pixel
    uint32_t lpt_pilot_depth = 0;     // ... and its max depth (0: the camera's); a path's segments
                                      // run one after another, so the pilot lasts as long as its
                                      // longest path
    static constexpr uint32_t kGridPieceAuto = 0xFFFFFFFFu;
    uint32_t grid_piece = kGridPieceAuto;   // light grid walks: cells per piece of the wave's
                                      // cooperative walk (0: one lane walks its own ray)
    uint32_t light_bvh_min = 64;      // light lists at least this long use the light BVH
                                      // (C2, 19 lights: the linear masked loop is faster)
    static constexpr uint32_t kMaxGroup = 32;
    uint32_t max_group = kMaxGroup;   // longest-first task list: at most this many chunks per task
    // longest-first task list with guided sizes (build_task_list; guide_div 0: equal-cost
    // tasks of max_group chunks at most): a task costs the remaining work / guide_div,
    // at least total / guide_floor, at most guide_max chunks
    // (C2 f64, max of 8 rank shares, 3 runs each: 16.32 ms vs equal-cost tasks 16.79;
    // one GPU 117.35 vs 118.46 ms; profiles/r06i_ab_split.jsonl)
    uint32_t guide_div = 16384, guide_max = 128;
    uint32_t cost_time = 1;           // tile costs in wave-time shares (KParams::cost_time); 0: work counts
    uint64_t guide_floor = 1u << 20;
    uint32_t balance = 1;             // multi-device renders: deal tiles by their counted costs
    uint32_t tile_cull = 1;           // f64 sphere + plane renders: tiles whose camera beam provably
                                      // misses the scene get no task, the fold answers them
                                      // (host/tile_cull.hpp); 0: off
    static constexpr int64_t kWindowAuto = -1;
    int64_t window = 0;               // sample windows (plan_windows): 0 off; N > 0: renders of more
                                      // than N samples per pixel run N at a time onto an f64
                                      // accumulator; kWindowAuto: the largest window whose chunk
                                      // sums fit partial_max
    uint32_t denoise_lds = 1;         // rtw_denoise's iterations (host/denoise_plan.hpp): 0 all direct,
                                      // 1 the plan's choice, 2 staged in LDS wherever the halo fits
};

// What plan_render decides.  err != RTW_OK: no render (err_text says why);
// chunk / n_chunks are valid even then.
struct RenderPlan {
    uint32_t chunk = 1, n_chunks = 0;   // samples per item, items per pixel
    uint32_t group = 1, n_groups = 0;   // chunks per wave task, tasks per tile
    uint32_t n_tasks = 0;               // in the plain tile order (a task list has its own count)
    int accel = RTW_ACCEL_BRUTE;        // RTW_ACCEL_AUTO resolved
    int world = kWorldLds;              // WorldMode: the kernel's kWorld
    int opts = 0;                       // the kernel's kOpt (rtw_kernels.h kOpt* bits; a variant that exists)
    uint32_t bvh_width = 0;
    uint32_t stack = kBvhStack;         // KParams::stack
    size_t launch_lds = 0;              // dynamic LDS the kernel is launched with
    uint32_t light_bvh = 0;             // KParams::light_bvh
    uint32_t grid_piece = 0;            // KParams::grid_piece
    uint32_t hit64 = 0;                 // KParams::hit64
    uint32_t robust = 0;                // DevScene::robust
    bool lpt = false;                   // the longest-tiles-first task order applies
    int err = RTW_OK;
    const char* err_text = "";
};

// Step 1: the samples per item.  An auto chunk (knobs.chunk 0) grows until the
// chunk sums of n_local_tiles tiles fit partial_max and half of dev_total (the
// device's memory, 0: unknown).
template <typename R>
uint32_t plan_chunk(const RenderKnobs& k, uint32_t spp, uint32_t n_local_tiles, size_t dev_total);

// Step 1 with sample windows (knobs.window): a render of spp samples runs as
// n_windows windows of `window` samples (a multiple of the chunk; the last may
// be short), each folded onto an f64 accumulator, so the chunk sums hold one
// window: partial_bytes = ceil(window / chunk) * n_local_tiles * 64 * 3 *
// sizeof(R).  knobs.window 0: one window of spp samples at plan_chunk's chunk
// (the one-shot render).  In window mode the auto chunk is sized against the
// window, never against spp: with kWindowAuto it stays auto_chunk at any spp.
struct WindowPlan {
    uint32_t chunk = 1, window = 0, n_windows = 0;
    size_t partial_bytes = 0;
};
template <typename R>
WindowPlan plan_windows(const RenderKnobs& k, uint32_t spp, uint32_t n_local_tiles, size_t dev_total);

// The world decision of step 2, shared with the ray queries (query_plan.hpp):
// fills p.accel, world, opts, bvh_width, stack, launch_lds, light_bvh, hit64,
// robust (by the scene's scale as seen from `center`) and err / err_text.
template <typename R>
void plan_world(const RenderKnobs& k, const DevScene<R>& sc, const double center[3], const SceneScale& scale,
                RenderPlan& p);

// Step 2: everything else, for the chunk that was actually allocated.
template <typename R>
RenderPlan plan_render(const RenderKnobs& k, const DevScene<R>& sc, const rtw_camera& cam, uint32_t n_local_tiles,
                       uint32_t chunk, const SceneScale& scale);

// The longest-tiles-first task list of tiles with these costs:
// {local tile, first chunk | chunks << 20} pairs.  fixed_group 0: sized by cost.
// skip (may be null): [local tile] 1 = the tile gets no task (provably empty,
// host/tile_cull.hpp) and weighs nothing, whatever its cost; a cost of 0 alone
// is a cheap tile like any other.
std::vector<uint32_t> build_task_list(const std::vector<uint32_t>& cost, uint32_t n_chunks, uint32_t fixed_group,
                                      uint64_t target, const RenderKnobs& k, const uint8_t* skip = nullptr);

}  // namespace rtw
