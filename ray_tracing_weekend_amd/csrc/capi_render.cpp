// capi_render.cpp -- the render entry points of the C-ABI (include/rtw.h): a
// render is plan (host/render_plan.hpp) -> buffers -> longest-tiles-first task
// list -> launch -> bookkeeping; the tile assembly and the blocking rtw_render.
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <type_traits>

#include "capi_ctx.hpp"
#include "host/render_adaptive.hpp"

namespace {

// The device copy of a buffer the kernels read (the split's maps): rewritten
// only when the split changes, after the device is idle -- a render still
// queued on another stream may read the old contents.
int upload_map(rtw_ctx* c, void** buf, size_t* cap, const std::vector<uint32_t>& h) {
    HIP_TRY(c, hipDeviceSynchronize());
    int rc = ensure(c, buf, cap, std::max<size_t>(h.size(), 1) * sizeof(uint32_t));
    if (rc) return rc;
    if (!h.empty()) HIP_TRY(c, hipMemcpy(*buf, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return RTW_OK;
}

// this rank's local tile -> global tile map of the active split on the device
int ensure_tile_map(rtw_ctx* c, uint32_t W, uint32_t H, uint32_t rank, uint32_t nranks) {
    SplitState& s = c->split;
    if (s.d_tile_map && s.tile_map_key == s.serial && s.tile_map_rank == rank) return RTW_OK;
    s.local_tiles(W, H, rank, nranks, s.h_tile_map);
    const int rc = upload_map(c, &s.d_tile_map, &s.tile_map_cap, s.h_tile_map);
    if (rc) return rc;
    s.tile_map_key = s.serial;
    s.tile_map_rank = rank;
    return RTW_OK;
}

// the assembly's map of the active split (host/tiles.hpp tile_slots)
int ensure_tile_slot(rtw_ctx* c, uint32_t nranks) {
    SplitState& s = c->split;
    if (s.d_tile_slot && s.tile_slot_key == s.serial) return RTW_OK;
    const int rc = upload_map(c, &s.d_tile_slot, &s.tile_slot_cap, rtw::tile_slots(s.rank, nranks));
    if (rc) return rc;
    s.tile_slot_key = s.serial;
    return RTW_OK;
}

template <typename R>
void fill_camera(rtw::KParams<R>& p, const rtw_camera* cam) {
    for (int k = 0; k < 3; ++k) {
        p.center[k] = (R)cam->center[k];
        p.p00[k] = (R)cam->pixel00_loc[k];
        p.du[k] = (R)cam->pixel_delta_u[k];
        p.dv[k] = (R)cam->pixel_delta_v[k];
        p.disk_u[k] = (R)cam->defocus_disk_u[k];
        p.disk_v[k] = (R)cam->defocus_disk_v[k];
        p.bg[k] = (R)cam->background[k];
    }
    // Uniform::new_inclusive(-0.5, 0.5) scale (rand 0.8.6)
    double max_rand = 1.0 - 2.220446049250313080847e-16;
    double scale = (0.5 - -0.5) / max_rand;
    while (scale * max_rand + -0.5 > 0.5) scale = nextafter(scale, 0.0);
    p.u_scale = (R)scale;
    p.defocus = cam->defocus_angle > 2.220446049250313080847e-16 ? 1u : 0u;
    p.W = cam->image_width;
    p.H = cam->image_height;
    p.spp = cam->samples_per_pixel;
    p.max_depth = cam->max_depth;
}

// the plan's kernel variant, then the chunk reduction into out; a sample window
// (accum non-null): the fold onto accum instead (out may be null)
template <typename R>
int launch_render(const rtw::KParams<R>& p, const rtw::RenderPlan& pl, R* out, hipStream_t stream, hipEvent_t mid,
                  double* accum = nullptr, uint32_t first = 0) {
    if constexpr (std::is_same<R, float>::value)
        return rtw::launch_render_f32(p, pl.world, pl.opts, pl.launch_lds, out, stream, mid, accum, first);
    else return rtw::launch_render_f64(p, pl.world, pl.opts, pl.launch_lds, out, stream, mid, accum, first);
}

// the device's memory, asked once (plan_chunk / plan_windows budget)
size_t device_total(rtw_ctx* c) {
    if (!c->dev_total) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) c->dev_total = tot;
    }
    return c->dev_total;
}

// One pass of a render: every sample of the camera (the one-shot render), or
// the window [first, first + n) folded onto `accum`.
struct Pass {
    uint32_t first = 0, n = 0;
    uint32_t chunk = 0;               // window passes: the samples per item (fixed for the render)
    double* accum = nullptr;          // non-null: a window pass
    bool begin = true;                // the first pass of a render: counters and stats start here
    const rtw_camera* key_cam = nullptr;   // the camera of the task-order key: the same for every
                                           // window of a render
    // A pass of an adaptive render (rtw_render_adaptive): the render kernel alone, in tile
    // order, on the n_tiles global tiles of tile_list (device memory, ascending; null: every
    // tile of the image) -- the caller folds the chunk sums (c->d_partial, by list position),
    // and the longest-first cache and the rank split are neither read nor written
    bool adaptive = false;
    const uint32_t* tile_list = nullptr;
    uint32_t n_tiles = 0;
};

// The tile costs counted by the last counting render (lpt.pending) -> lpt.h_cost
// (waits for that render: once per key)
int lpt_readback(rtw_ctx* c, uint32_t nt) {
    LptCache& l = c->lpt;
    l.pending = false;   // (an error below recounts at the next render)
    HIP_TRY(c, hipEventSynchronize(l.ev));
    l.h_cost.resize(nt);
    // on the context's own (idle, non-blocking) stream: waits for nothing but the copy
    if (nt) {
        HIP_TRY(c, hipMemcpyAsync(l.h_cost.data(), l.d_cost, (size_t)nt * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                  c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    l.valid = true;
    return RTW_OK;
}

// Longest tiles first: a 2-sample-per-pixel pilot render of the rank's tiles
// counts each tile's segments (lpt.h_cost); build_task_list turns them into the
// task list.  Blocking (reads the counts back); cached by the caller.
template <typename R>
int lpt_pilot(rtw_ctx* c, const rtw::KParams<R>& p, const rtw::RenderPlan& pl, hipStream_t stream) {
    const rtw::RenderKnobs& k = c->knobs;
    LptCache& l = c->lpt;
    const uint32_t nt = p.n_local_tiles;
    rtw::KParams<R> q = p;
    q.spp = std::min(p.spp, std::max(k.lpt_pilot_spp, 1u));
    if (k.lpt_pilot_depth) q.max_depth = std::min(p.max_depth, k.lpt_pilot_depth);
    q.chunk = 1;
    q.n_chunks = q.spp;
    q.group = q.n_chunks;
    q.n_groups = 1;
    q.n_tasks = nt;
    q.seed = p.seed ^ 0x5851F42D4C957F2Dull;
    q.s_base = q.c_base = 0;      // (its own samples: only their costs matter)
    q.task_table = nullptr;
    const size_t words = align_up((size_t)nt, 64);
    const size_t tile_bytes = (size_t)nt * 64 * 3 * sizeof(R);
    const size_t bytes = words * sizeof(uint32_t) + (size_t)q.n_chunks * tile_bytes + tile_bytes;
    int rc = ensure(c, &l.d_cost, &l.cost_cap, bytes);
    if (rc) return rc;
    uint32_t* d_cost = reinterpret_cast<uint32_t*>(l.d_cost);
    R* d_part = reinterpret_cast<R*>(d_cost + words);
    R* d_pout = d_part + (size_t)q.n_chunks * nt * 64 * 3;
    q.partial = d_part;
    q.tile_cost = d_cost;
    q.cost_spp = q.spp;
    q.cost_time = k.cost_time;
    HIP_TRY(c, hipMemsetAsync(d_cost, 0, (size_t)nt * sizeof(uint32_t), stream));
    HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, rtw_ctx::kCounters * sizeof(unsigned long long), stream));
    if (launch_render(q, pl, d_pout, stream, nullptr) < 0)
        return fail(c, RTW_E_DEVICE, std::string("pilot launch failed: ") + hipGetErrorString(hipGetLastError()));
    l.h_cost.resize(nt);
    HIP_TRY(c, hipMemcpyAsync(l.h_cost.data(), d_cost, (size_t)nt * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));
    return RTW_OK;
}

// The task order of this render (the plan says longest tiles first applies):
// tile costs of `key` from a dealt split, from the render before, from a pilot,
// or counted by this very render (p.tile_cost: plain tile order this time);
// with costs, the task list on the device (p.task_table).
template <typename R>
int lpt_prepare(rtw_ctx* c, rtw::KParams<R>& p, const rtw::RenderPlan& pl, const LptKey& key, bool split,
                hipStream_t stream) {
    const rtw::RenderKnobs& k = c->knobs;
    LptCache& l = c->lpt;
    const bool same = l.has(key);
    const bool dbg = getenv("RTW_DEBUG_LPT") != nullptr;   // cold-render cost breakdown (stderr)
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t0 = now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(now() - t0).count(); };
    int rc = RTW_OK;
    if (!same && split && !c->split.cost.empty()) {
        // a split dealt by tile costs: those costs order this rank's tasks (no counting)
        l.pending = false;
        l.tab_valid = false;
        l.h_cost.resize(p.n_local_tiles);
        for (uint32_t t = 0; t < p.n_local_tiles; ++t) l.h_cost[t] = c->split.cost[c->split.h_tile_map[t]];
        l.valid = true;
        l.key = key;
    } else if (!same && k.lpt_inline) {
        // this render counts its tiles' costs on the way (plain tile order);
        // the key is kept and the counts marked pending only once lpt.ev is
        // recorded after the launch (lpt_counted), so a failed launch leaves no
        // pending state behind
        l.valid = l.pending = false;
        l.tab_valid = false;
        const uint32_t nt = p.n_local_tiles;
        // a counting render of an earlier key may still run on another stream:
        // the counters are reused only after it
        if (l.ev) HIP_TRY(c, hipStreamWaitEvent(stream, l.ev, 0));
        rc = ensure(c, &l.d_cost, &l.cost_cap, align_up((size_t)nt, 64) * sizeof(uint32_t));
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(l.d_cost, 0, (size_t)nt * sizeof(uint32_t), stream));
        p.tile_cost = reinterpret_cast<uint32_t*>(l.d_cost);
        p.cost_spp = std::min(p.spp, std::max(k.lpt_pilot_spp, 1u));
        p.cost_time = k.cost_time;
    } else if (!same) {
        l.valid = l.pending = false;
        l.tab_valid = false;
        rc = lpt_pilot(c, p, pl, stream);
        if (dbg) fprintf(stderr, "lpt pilot %.3f ms (%u tiles)\n", ms(), p.n_local_tiles);
        t0 = now();
        if (rc) return rc;
        l.valid = true;
        l.key = key;
        HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, rtw_ctx::kCounters * sizeof(unsigned long long), stream));
    } else if (l.pending) {
        // the counts of the render before (waits for it: once per key)
        rc = lpt_readback(c, p.n_local_tiles);
        if (rc) return rc;
        if (dbg) fprintf(stderr, "lpt counts read back %.3f ms (%u tiles)\n", ms(), p.n_local_tiles);
        t0 = now();
    }
    const uint64_t target = k.target_tasks ? k.target_tasks : rtw::kAutoTasks;
    if (l.valid && (!l.tab_valid || l.tab_chunks != p.n_chunks || l.tab_group != k.group || l.tab_target != target)) {
        l.tab_valid = false;
        l.h_tasks = rtw::build_task_list(l.h_cost, p.n_chunks, k.group ? p.group : 0u, target, k);
        rc = ensure(c, &l.d_tasks, &l.tasks_cap, l.h_tasks.size() * sizeof(uint32_t));
        if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(l.d_tasks, l.h_tasks.data(), l.h_tasks.size() * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, stream));
        HIP_TRY(c, hipStreamSynchronize(stream));
        if (dbg) fprintf(stderr, "lpt tasks %.3f ms (%zu tasks)\n", ms(), l.h_tasks.size() / 2);
        l.tab_valid = true;
        l.tab_chunks = p.n_chunks;
        l.tab_group = k.group;
        l.tab_target = target;
    }
    if (l.valid) {
        p.task_table = reinterpret_cast<const uint32_t*>(l.d_tasks);
        p.n_tasks = (uint32_t)(l.h_tasks.size() / 2);
    }
    return RTW_OK;
}

// after the launch of a counting render: its counts are complete after lpt.ev,
// read back by the next render of the same key
int lpt_counted(rtw_ctx* c, const LptKey& key, hipStream_t stream) {
    LptCache& l = c->lpt;
    if (!l.ev) HIP_TRY(c, hipEventCreateWithFlags(&l.ev, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(l.ev, stream));
    l.key = key;
    l.pending = true;
    return RTW_OK;
}

// The chunk-sum buffer of a render, and the plan for the chunk it holds: when
// the device cannot hold it (other allocations) an auto chunk doubles instead
// of failing -- stats.chunk reports it, the fold is then chunk-associated
// (rounding level)
// (fixed_chunk > 0, a window pass: that chunk or an error -- the windows of a
// render share one fold association)
template <typename R>
int plan_and_allocate(rtw_ctx* c, const rtw::DevScene<R>& sc, const rtw_camera* cam, uint32_t n_local_tiles,
                      rtw::RenderPlan* pl, uint32_t fixed_chunk = 0) {
    const uint32_t spp = cam->samples_per_pixel;
    if (!c->knobs.chunk && spp) (void)device_total(c);
    const size_t per_chunk = (size_t)n_local_tiles * 64 * 3 * sizeof(R);
    uint32_t chunk = fixed_chunk ? fixed_chunk : rtw::plan_chunk<R>(c->knobs, spp, n_local_tiles, c->dev_total);
    for (;;) {
        *pl = rtw::plan_render<R>(c->knobs, sc, *cam, n_local_tiles, chunk, c->scale);
        const size_t bytes = std::max<size_t>((size_t)pl->n_chunks * per_chunk, 64);
        if (c->partial_cap >= bytes) break;
        if (c->d_partial) (void)hipFree(c->d_partial);
        c->d_partial = nullptr;
        c->partial_cap = 0;
        const hipError_t e = hipMalloc(&c->d_partial, bytes);
        if (e == hipSuccess) { c->partial_cap = bytes; break; }
        c->d_partial = nullptr;
        (void)hipGetLastError();
        if (c->knobs.chunk || fixed_chunk || chunk >= spp || e != hipErrorOutOfMemory)
            return hip_fail(c, e, "hipMalloc(chunk sums)");
        chunk = std::min<uint32_t>(chunk * 2, spp);
    }
    return pl->err ? fail(c, pl->err, pl->err_text) : RTW_OK;
}

// (a window pass writes d_out only when it is given: the render's last window)
template <typename R>
int render_pass_t(rtw_ctx* c, const rtw_camera* cam_in, uint64_t seed, uint32_t rank, uint32_t nranks,
                  void* d_out, size_t out_bytes, hipStream_t stream, const Pass& pass) {
    // the plan and the kernel see the pass's samples; their RNG streams start at s_base
    rtw_camera pass_cam = *cam_in;
    pass_cam.samples_per_pixel = pass.n;
    const rtw_camera* cam = &pass_cam;
    rtw::KParams<R> p{};
    p.sc = *reinterpret_cast<const rtw::DevScene<R>*>(
        std::is_same<R, float>::value ? (const void*)&c->sc32 : (const void*)&c->sc64);
    fill_camera(p, cam);
    p.s_base = pass.first;   // (c_base: once the chunk is planned)
    // the kernel holds a lane's pixel as i | j << 16
    if (p.W > 65535 || p.H > 65535) return fail(c, RTW_E_UNSUPPORTED, "image width or height beyond 65535");
    p.seed = seed;
    p.rank = rank;
    p.nranks = nranks;
    p.tiles_x = rtw::tiles_across(p.W);
    p.n_local_tiles = pass.adaptive ? pass.n_tiles : rtw::tiles_for_rank(p.W, p.H, rank, nranks);
    const size_t need_out = (size_t)p.n_local_tiles * 64 * 3 * sizeof(R);
    if (!pass.adaptive && (!pass.accum || d_out)) {
        if (out_bytes < need_out) return fail(c, RTW_E_INVALID, "d_out is smaller than tiles_for_rank*64*3");
        if (need_out && !d_out) return fail(c, RTW_E_INVALID, "d_out is NULL");
    }
    // the split's local -> global tile map (a dealt split; null: the round robin)
    const bool split = !pass.adaptive && c->split.active(p.W, p.H, nranks);
    p.tile_map = pass.adaptive ? pass.tile_list : nullptr;
    if (split && p.n_local_tiles) {
        const int mrc = ensure_tile_map(c, p.W, p.H, rank, nranks);
        if (mrc) return mrc;
        p.tile_map = reinterpret_cast<const uint32_t*>(c->split.d_tile_map);
    }
    rtw::RenderPlan pl;
    int rc = plan_and_allocate<R>(c, p.sc, cam, p.n_local_tiles, &pl, pass.accum || pass.adaptive ? pass.chunk : 0u);
    if (rc) return rc;
    p.chunk = pl.chunk;
    p.c_base = p.s_base / std::max(pl.chunk, 1u);
    p.n_chunks = pl.n_chunks;
    p.group = pl.group;
    p.n_groups = pl.n_groups;
    p.n_tasks = pl.n_tasks;
    p.item_order = c->knobs.item_order;
    p.persist = c->knobs.persist;
    p.partial = reinterpret_cast<R*>(c->d_partial);
    p.counters = c->d_counters;
    p.stack = pl.stack;
    p.sc.robust = pl.robust;
    p.light_bvh = pl.light_bvh;
    p.hit64 = pl.hit64;
    p.grid_piece = pl.grid_piece;
    p.task_table = nullptr;
    p.tile_cost = nullptr;
    p.cost_spp = 0;
    p.cost_time = 0;
    if (pass.begin) {
        HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, rtw_ctx::kCounters * sizeof(unsigned long long), stream));
    } else {
        // a later window of the same render: the counters go on, but the task counter starts over
        HIP_TRY(c, hipMemsetAsync(c->d_counters + 6, 0, sizeof(unsigned long long), stream));
    }
    const LptKey key = lpt_key(c, pass.key_cam ? pass.key_cam : cam_in, rank, nranks);
    if (pl.lpt && !pass.adaptive) {
        rc = lpt_prepare(c, p, pl, key, split, stream);
        if (rc) return rc;
    }
    hipEvent_t* ev = c->ring[c->n_renders % rtw_ctx::kRing];
    if (pass.begin) HIP_TRY(c, hipEventRecord(c->ev0, stream));
    HIP_TRY(c, hipEventRecord(ev[0], stream));
    int lrc = 0;
    if (need_out == 0) {
        HIP_TRY(c, hipEventRecord(ev[1], stream));
    } else if (pass.adaptive) {
        if (p.max_depth == 0) p.n_tasks = 0;   // every sample is 0: the caller folds no chunk sums
        if constexpr (std::is_same<R, float>::value)
            lrc = rtw::launch_render_only_f32(p, pl.world, pl.opts, pl.launch_lds, stream, ev[1]);
        else lrc = rtw::launch_render_only_f64(p, pl.world, pl.opts, pl.launch_lds, stream, ev[1]);
    } else if (pass.accum) {
        if (p.max_depth == 0) p.n_tasks = p.n_chunks = 0;   // every sample is 0: the fold alone
        lrc = launch_render(p, pl, reinterpret_cast<R*>(d_out), stream, ev[1], pass.accum, pass.first);
    } else if (p.spp == 0 || p.max_depth == 0) {
        // depth == 0: every sample is Colour::default() + res = 0 (camera.rs:470-472)
        HIP_TRY(c, hipMemsetAsync(d_out, 0, need_out, stream));
        HIP_TRY(c, hipEventRecord(ev[1], stream));
    } else {
        lrc = launch_render(p, pl, reinterpret_cast<R*>(d_out), stream, ev[1]);
    }
    if (lrc < 0) return fail(c, RTW_E_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    // (the launcher reports the instantiation it launched, not what it was asked for)
    if (lrc && lrc != rtw::variant_code(pl.world, pl.opts))
        return fail(c, RTW_E_DEVICE, "the launched kernel variant is not the render plan's");
    c->last_variant = lrc;
    if (p.tile_cost) {
        rc = lpt_counted(c, key, stream);
        if (rc) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev1, stream));
    HIP_TRY(c, hipEventRecord(ev[2], stream));
    ++c->n_renders;
    std::vector<uint32_t> tiles;
    c->split.local_tiles(p.W, p.H, rank, nranks, tiles);
    const uint64_t before = pass.begin ? 0 : c->last.samples;
    c->last = rtw_stats{};
    c->last.samples = before + rtw::tile_pixels(p.W, p.H, tiles) * p.spp;
    c->last.accel = (uint32_t)pl.accel;
    c->last.bvh_width = pl.bvh_width;
    c->last.kernel = (uint32_t)pl.world;
    c->last_n_sph = p.sc.n_sph;
    c->last_light_bvh = p.light_bvh;
    c->last_n_list = p.sc.n_list;
    c->last.chunk = pl.chunk;
    return RTW_OK;
}

// this context's f64 accumulator of window renders: n_local_tiles * 64 * 3 doubles
int ensure_accum(rtw_ctx* c, uint32_t n_local_tiles) {
    return ensure(c, &c->d_accum, &c->accum_cap, std::max<size_t>((size_t)n_local_tiles * 64 * 3 * sizeof(double), 64));
}

// A render of this rank's tiles: one pass, or (tuning "window") the windows of
// plan_windows one after another on `stream`, folded onto the context's
// accumulator; the last one writes d_out.
template <typename R>
int render_device_t(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t rank, uint32_t nranks,
                    void* d_out, size_t out_bytes, hipStream_t stream) {
    Pass one;
    one.n = cam->samples_per_pixel;
    if (c->knobs.window == 0) return render_pass_t<R>(c, cam, seed, rank, nranks, d_out, out_bytes, stream, one);
    const uint32_t nt = rtw::tiles_for_rank(cam->image_width, cam->image_height, rank, nranks);
    const rtw::WindowPlan w = rtw::plan_windows<R>(c->knobs, cam->samples_per_pixel, nt, device_total(c));
    if (w.n_windows <= 1 || nt == 0) return render_pass_t<R>(c, cam, seed, rank, nranks, d_out, out_bytes, stream, one);
    if (out_bytes < (size_t)nt * 64 * 3 * sizeof(R)) return fail(c, RTW_E_INVALID, "d_out is smaller than tiles_for_rank*64*3");
    if (!d_out) return fail(c, RTW_E_INVALID, "d_out is NULL");
    int rc = ensure_accum(c, nt);
    if (rc) return rc;
    for (uint32_t k = 0; k < w.n_windows; ++k) {
        Pass ps;
        ps.first = k * w.window;
        ps.n = std::min(w.window, cam->samples_per_pixel - ps.first);
        ps.chunk = w.chunk;   // (not clamped to a short last window: s_base stays a multiple of it)
        ps.accum = reinterpret_cast<double*>(c->d_accum);
        ps.begin = k == 0;
        ps.key_cam = cam;
        const bool last = k + 1 == w.n_windows;
        rc = render_pass_t<R>(c, cam, seed, rank, nranks, last ? d_out : nullptr, last ? out_bytes : 0, stream, ps);
        if (rc) return rc;
    }
    return RTW_OK;
}

// The samples per item of a window of n samples (rtw_render_window_device);
// windows continue each other only when they start on an item boundary.
template <typename R>
uint32_t window_chunk(rtw_ctx* c, uint32_t n, uint32_t nt) {
    return c->knobs.chunk ? c->knobs.chunk : rtw::plan_chunk<R>(c->knobs, n, nt, device_total(c));
}

// rtw_render_window_device's arguments (nothing is launched)
template <typename R>
int check_window(rtw_ctx* c, const rtw_camera* cam, uint32_t rank, uint32_t nranks, uint32_t first, uint32_t n,
                 const double* d_accum, size_t accum_bytes) {
    const uint32_t nt = rtw::tiles_for_rank(cam->image_width, cam->image_height, rank, nranks);
    const uint32_t chunk = window_chunk<R>(c, n, nt);
    if (first % chunk)
        return fail(c, RTW_E_INVALID, "first_sample is not a multiple of the chunk (" + std::to_string(chunk) + ")");
    if (accum_bytes < (size_t)nt * 64 * 3 * sizeof(double))
        return fail(c, RTW_E_INVALID, "d_accum is smaller than tiles_for_rank*64*3 doubles");
    if (nt && !d_accum) return fail(c, RTW_E_INVALID, "d_accum is NULL");
    return RTW_OK;
}

// rtw_render_window_device on a one-device context, its arguments checked
template <typename R>
int render_window_t(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t rank, uint32_t nranks,
                    uint32_t first, uint32_t n, double* d_accum, hipStream_t stream) {
    const uint32_t nt = rtw::tiles_for_rank(cam->image_width, cam->image_height, rank, nranks);
    const uint32_t chunk = window_chunk<R>(c, n, nt);
    // the task-order key of a window render: the camera without its sample count
    rtw_camera key_cam = *cam;
    key_cam.samples_per_pixel = 0;
    Pass ps;
    ps.first = first;
    ps.n = n;
    ps.chunk = chunk;
    ps.accum = d_accum;
    ps.key_cam = &key_cam;
    if (nt == 0) ps.accum = nullptr;   // nothing to fold: the bookkeeping of an empty render
    return render_pass_t<R>(c, cam, seed, rank, nranks, nullptr, 0, stream, ps);
}

// The adaptive state of an image of nt tiles, carved from c->d_adapt: doubles
// first (sums nt * 192, s12 nt * 128), then the words.
struct AdaptiveBuffers {
    double *sums, *s12;
    uint32_t *counts, *flags, *list[2], *meta[2];   // meta: {list length, pixels inside the image}
};
int adaptive_buffers(rtw_ctx* c, uint32_t nt, AdaptiveBuffers* b) {
    const size_t doubles = (size_t)nt * 64 * 5, words = (size_t)nt * 4 + 4;
    const int rc = ensure(c, &c->d_adapt, &c->adapt_cap, doubles * sizeof(double) + words * sizeof(uint32_t));
    if (rc) return rc;
    b->sums = reinterpret_cast<double*>(c->d_adapt);
    b->s12 = b->sums + (size_t)nt * 64 * 3;
    b->counts = reinterpret_cast<uint32_t*>(b->sums + doubles);
    b->flags = b->counts + nt;
    b->list[0] = b->flags + nt;
    b->list[1] = b->list[0] + nt;
    b->meta[0] = b->list[1] + nt;
    b->meta[1] = b->meta[0] + 2;
    return RTW_OK;
}

// rtw_render_adaptive_device, its arguments checked: the passes of
// host/render_adaptive.hpp on render_pass_t's machinery.  Per pass: the render
// kernel on the active tiles (sub-passes under the chunk-sum budget), the fold
// with the stop vote, the compaction of the tiles that go on, and one 8-byte
// read-back with a stream synchronisation -- the next pass is planned for that
// many tiles.  The passes run in tile order (no task table): the longest-first
// cache and the split are left as they are.
template <typename R>
int render_adaptive_t(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t min_samples, uint32_t max_samples,
                      uint32_t window, double tolerance, double* d_sums, uint32_t* d_counts, hipStream_t stream) {
    const uint32_t W = cam->image_width, H = cam->image_height;
    const uint32_t nt = (uint32_t)rtw::n_tiles_of(W, H);
    AdaptiveBuffers b{};
    int rc = adaptive_buffers(c, nt, &b);
    if (rc) return rc;
    uint32_t n_active = nt, first = 0;
    uint64_t active_px = (uint64_t)W * H, total = 0;
    const uint32_t* list = nullptr;   // pass 0: every tile
    int cur = 0;
    const uint32_t n_passes = rtw::adaptive_passes(min_samples, max_samples, window);
    for (uint32_t k = 0; k < n_passes && n_active; ++k) {
        const uint32_t end = rtw::adaptive_pass_end(min_samples, max_samples, window, k);
        const bool last = end == max_samples;
        const uint32_t cap = rtw::adaptive_sub_samples<R>(c->knobs, n_active, device_total(c));
        for (uint32_t s = first; s < end;) {
            const uint32_t n = std::min(cap, end - s);
            Pass ps;
            ps.first = s;
            ps.n = n;
            ps.chunk = 1;
            ps.begin = s == 0;
            ps.adaptive = true;
            ps.tile_list = list;
            ps.n_tiles = n_active;
            rc = render_pass_t<R>(c, cam, seed, 0, 1, nullptr, 0, stream, ps);
            if (rc) return rc;
            rtw::AdaptiveFold f{};
            f.partial = c->d_partial;
            f.n_chunks = cam->max_depth ? n : 0;   // depth 0: every sample is 0
            f.list = list;
            f.n_active = n_active;
            f.sums = b.sums;
            f.s12 = b.s12;
            f.first = s;
            f.W = W;
            f.H = H;
            f.n_end = end;
            f.decide = s + n == end;
            f.last = last;
            f.tolerance = tolerance;
            f.counts = b.counts;
            f.flags = b.flags;
            if (rtw::launch_fold_adaptive(sizeof(R) == 8, f, stream))
                return fail(c, RTW_E_DEVICE, std::string("adaptive fold launch failed: ") + hipGetErrorString(hipGetLastError()));
            s += n;
        }
        total += active_px * (end - first);
        first = end;
        if (last) break;
        cur ^= 1;
        if (rtw::launch_compact_tiles(b.flags, nt, W, H, b.list[cur], b.meta[cur], stream))
            return fail(c, RTW_E_DEVICE, std::string("tile compaction launch failed: ") + hipGetErrorString(hipGetLastError()));
        uint32_t h_meta[2] = {0, 0};
        HIP_TRY(c, hipMemcpyAsync(h_meta, b.meta[cur], sizeof h_meta, hipMemcpyDeviceToHost, stream));
        HIP_TRY(c, hipStreamSynchronize(stream));
        if (h_meta[0] > n_active) return fail(c, RTW_E_DEVICE, "adaptive: the active tile list grew");
        n_active = h_meta[0];
        active_px = h_meta[1];
        list = b.list[cur];
    }
    if (rtw::launch_unpack_adaptive(b.sums, b.counts, W, H, d_sums, d_counts, stream))
        return fail(c, RTW_E_DEVICE, std::string("adaptive unpack launch failed: ") + hipGetErrorString(hipGetLastError()));
    HIP_TRY(c, hipEventRecord(c->ev1, stream));   // the stats' time covers the last fold too
    c->last.samples = total;
    c->last.chunk = 1;
    return RTW_OK;
}

}  // namespace

int tile_costs_of(rtw_ctx* c, const rtw_camera* cam, uint32_t rank, uint32_t nranks, uint32_t* cost) {
    if (!c->lpt.has(lpt_key(c, cam, rank, nranks)))
        return fail(c, RTW_E_INVALID, "no tile costs for this camera, scene and rank split: render once with "
                                      "tuning lpt on and spp >= lpt_min_spp first");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<uint32_t> tiles;
    c->split.local_tiles(cam->image_width, cam->image_height, rank, nranks, tiles);
    if (c->lpt.pending) {
        const int rc = lpt_readback(c, (uint32_t)tiles.size());
        if (rc) return rc;
    }
    if (c->lpt.h_cost.size() != tiles.size()) return fail(c, RTW_E_INVALID, "tile cost count mismatch");
    for (size_t k = 0; k < tiles.size(); ++k) cost[tiles[k]] = c->lpt.h_cost[k];
    return RTW_OK;
}

extern "C" {

int rtw_tile_costs(rtw_ctx* c, const rtw_camera* cam, uint32_t rank, uint32_t nranks, uint32_t* tile_cost) {
    if (!c || !cam || !tile_cost || nranks == 0 || rank >= nranks) return fail(c, RTW_E_INVALID, "bad argument");
    return tile_costs_of(c, cam, rank, nranks, tile_cost);
}

int rtw_assemble_tiles(rtw_ctx* c, const void* d_ranks, size_t rank_stride_bytes, uint32_t nranks, uint32_t W,
                       uint32_t H, void* d_image, void* stream) {
    if (!c || nranks == 0) return fail(c, RTW_E_INVALID, "bad argument");
    const size_t esz = c->precision == RTW_F32 ? sizeof(float) : sizeof(double);
    if ((uint64_t)W * H == 0) return RTW_OK;
    if (!d_ranks || !d_image || rank_stride_bytes % esz)
        return fail(c, RTW_E_INVALID, "bad assemble buffers");
    if (rank_stride_bytes < (size_t)rtw::tiles_for_rank(W, H, 0, nranks) * 64 * 3 * esz)
        return fail(c, RTW_E_INVALID, "rank stride is smaller than tiles_for_rank(rank 0)*64*3");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    const size_t stride = rank_stride_bytes / esz;
    // a dealt split: each tile's slot from its map (null: the round robin)
    const uint32_t* slot = nullptr;
    if (c->split.active(W, H, nranks)) {
        const int mrc = ensure_tile_slot(c, nranks);
        if (mrc) return mrc;
        slot = reinterpret_cast<const uint32_t*>(c->split.d_tile_slot);
    }
    const int rc = c->precision == RTW_F32
                       ? rtw::launch_assemble_f32(reinterpret_cast<const float*>(d_ranks), stride, nranks, W, H,
                                                  slot, reinterpret_cast<float*>(d_image), s)
                       : rtw::launch_assemble_f64(reinterpret_cast<const double*>(d_ranks), stride, nranks, W, H,
                                                  slot, reinterpret_cast<double*>(d_image), s);
    if (rc) return fail(c, RTW_E_DEVICE, std::string("assemble launch failed: ") + hipGetErrorString(hipGetLastError()));
    return RTW_OK;
}

int rtw_render_device(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t rank, uint32_t nranks,
                      void* d_out, size_t out_bytes, void* stream) {
    if (!c || !cam || nranks == 0 || rank >= nranks) return fail(c, RTW_E_INVALID, "bad argument");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    // a multi-device context renders on rank 0 only here: its stats are rank 0's
    c->stats_ranks = 1;
    if (c->gather_pending) {
        // the last gather / assembly may still read d_gather (rank 0 renders into it
        // again only through rtw_render_image_device, but d_out may alias it)
        HIP_TRY(c, hipStreamWaitEvent(s, c->gather_ev, 0));
    }
    return c->precision == RTW_F32 ? render_device_t<float>(c, cam, seed, rank, nranks, d_out, out_bytes, s)
                                   : render_device_t<double>(c, cam, seed, rank, nranks, d_out, out_bytes, s);
}

int rtw_render_window_device(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t rank, uint32_t nranks,
                             uint32_t first_sample, uint32_t n_samples, double* d_accum, size_t accum_bytes,
                             void* stream) {
    if (!c || !cam || nranks == 0 || rank >= nranks) return fail(c, RTW_E_INVALID, "bad argument");
    if (c->multi) return fail(c, RTW_E_UNSUPPORTED, "sample windows of a multi-device context: tuning \"window\"");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    if ((uint64_t)first_sample + n_samples > 0xFFFFFFFFull)
        return fail(c, RTW_E_INVALID, "first_sample + n_samples overflows");
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = c->precision == RTW_F32
                       ? check_window<float>(c, cam, rank, nranks, first_sample, n_samples, d_accum, accum_bytes)
                       : check_window<double>(c, cam, rank, nranks, first_sample, n_samples, d_accum, accum_bytes);
    if (rc || n_samples == 0) return rc;
    hipStream_t s = resolve_stream(c, stream);
    c->stats_ranks = 1;
    return c->precision == RTW_F32
               ? render_window_t<float>(c, cam, seed, rank, nranks, first_sample, n_samples, d_accum, s)
               : render_window_t<double>(c, cam, seed, rank, nranks, first_sample, n_samples, d_accum, s);
}

int rtw_render_window(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t first_sample, uint32_t n_samples,
                      double* sums, rtw_stats* stats) {
    if (!c || !cam || !sums) return fail(c, RTW_E_INVALID, "bad argument");
    if (c->multi) return fail(c, RTW_E_UNSUPPORTED, "sample windows of a multi-device context: tuning \"window\"");
    const uint32_t W = cam->image_width, H = cam->image_height;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<uint32_t> tiles;   // the packed order of the one rank's tiles (host/tiles.hpp)
    c->split.local_tiles(W, H, 0, 1, tiles);
    const size_t n = tiles.size() * 64 * 3;
    int rc = ensure_accum(c, (uint32_t)tiles.size());
    if (rc) return rc;
    const uint32_t tiles_x = rtw::tiles_across(W);
    // image [H][W][3] <-> packed tiles [lt][ly * 8 + lx][3]
    auto each_pixel = [&](auto&& f) {
        for (size_t lt = 0; lt < tiles.size(); ++lt) {
            const uint32_t tx = tiles[lt] % tiles_x, ty = tiles[lt] / tiles_x;
            for (uint32_t px = 0; px < 64; ++px) {
                const uint32_t i = tx * rtw::kTile + (px & 7u), j = ty * rtw::kTile + (px >> 3);
                if (i < W && j < H) f(((size_t)j * W + i) * 3, (lt * 64 + px) * 3);
            }
        }
    };
    std::vector<double> packed(n, 0.0);
    if (first_sample && n_samples && n) {
        each_pixel([&](size_t img, size_t pk) {
            for (int k = 0; k < 3; ++k) packed[pk + k] = sums[img + k];
        });
        HIP_TRY(c, hipMemcpyAsync(c->d_accum, packed.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    rc = rtw_render_window_device(c, cam, seed, 0, 1, first_sample, n_samples, reinterpret_cast<double*>(c->d_accum),
                                  c->accum_cap, nullptr);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the upload reads `packed`)
        return rc;
    }
    if (n_samples == 0) return RTW_OK;
    if (n) HIP_TRY(c, hipMemcpyAsync(packed.data(), c->d_accum, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    each_pixel([&](size_t img, size_t pk) {
        for (int k = 0; k < 3; ++k) sums[img + k] = packed[pk + k];
    });
    rtw_stats st{};
    rc = rtw_get_stats(c, &st);
    if (stats) *stats = st;
    return rc;
}

int rtw_render_adaptive_device(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t min_samples,
                               uint32_t max_samples, uint32_t window, double tolerance, double* d_sums,
                               size_t sums_bytes, uint32_t* d_counts, size_t counts_bytes, void* stream) {
    if (!c || !cam) return fail(c, RTW_E_INVALID, "bad argument");
    if (c->multi) return fail(c, RTW_E_UNSUPPORTED, "adaptive sampling of a multi-device context");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    if (const char* why = rtw::adaptive_check(min_samples, max_samples, window, tolerance, c->knobs.chunk))
        return fail(c, RTW_E_INVALID, why);
    const uint32_t W = cam->image_width, H = cam->image_height;
    if (W > 65535 || H > 65535) return fail(c, RTW_E_UNSUPPORTED, "image width or height beyond 65535");
    const size_t px = (size_t)W * H;
    if (px == 0) return RTW_OK;
    if (!d_sums || !d_counts) return fail(c, RTW_E_INVALID, "d_sums or d_counts is NULL");
    if (sums_bytes < px * 3 * sizeof(double) || counts_bytes < px * sizeof(uint32_t))
        return fail(c, RTW_E_INVALID, "d_sums is smaller than H*W*3 doubles or d_counts than H*W");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    c->stats_ranks = 1;
    return c->precision == RTW_F32
               ? render_adaptive_t<float>(c, cam, seed, min_samples, max_samples, window, tolerance, d_sums, d_counts, s)
               : render_adaptive_t<double>(c, cam, seed, min_samples, max_samples, window, tolerance, d_sums, d_counts, s);
}

int rtw_render_adaptive(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t min_samples, uint32_t max_samples,
                        uint32_t window, double tolerance, double* sums, uint32_t* counts, rtw_stats* stats) {
    if (!c || !cam || !sums || !counts) return fail(c, RTW_E_INVALID, "bad argument");
    if (c->multi) return fail(c, RTW_E_UNSUPPORTED, "adaptive sampling of a multi-device context");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    if (const char* why = rtw::adaptive_check(min_samples, max_samples, window, tolerance, c->knobs.chunk))
        return fail(c, RTW_E_INVALID, why);
    if (cam->image_width > 65535 || cam->image_height > 65535)
        return fail(c, RTW_E_UNSUPPORTED, "image width or height beyond 65535");
    const size_t px = (size_t)cam->image_width * cam->image_height;
    if (px == 0) {   // nothing to render: the stats of no samples
        if (stats) {
            *stats = rtw_stats{};
            stats->chunk = 1;
        }
        return RTW_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // the image-order sums, then the counts
    int rc = ensure(c, &c->d_adapt_img, &c->adapt_img_cap, px * (3 * sizeof(double) + sizeof(uint32_t)));
    if (rc) return rc;
    double* d_sums = reinterpret_cast<double*>(c->d_adapt_img);
    uint32_t* d_counts = reinterpret_cast<uint32_t*>(d_sums + px * 3);
    rc = rtw_render_adaptive_device(c, cam, seed, min_samples, max_samples, window, tolerance, d_sums,
                                    px * 3 * sizeof(double), d_counts, px * sizeof(uint32_t), nullptr);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(sums, d_sums, px * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(counts, d_counts, px * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rtw_stats st{};
    rc = rtw_get_stats(c, &st);
    if (stats) *stats = st;
    return rc;
}

int rtw_render(rtw_ctx* c, const rtw_camera* cam, const rtw_scene* scene, uint64_t seed, double* out_sum,
               rtw_stats* stats) {
    if (!c || !cam || !out_sum) return fail(c, RTW_E_INVALID, "bad argument");
    if (scene) {
        int rc = rtw_set_scene(c, scene);
        if (rc) return rc;
    }
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "no scene");
    const size_t esz = c->precision == RTW_F32 ? sizeof(float) : sizeof(double);
    const size_t n = (size_t)cam->image_width * cam->image_height * 3;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure(c, &c->d_img, &c->img_cap, std::max<size_t>(n * esz, 64));
    if (rc) return rc;
    // every device of the context renders its share; the image lands on the first
    rc = rtw_render_image_device(c, cam, seed, c->d_img, c->img_cap, nullptr);
    if (rc) return rc;
    c->h_out.resize(n * esz);
    if (n) HIP_TRY(c, hipMemcpyAsync(c->h_out.data(), c->d_img, n * esz, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->precision == RTW_F32) {
        const float* f = reinterpret_cast<const float*>(c->h_out.data());
        for (size_t k = 0; k < n; ++k) out_sum[k] = (double)f[k];
    } else {
        memcpy(out_sum, c->h_out.data(), n * sizeof(double));
    }
    rtw_stats st{};
    rc = rtw_get_stats(c, &st);
    if (stats) *stats = st;
    return rc;
}

}  // extern "C"
