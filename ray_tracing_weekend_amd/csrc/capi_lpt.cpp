// capi_lpt.cpp -- longest tiles first, the device work: where a render's tile
// costs come from is host/lpt_state.hpp's decision (lpt_source); here are the
// pilot render, the inline counting, the read-back, the upload of the task
// list (host/render_plan.hpp build_task_list), and rtw_tile_costs.
#include <stdio.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>

#include "capi_ctx.hpp"

namespace {

// The tile costs counted by the last counting render (st.pending) -> st.h_cost
// (waits for that render: once per key)
int lpt_readback(rtw_ctx* c, uint32_t nt) {
    LptCache& l = c->lpt;
    auto copy = [&]() -> int {
        HIP_TRY(c, hipEventSynchronize(l.ev));
        l.st.h_cost.resize(nt);
        // on the context's own (idle, non-blocking) stream: waits for nothing but the copy
        if (nt) {
            HIP_TRY(c, hipMemcpyAsync(l.st.h_cost.data(), l.d_cost, (size_t)nt * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        return RTW_OK;
    };
    const int rc = copy();
    l.st.read_back(rc == RTW_OK);
    return rc;
}

// A 2-sample-per-pixel pilot render of the rank's tiles counts each tile's
// segments (st.h_cost).  Blocking (reads the counts back).
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
    const size_t tile_bytes = rtw::packed_bytes(nt, sizeof(R));
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
    HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, rtw::kCounters * sizeof(unsigned long long), stream));
    if (rtw::launch_render(q, pl.world, pl.opts, pl.launch_lds, rtw::Fold<R>{rtw::kFoldReduce, d_pout, nullptr, 0},
                           stream, nullptr) < 0)
        return fail(c, RTW_E_DEVICE, std::string("pilot launch failed: ") + hipGetErrorString(hipGetLastError()));
    l.st.h_cost.resize(nt);
    HIP_TRY(c, hipMemcpyAsync(l.st.h_cost.data(), d_cost, (size_t)nt * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(c, hipStreamSynchronize(stream));
    return RTW_OK;
}

}  // namespace

template <typename R>
int lpt_prepare(rtw_ctx* c, rtw::KParams<R>& p, const rtw::RenderPlan& pl, const LptKey& key, bool split_has_costs,
                hipStream_t stream, const uint8_t* skip, uint32_t cull_id) {
    const rtw::RenderKnobs& k = c->knobs;
    LptCache& l = c->lpt;
    const uint32_t nt = p.n_local_tiles;
    const bool dbg = getenv("RTW_DEBUG_LPT") != nullptr;   // cold-render cost breakdown (stderr)
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t0 = now();
    auto lap = [&](const char* what, size_t n, const char* unit) {
        if (dbg) fprintf(stderr, "lpt %s %.3f ms (%zu %s)\n", what,
                         std::chrono::duration<double, std::milli>(now() - t0).count(), n, unit);
        t0 = now();
    };
    int rc = RTW_OK;
    switch (rtw::lpt_source(l.st, key, split_has_costs, k.lpt_inline != 0)) {
    case rtw::kSplitCosts:
        // a split dealt by tile costs: those costs order this rank's tasks
        l.st.h_cost.resize(nt);
        for (uint32_t t = 0; t < nt; ++t)
            l.st.h_cost[t] = skip && skip[t] ? 0u : c->split.cost[c->split.h_tile_map[t]];
        l.st.adopt(key);
        break;
    case rtw::kCountInline:
        // the key is kept and the counts marked pending only once lpt.ev is recorded
        // after the launch (lpt_counted), so a failed launch leaves no pending state behind
        l.st.invalidate();
        // a counting render of an earlier key may still run on another stream:
        // the counters are reused only after it
        if (l.ev) HIP_TRY(c, hipStreamWaitEvent(stream, l.ev, 0));
        rc = ensure(c, &l.d_cost, &l.cost_cap, align_up((size_t)nt, 64) * sizeof(uint32_t));
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(l.d_cost, 0, (size_t)nt * sizeof(uint32_t), stream));
        p.tile_cost = reinterpret_cast<uint32_t*>(l.d_cost);
        p.cost_spp = std::min(p.spp, std::max(k.lpt_pilot_spp, 1u));
        p.cost_time = k.cost_time;
        break;
    case rtw::kPilot:
        l.st.invalidate();
        rc = lpt_pilot(c, p, pl, stream);
        lap("pilot", nt, "tiles");
        if (rc) return rc;
        // (the pilot traces every tile; a provably empty one costs nothing in the render)
        for (uint32_t t = 0; skip && t < nt; ++t)
            if (skip[t]) l.st.h_cost[t] = 0;
        l.st.adopt(key);
        HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, rtw::kCounters * sizeof(unsigned long long), stream));
        break;
    case rtw::kReadBack:
        rc = lpt_readback(c, nt);
        if (rc) return rc;
        lap("counts read back", nt, "tiles");
        break;
    case rtw::kCached:
        break;
    }
    if (!l.st.valid) return RTW_OK;   // (this render counts: the plain tile order)
    const uint64_t target = k.target_tasks ? k.target_tasks : rtw::kAutoTasks;
    if (l.st.table_stale(p.n_chunks, k.group, target, cull_id)) {
        l.st.tab_valid = false;
        l.st.h_tasks = rtw::build_task_list(l.st.h_cost, p.n_chunks, k.group ? p.group : 0u, target, k, skip);
        rc = ensure(c, &l.d_tasks, &l.tasks_cap, std::max<size_t>(l.st.h_tasks.size(), 2) * sizeof(uint32_t));
        if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(l.d_tasks, l.st.h_tasks.data(), l.st.h_tasks.size() * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, stream));
        HIP_TRY(c, hipStreamSynchronize(stream));
        lap("tasks", l.st.h_tasks.size() / 2, "tasks");
        l.st.table_built(p.n_chunks, k.group, target, cull_id);
    }
    p.task_table = reinterpret_cast<const uint32_t*>(l.d_tasks);
    p.n_tasks = (uint32_t)(l.st.h_tasks.size() / 2);
    return RTW_OK;
}
template int lpt_prepare<float>(rtw_ctx*, rtw::KParams<float>&, const rtw::RenderPlan&, const LptKey&, bool, hipStream_t,
                                const uint8_t*, uint32_t);
template int lpt_prepare<double>(rtw_ctx*, rtw::KParams<double>&, const rtw::RenderPlan&, const LptKey&, bool, hipStream_t,
                                 const uint8_t*, uint32_t);

// the counts are complete after lpt.ev, read back by the next render of the same key
int lpt_counted(rtw_ctx* c, const LptKey& key, hipStream_t stream) {
    LptCache& l = c->lpt;
    if (!l.ev) HIP_TRY(c, hipEventCreateWithFlags(&l.ev, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(l.ev, stream));
    l.st.counted(key);
    return RTW_OK;
}

int tile_costs_of(rtw_ctx* c, const rtw_camera* cam, uint32_t rank, uint32_t nranks, uint32_t* cost) {
    const rtw::LptState& st = c->lpt.st;
    if (!st.has(lpt_key(c, cam, rank, nranks)))
        return fail(c, RTW_E_INVALID, "no tile costs for this camera, scene and rank split: render once with "
                                      "tuning lpt on and spp >= lpt_min_spp first");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<uint32_t> tiles;
    c->split.local_tiles(cam->image_width, cam->image_height, rank, nranks, tiles);
    if (st.pending) {
        const int rc = lpt_readback(c, (uint32_t)tiles.size());
        if (rc) return rc;
    }
    if (st.h_cost.size() != tiles.size()) return fail(c, RTW_E_INVALID, "tile cost count mismatch");
    // A provably empty tile was never traced and counted nothing: it is reported with the
    // smallest cost, 1 -- the fold answers it -- so that 0 keeps meaning "not counted"
    const LptKey key = lpt_key(c, cam, rank, nranks);
    const rtw::CullState& cs = c->cull.st;
    const bool culled = cs.has(key) && cs.flags.size() == tiles.size();
    for (size_t k = 0; k < tiles.size(); ++k)
        cost[tiles[k]] = culled && cs.flags[k] && !st.h_cost[k] ? 1u : st.h_cost[k];
    return RTW_OK;
}

extern "C" int rtw_tile_costs(rtw_ctx* c, const rtw_camera* cam, uint32_t rank, uint32_t nranks, uint32_t* tile_cost) {
    if (!c || !cam || !tile_cost || nranks == 0 || rank >= nranks) return fail(c, RTW_E_INVALID, "bad argument");
    return tile_costs_of(c, cam, rank, nranks, tile_cost);
}
