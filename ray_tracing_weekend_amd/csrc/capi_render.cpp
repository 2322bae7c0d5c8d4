// capi_render.cpp -- the render entry points of the C-ABI (include/rtw.h): a
// render is one pass or several (host/render_pass.hpp); a pass is plan
// (host/render_plan.hpp) -> params -> buffers -> task order (capi_lpt.cpp) ->
// launch -> bookkeeping.  The one-shot and window entries, the tile assembly
// and the blocking rtw_render / rtw_render_window / rtw_render_window_image.
#include <algorithm>

#include "capi_ctx.hpp"

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

// The flags of the provably empty tiles of `key` (host/tile_cull.hpp), on the
// host and the device: classified once per key, dropped with it.  The device
// copies are rewritten only after the device is idle (upload_map's reason).
int cull_prepare(rtw_ctx* c, const LptKey& key, uint32_t rank, uint32_t nranks) {
    CullCache& k = c->cull;
    if (k.st.has(key)) return RTW_OK;
    std::vector<uint32_t> tiles;
    c->split.local_tiles(key.cam.image_width, key.cam.image_height, rank, nranks, tiles);
    rtw::cull_classify(k.st, key, *c->cull_scene, tiles);
    if (!k.st.n_culled) return RTW_OK;
    auto upload = [&]() -> int {
        HIP_TRY(c, hipDeviceSynchronize());
        const int rc = ensure(c, &k.d_flags, &k.flags_cap, align_up(k.st.flags.size(), 64));
        if (rc) return rc;
        HIP_TRY(c, hipMemcpy(k.d_flags, k.st.flags.data(), k.st.flags.size(), hipMemcpyHostToDevice));
        return RTW_OK;
    };
    const int rc = upload();
    if (rc) k.st.drop();
    return rc;
}

// A render of a key with provably empty tiles and no longest-first task list
// (its first render, or a render too short for one): the plain tile order
// without those tiles, as a task table.
template <typename R>
int cull_plain_tasks(rtw_ctx* c, rtw::KParams<R>& p) {
    CullCache& k = c->cull;
    if (!k.st.tab_valid || k.st.tab_chunks != p.n_chunks || k.st.tab_group != p.group) {
        k.st.tab_valid = false;
        k.st.h_tasks = rtw::plain_task_list(k.st.flags, p.n_chunks, p.group);
        HIP_TRY(c, hipDeviceSynchronize());
        const int rc = ensure(c, &k.d_tasks, &k.tasks_cap, std::max<size_t>(k.st.h_tasks.size(), 2) * sizeof(uint32_t));
        if (rc) return rc;
        if (!k.st.h_tasks.empty())
            HIP_TRY(c, hipMemcpy(k.d_tasks, k.st.h_tasks.data(), k.st.h_tasks.size() * sizeof(uint32_t),
                                 hipMemcpyHostToDevice));
        k.st.tab_chunks = p.n_chunks;
        k.st.tab_group = p.group;
        k.st.tab_valid = true;
    }
    p.task_table = reinterpret_cast<const uint32_t*>(k.d_tasks);
    p.n_tasks = (uint32_t)(k.st.h_tasks.size() / 2);
    return RTW_OK;
}

// The chunk-sum buffer of a render, and the plan for the chunk it holds: when
// the device cannot hold it (other allocations) an auto chunk doubles instead
// of failing -- stats.chunk reports it, the fold is then chunk-associated
// (rounding level)
// (fixed_chunk > 0: that chunk or an error, host/render_pass.hpp PassKindRow)
template <typename R>
int plan_and_allocate(rtw_ctx* c, const rtw::DevScene<R>& sc, const rtw_camera* cam, uint32_t n_local_tiles,
                      rtw::RenderPlan* pl, uint32_t fixed_chunk) {
    const uint32_t spp = cam->samples_per_pixel;
    if (!c->knobs.chunk && spp) (void)device_total(c);
    const size_t per_chunk = rtw::packed_bytes(n_local_tiles, sizeof(R));
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

template <typename R>
int render_pass_t(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t rank, uint32_t nranks, void* d_out,
                  hipStream_t stream, const rtw::Pass& pass) {
    const rtw::PassKindRow& kind = rtw::kPassKinds[pass.kind];
    const uint32_t W = cam->image_width, H = cam->image_height;
    const uint32_t nt = rtw::pass_tiles(pass, W, H, rank, nranks);
    // params: the plan sees the pass's samples (the chunk sums are allocated with it)
    rtw_camera pass_cam = *cam;
    pass_cam.samples_per_pixel = pass.n;
    rtw::RenderPlan pl;
    int rc = plan_and_allocate<R>(c, dev_scene<R>(c), &pass_cam, nt, &pl, kind.fixed_chunk ? pass.chunk : 0u);
    if (rc) return rc;
    rtw::KParams<R> p = rtw::pass_params<R>(dev_scene<R>(c), *cam, seed, rank, nranks, c->knobs, pl, pass);
    // buffers: the chunk sums, the counters, a dealt split's local -> global tile map
    p.partial = reinterpret_cast<R*>(c->d_partial);
    p.counters = c->d_counters;
    const bool split = kind.split && c->split.active(W, H, nranks);
    if (split && nt) {
        rc = ensure_tile_map(c, W, H, rank, nranks);
        if (rc) return rc;
        p.tile_map = reinterpret_cast<const uint32_t*>(c->split.d_tile_map);
    }
    // (a later pass of the same render: the counters go on, but the task counter starts over)
    HIP_TRY(c, pass.begin ? hipMemsetAsync(c->d_counters, 0, rtw::kCounters * sizeof(unsigned long long), stream)
                          : hipMemsetAsync(c->d_counters + rtw::kCounterNextTask, 0, sizeof(unsigned long long), stream));
    const rtw_camera key_cam = rtw::key_camera(*cam, pass);
    const LptKey key = lpt_key(c, &key_cam, rank, nranks);
    const bool dark = p.spp == 0 || p.max_depth == 0;   // every sample is Colour::default() + res = 0 (camera.rs:470-472)
    // provably empty tiles (f64 sphere + plane kernels): no task, the fold answers them
    const rtw::CullState* cull = nullptr;
    if (kind.cull && sizeof(R) == 8 && c->knobs.tile_cull && c->cull_scene && nt && !dark && !pl.err &&
        !(pl.opts & (rtw::dev::kOptPrims | rtw::dev::kOptTex)) && p.n_chunks < (1u << 20)) {
        rc = cull_prepare(c, key, rank, nranks);
        if (rc) return rc;
        if (c->cull.st.n_culled) cull = &c->cull.st;
    }
    // task order
    if (pl.lpt && kind.lpt) {
        rc = lpt_prepare(c, p, pl, key, split && !c->split.cost.empty(), stream, cull ? cull->flags.data() : nullptr,
                         cull ? cull->serial : 0u);
        if (rc) return rc;
    }
    if (cull && !p.task_table) {
        rc = cull_plain_tasks(c, p);
        if (rc) return rc;
    }
    // launch
    hipEvent_t* ev = c->ring[c->n_renders % rtw_ctx::kRing];
    if (pass.begin) HIP_TRY(c, hipEventRecord(c->ev0, stream));
    HIP_TRY(c, hipEventRecord(ev[0], stream));
    int lrc = 0;
    if (nt == 0 || (dark && kind.zero_fill)) {
        if (nt) HIP_TRY(c, hipMemsetAsync(d_out, 0, rtw::packed_bytes(nt, sizeof(R)), stream));
        HIP_TRY(c, hipEventRecord(ev[1], stream));
    } else {
        if (dark) p.n_tasks = p.n_chunks = 0;
        lrc = rtw::launch_render(p, pl.world, pl.opts, pl.launch_lds,
                                 rtw::Fold<R>{kind.fold, reinterpret_cast<R*>(d_out), pass.accum, pass.first,
                                              cull ? reinterpret_cast<const uint8_t*>(c->cull.d_flags) : nullptr},
                                 stream, ev[1]);
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
    // bookkeeping
    ++c->n_renders;
    c->no_work = false;
    std::vector<uint32_t> tiles;
    c->split.local_tiles(W, H, rank, nranks, tiles);
    const uint64_t before = pass.begin ? 0 : c->last.samples;
    c->last = rtw_stats{};
    c->last.samples = before + rtw::tile_pixels(W, H, tiles) * p.spp;
    // (a culled sample is one segment that misses everything: credited here, the kernel never saw it)
    c->last_culled = cull ? cull->n_culled : 0u;
    if (pass.begin) c->cull_segments = 0;
    if (cull) c->cull_segments += cull->culled_pixels * p.spp;
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
    return ensure(c, &c->d_accum, &c->accum_cap, std::max<size_t>(rtw::packed_bytes(n_local_tiles, sizeof(double)), 64));
}

// A render of this rank's tiles: one pass, or (tuning "window") the windows of
// plan_windows one after another on `stream`, folded onto the context's
// accumulator; the last one writes d_out.
template <typename R>
int render_device_t(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t rank, uint32_t nranks,
                    void* d_out, size_t out_bytes, hipStream_t stream) {
    int rc = check_image_size(c, cam);
    if (rc) return rc;
    const uint32_t spp = cam->samples_per_pixel;
    const uint32_t nt = rtw::tiles_for_rank(cam->image_width, cam->image_height, rank, nranks);
    if (out_bytes < rtw::packed_bytes(nt, sizeof(R))) return fail(c, RTW_E_INVALID, "d_out is smaller than tiles_for_rank*64*3");
    if (nt && !d_out) return fail(c, RTW_E_INVALID, "d_out is NULL");
    rtw::WindowPlan w;   // (window 0: one pass)
    if (c->knobs.window && nt) w = rtw::plan_windows<R>(c->knobs, spp, nt, device_total(c));
    if (w.n_windows <= 1) return render_pass_t<R>(c, cam, seed, rank, nranks, d_out, stream, rtw::one_shot_pass(*cam));
    rc = ensure_accum(c, nt);
    for (uint32_t k = 0; k < w.n_windows && !rc; ++k) {
        // (the chunk is not clamped to a short last window: s_base stays a multiple of it)
        const uint32_t first = k * w.window;
        const rtw::Pass ps = rtw::window_pass(first, std::min(w.window, spp - first), w.chunk,
                                              reinterpret_cast<double*>(c->d_accum), k == 0, spp);
        rc = render_pass_t<R>(c, cam, seed, rank, nranks, k + 1 == w.n_windows ? d_out : nullptr, stream, ps);
    }
    return rc;
}

// The samples per item of a window of n samples (rtw_render_window_device);
// windows continue each other only when they start on an item boundary.
template <typename R>
uint32_t window_chunk(rtw_ctx* c, uint32_t n, uint32_t nt) {
    return c->knobs.chunk ? c->knobs.chunk : rtw::plan_chunk<R>(c->knobs, n, nt, device_total(c));
}

// rtw_render_window_device on a one-device context: its arguments checked
// (before anything is launched), then the one window pass
template <typename R>
int render_window_t(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t rank, uint32_t nranks,
                    uint32_t first, uint32_t n, double* d_accum, size_t accum_bytes, hipStream_t stream) {
    const uint32_t nt = rtw::tiles_for_rank(cam->image_width, cam->image_height, rank, nranks);
    const uint32_t chunk = window_chunk<R>(c, n, nt);
    if (first % chunk)
        return fail(c, RTW_E_INVALID, "first_sample is not a multiple of the chunk (" + std::to_string(chunk) + ")");
    if (accum_bytes < rtw::packed_bytes(nt, sizeof(double)))
        return fail(c, RTW_E_INVALID, "d_accum is smaller than tiles_for_rank*64*3 doubles");
    if (nt && !d_accum) return fail(c, RTW_E_INVALID, "d_accum is NULL");
    if (n == 0) return RTW_OK;
    const int rc = check_image_size(c, cam);
    if (rc) return rc;
    c->stats_ranks = 1;
    // the task-order key of a window render: the camera without its sample count
    rtw::Pass ps = rtw::window_pass(first, n, chunk, d_accum, true, 0);
    if (nt == 0) ps.kind = rtw::kPassOneShot;   // nothing to fold: the bookkeeping of an empty render
    return render_pass_t<R>(c, cam, seed, rank, nranks, nullptr, stream, ps);
}

// rtw_render_window_image on a multi-device context: every rank folds the
// window onto its own packed f64 accumulator (rank 0's is its slot of the
// gather target), continued from the caller's sums; ONE gather, the assembly
// in f64 whatever the precision, the download.
template <typename R>
int render_window_multi_t(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t first, uint32_t n_samples,
                          double* sums, rtw_stats* stats) {
    const uint32_t W = cam->image_width, H = cam->image_height, n = rtw_device_count(c);
    hipStream_t s0 = c->stream;
    // every rank's window is checked before any rank launches
    for (uint32_t k = 0; k < n; ++k) {
        rtw_ctx* ck = rtw_device_ctx(c, k);
        HIP_TRY(c, hipSetDevice(ck->device));
        const uint32_t chunk = window_chunk<R>(ck, n_samples, rtw::tiles_for_rank(W, H, k, n));
        if (first % chunk) {
            (void)hipSetDevice(c->device);
            return fail(c, RTW_E_INVALID, "first_sample is not a multiple of the chunk (" + std::to_string(chunk) + ")");
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (n_samples == 0) return RTW_OK;
    int rc = check_image_size(c, cam);
    if (rc) return rc;
    const size_t per = std::max<size_t>((size_t)rtw::tiles_for_rank(W, H, 0, n) * 64 * 3, 1), img = (size_t)W * H * 3;
    rc = ensure(c, &c->d_gather, &c->gather_cap, (size_t)n * per * sizeof(double));
    if (!rc) rc = ensure(c, &c->d_img, &c->img_cap, std::max<size_t>(img * sizeof(double), 64));
    if (rc) return rc;
    const uint32_t* slot = nullptr;
    if (c->split.active(W, H, n)) {
        rc = ensure_tile_slot(c, n);
        if (rc) return rc;
        slot = reinterpret_cast<const uint32_t*>(c->split.d_tile_slot);
    }
    // (the previous call's gather + assembly may still read d_gather on another stream)
    if (c->gather_pending) HIP_TRY(c, hipStreamWaitEvent(s0, c->gather_ev, 0));
    std::vector<std::vector<double>> packed(n);   // the uploads read them until the streams are waited for
    std::vector<const void*> src(n, c->d_gather);
    std::vector<uint32_t> tiles;
    auto ranks = [&]() -> int {
        for (uint32_t k = 0; k < n; ++k) {
            rtw_ctx* ck = rtw_device_ctx(c, k);
            HIP_TRY(c, hipSetDevice(ck->device));
            c->split.local_tiles(W, H, k, n, tiles);
            hipStream_t s = k ? ck->stream : s0;
            if (k) {
                // (rank 0's tile count, the most: the gather reads equal-size buffers)
                const int erc = ensure_accum(ck, rtw::tiles_for_rank(W, H, 0, n));
                if (erc) return fail(c, erc, ck->err);
                src[k] = ck->d_accum;
            }
            double* acc = k ? reinterpret_cast<double*>(ck->d_accum) : reinterpret_cast<double*>(c->d_gather);
            const size_t bytes = rtw::packed_bytes((uint32_t)tiles.size(), sizeof(double));
            if (first && bytes) {
                packed[k].resize(tiles.size() * 64 * 3);
                rtw::image_to_packed(sums, W, H, tiles, packed[k].data());
                HIP_TRY(c, hipMemcpyAsync(acc, packed[k].data(), bytes, hipMemcpyHostToDevice, s));
            }
            const int wrc = render_window_t<R>(ck, cam, seed, k, n, first, n_samples, acc, bytes, s);
            if (wrc) return k ? fail(c, wrc, ck->err) : wrc;
        }
        return gather_ranks(c, src, per, sizeof(double), s0);
    };
    rc = ranks();
    if (!rc) rc = hipSetDevice(c->device) == hipSuccess ? RTW_OK : fail(c, RTW_E_DEVICE, "hipSetDevice failed");
    if (!rc && rtw::launch_assemble(reinterpret_cast<const double*>(c->d_gather), per, n, W, H, slot,
                                    reinterpret_cast<double*>(c->d_img), s0))
        rc = fail(c, RTW_E_DEVICE, std::string("assemble launch failed: ") + hipGetErrorString(hipGetLastError()));
    if (!rc) rc = gather_done(c, s0);
    if (rc) {
        // the first error is the call's; no buffer (the uploads' host side included) stays in use
        for (uint32_t k = 0; k < n; ++k) {
            rtw_ctx* ck = rtw_device_ctx(c, k);
            if (hipSetDevice(ck->device) == hipSuccess) (void)hipStreamSynchronize(k ? ck->stream : s0);
        }
        (void)hipSetDevice(c->device);
        return rc;
    }
    c->stats_ranks = n;
    if (img) HIP_TRY(c, hipMemcpyAsync(sums, c->d_img, img * sizeof(double), hipMemcpyDeviceToHost, s0));
    HIP_TRY(c, hipStreamSynchronize(s0));
    return fetch_stats(c, stats);
}

}  // namespace

// the assembly's map of the active split (host/tiles.hpp tile_slots)
int ensure_tile_slot(rtw_ctx* c, uint32_t nranks) {
    SplitState& s = c->split;
    if (s.d_tile_slot && s.tile_slot_key == s.serial) return RTW_OK;
    const int rc = upload_map(c, &s.d_tile_slot, &s.tile_slot_cap, rtw::tile_slots(s.rank, nranks));
    if (rc) return rc;
    s.tile_slot_key = s.serial;
    return RTW_OK;
}

size_t device_total(rtw_ctx* c) {
    if (!c->dev_total) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) c->dev_total = tot;
    }
    return c->dev_total;
}

int render_pass(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t rank, uint32_t nranks, void* d_out,
                hipStream_t stream, const rtw::Pass& pass) {
    return by_precision(c, [&](auto r) {
        return render_pass_t<decltype(r)>(c, cam, seed, rank, nranks, d_out, stream, pass);
    });
}

extern "C" {

int rtw_assemble_tiles(rtw_ctx* c, const void* d_ranks, size_t rank_stride_bytes, uint32_t nranks, uint32_t W,
                       uint32_t H, void* d_image, void* stream) {
    if (!c || nranks == 0) return fail(c, RTW_E_INVALID, "bad argument");
    const size_t esz = c->precision == RTW_F32 ? sizeof(float) : sizeof(double);
    if ((uint64_t)W * H == 0) return RTW_OK;
    if (!d_ranks || !d_image || rank_stride_bytes % esz)
        return fail(c, RTW_E_INVALID, "bad assemble buffers");
    if (rank_stride_bytes < rtw::packed_bytes(rtw::tiles_for_rank(W, H, 0, nranks), esz))
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
    const int rc = by_precision(c, [&](auto r) {
        using R = decltype(r);
        return rtw::launch_assemble(reinterpret_cast<const R*>(d_ranks), stride, nranks, W, H, slot,
                                    reinterpret_cast<R*>(d_image), s);
    });
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
    return by_precision(c, [&](auto r) {
        return render_device_t<decltype(r)>(c, cam, seed, rank, nranks, d_out, out_bytes, s);
    });
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
    hipStream_t s = resolve_stream(c, stream);
    return by_precision(c, [&](auto r) {
        return render_window_t<decltype(r)>(c, cam, seed, rank, nranks, first_sample, n_samples, d_accum, accum_bytes, s);
    });
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
    // image [H][W][3] <-> packed tiles [lt][ly * 8 + lx][3] (host/tiles.hpp)
    std::vector<double> packed(n, 0.0);
    if (first_sample && n_samples && n) {
        rtw::image_to_packed(sums, W, H, tiles, packed.data());
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
    rtw::packed_to_image(packed.data(), W, H, tiles, sums);
    return fetch_stats(c, stats);
}

int rtw_render_window_image(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t first_sample, uint32_t n_samples,
                            double* sums, rtw_stats* stats) {
    if (!c || !cam || !sums) return fail(c, RTW_E_INVALID, "bad argument");
    if (!c->multi) return rtw_render_window(c, cam, seed, first_sample, n_samples, sums, stats);
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    if ((uint64_t)first_sample + n_samples > 0xFFFFFFFFull)
        return fail(c, RTW_E_INVALID, "first_sample + n_samples overflows");
    return by_precision(c, [&](auto r) {
        return render_window_multi_t<decltype(r)>(c, cam, seed, first_sample, n_samples, sums, stats);
    });
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
    return fetch_stats(c, stats);
}

}  // extern "C"
