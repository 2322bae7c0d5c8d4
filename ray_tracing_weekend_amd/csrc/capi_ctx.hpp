// capi_ctx.hpp -- private to the C-ABI units (capi.cpp, capi_render.cpp,
// capi_lpt.cpp, capi_adaptive.cpp, capi_multi.cpp, capi_query.cpp, capi_nee.cpp,
// capi_path.cpp, capi_wavefront.cpp, capi_features.cpp, capi_denoise.cpp, capi_denoise_variance.cpp,
// capi_moments.cpp): the context behind include/rtw.h's rtw_ctx and the
// helpers they share.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: the functions are resolved at run time (capi_multi.cpp rccl_api)
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/rtw.h"
#include "host/lpt_state.hpp"
#include "host/render_pass.hpp"
#include "host/render_plan.hpp"
#include "host/stage_scene.hpp"
#include "host/tile_cull.hpp"
#include "host/tiles.hpp"
#include "rtw_kernels.h"

using rtw::LptKey;

// longest-tiles-first task order: the state (host/lpt_state.hpp) and its device
// half (capi_lpt.cpp; build_task_list: host/render_plan.hpp)
struct LptCache {
    rtw::LptState st;
    void* d_cost = nullptr;           // [tile cost]; a pilot: [tile cost | chunk sums | tiles]
    size_t cost_cap = 0;
    hipEvent_t ev = nullptr;          // after the last counting render (st.pending)
    void* d_tasks = nullptr;          // the task list st.h_tasks
    size_t tasks_cap = 0;
};

// Provably empty tiles (host/tile_cull.hpp): the flags of the last classified key
// and their plain-order task list, with their device copies (capi_render.cpp)
struct CullCache {
    rtw::CullState st;
    void* d_flags = nullptr;          // st.flags
    size_t flags_cap = 0;
    void* d_tasks = nullptr;          // st.h_tasks
    size_t tasks_cap = 0;
};

// Rank split (ABI 10): renders of a W x H image over n ranks give tile T to
// rank rank[T] (rtw_set_split; empty: T mod n, the round robin).  Each rank
// keeps the round robin's tile COUNT, so the packed buffers and the gather are
// unchanged.  cost: the tile costs the split was dealt by -- they order the
// next renders' tasks (no counting render after a deal).  automatic: dealt by
// rtw_render_image_device (tuning "balance") for cam / scene, re-dealt when
// they change.
struct SplitState {
    uint32_t W = 0, H = 0, n = 0;
    uint64_t serial = 0;              // ++ per split set: the split's id in the task-order key
    bool automatic = false;
    rtw_camera cam{};
    uint64_t scene = 0;
    std::vector<uint32_t> rank, cost;
    // the device copies of the split: this rank's local tile -> global tile (render
    // kernel) and global tile -> lt * n + rank (assembly), for split id *_key
    std::vector<uint32_t> h_tile_map;
    void* d_tile_map = nullptr;
    size_t tile_map_cap = 0;
    uint64_t tile_map_key = 0;
    uint32_t tile_map_rank = 0;
    void* d_tile_slot = nullptr;
    size_t tile_slot_cap = 0;
    uint64_t tile_slot_key = 0;
    // a split is set for renders of this image size and rank count
    bool active(uint32_t w, uint32_t h, uint32_t nranks) const {
        return !rank.empty() && W == w && H == h && n == nranks;
    }
    // the id of the split renders of (w, h, nranks) follow: 0 = the round robin
    uint64_t id(uint32_t w, uint32_t h, uint32_t nranks) const { return active(w, h, nranks) ? serial : 0; }
    // the global tiles of rank r, in the order they are packed
    void local_tiles(uint32_t w, uint32_t h, uint32_t r, uint32_t nranks, std::vector<uint32_t>& out) const {
        rtw::local_tiles(active(w, h, nranks) ? &rank : nullptr, w, h, r, nranks, out);
    }
};

// Batched ray queries (capi_query.cpp) and the feature pass (capi_features.cpp):
// their counters, events and staging buffers, allocated by the first of them.
struct QueryState {
    // rtw::kQueryCounters counters, then the feature pass's next tile (kFeatureNextTile)
    unsigned long long* d_counters = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the queries' host forms' staging: rays in, records out
    void* d_rays = nullptr;
    size_t rays_cap = 0;
    void* d_out = nullptr;
    size_t out_cap = 0;
    void* d_ids = nullptr;
    size_t ids_cap = 0;
    // rtw_render_features' staging: the sums, the counts, the ids
    void* d_feat = nullptr;
    size_t feat_cap = 0;
    void* d_feat_counts = nullptr;
    size_t feat_counts_cap = 0;
    void* d_feat_ids = nullptr;
    size_t feat_ids_cap = 0;
    // the wavefront path rounds (capi_wavefront.cpp): the driver's two path states, round
    // arrays and colours in one allocation (host/wavefront_plan.hpp), the host form's sums,
    // {the survivor count, kQueryCounters totals of a driver call} with a pinned host word
    // for the count's readback, and the event a driver call starts at
    void* d_wf = nullptr;
    size_t wf_cap = 0;
    void* d_wf_sums = nullptr;
    size_t wf_sums_cap = 0;
    unsigned long long* d_wf_words = nullptr;
    unsigned long long* h_wf_count = nullptr;
    hipEvent_t ev_span = nullptr;
    rtw_query_stats last{};
    bool any = false;                 // a query was launched
};

// rtw_denoise (capi_denoise.cpp) and rtw_denoise_variance (capi_denoise_variance.cpp):
// the record arrays, the counters and events and the host forms' staging, allocated by
// the first denoise and grown on demand.
struct DenoiseState {
    // guide | albedo | colour 0 | colour 1 (host/denoise_plan.hpp), then the variance
    // filter's variance 0 | variance 1 (host/denoise_variance_plan.hpp)
    void* d_records = nullptr;
    size_t records_cap = 0;
    unsigned long long* d_counters = nullptr;   // {filled, left non-finite}
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the host form's staging: sums, features, counts in; the means out
    void* d_sums = nullptr;
    size_t sums_cap = 0;
    void* d_features = nullptr;
    size_t features_cap = 0;
    void* d_counts = nullptr;
    size_t counts_cap = 0;
    void* d_moments = nullptr;        // (the variance filter's)
    size_t moments_cap = 0;
    void* d_out = nullptr;
    size_t out_cap = 0;
    rtw_denoise_stats last{};
    bool any = false;                 // a denoise was launched
};

struct rtw_ctx {
    int device = 0;
    int precision = RTW_F32;
    rtw::RenderKnobs knobs;
    size_t dev_total = 0;         // the device's memory (hipMemGetInfo), 0 until asked
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // ring of per-render event triples: [start, after render kernel, after reduce]
    static constexpr int kRing = 64;
    hipEvent_t ring[kRing][3] = {};
    uint64_t n_renders = 0;
    // device scene (one allocation holding every array)
    void* d_scene = nullptr;
    size_t scene_bytes = 0;           // allocation
    size_t scene_used = 0;            // the current scene's bytes
    rtw::SceneScale scale;            // of the staged scene (knob robust = 2, the lpt heuristic)
    rtw::DevScene<float> sc32{};
    rtw::DevScene<double> sc64{};
    bool has_scene = false;
    bool has_lambertian = false;      // the staged scene holds a Lambertian material (rtw_shade_rays)
    uint64_t scene_serial = 0;        // ++ per rtw_upload_scene
    // work buffers
    void* d_partial = nullptr;
    size_t partial_cap = 0;
    void* d_accum = nullptr;      // sample windows: the f64 running sums of this rank's packed tiles
    size_t accum_cap = 0;
    // adaptive sampling (capi_adaptive.cpp adaptive_buffers): per global tile the f64 colour
    // sums and {S1, S2}, the counts and flags, two tile lists and their {length, pixels};
    // then the image-order sums and counts of the host form
    void* d_adapt = nullptr;
    size_t adapt_cap = 0;
    void* d_adapt_img = nullptr;
    size_t adapt_img_cap = 0;
    // d_adapt holds the whole state of a finished one-device adaptive render of this image
    // size (rtw_adaptive_moments reads its {S1, S2}); rtw_set_scene forgets it
    bool adapt_done = false;
    uint32_t adapt_w = 0, adapt_h = 0;
    // rtw_render_window_moments' host form: the image-order sums, then the moments
    void* d_moments_img = nullptr;
    size_t moments_img_cap = 0;
    // ... and two pinned host words: the {length, pixels} read back after each pass (a
    // copy into pageable memory could hold the host until the pass is done)
    uint32_t* h_adapt = nullptr;
    void* d_out = nullptr;        // rtw_render: the packed tiles, then the image
    size_t out_cap = 0;
    void* d_img = nullptr;
    size_t img_cap = 0;
    unsigned long long* d_counters = nullptr;
    std::vector<unsigned char> h_out;
    LptCache lpt;
    // f64 contexts: what the tile classifier reads of the staged scene (shared by the ranks)
    std::shared_ptr<const rtw::CullScene> cull_scene;
    CullCache cull;
    uint32_t last_culled = 0;         // provably empty tiles of the last render (rtw_culled_tiles)
    uint64_t cull_segments = 0;       // ... their samples so far, one segment each (stats.segments)
    SplitState split;
    rtw_stats last{};
    int last_variant = 0;             // render kernel of the last render: rtw_kernels.h variant_code
    uint32_t last_n_sph = 0;
    uint32_t last_light_bvh = 0;      // KParams::light_bvh of the last render (0: the linear light loop)
    uint32_t last_n_list = 0;         // ... and its light-list length
    std::string err;
    // multi-device context (rtw_create_devices): this context is rank 0 on the
    // first device; peers[k - 1] is the context of rank k on device k of the
    // list, mirroring every knob and the scene.  One RCCL communicator per rank
    // (a single-process clique) for the framebuffer gather to rank 0.
    bool multi = false;
    std::vector<rtw_ctx*> peers;
    std::vector<ncclComm_t> comms;
    void* d_gather = nullptr;         // rank 0's device: the n ranks' packed tiles (gather target)
    size_t gather_cap = 0;
    // virtual ranks (rtw_create_virtual, a test mode): every rank on one device,
    // the gather done by device copies on rank 0's stream after peer_ev[k - 1]
    bool virt = false;
    std::vector<hipEvent_t> peer_ev;
    // the last multi-device gather + assembly, on rank 0's stream of that call:
    // the next call's renders (every rank) wait for it before they overwrite
    // d_gather or a peer's packed tiles
    hipEvent_t gather_ev = nullptr;
    bool gather_pending = false;
    // ranks whose counters the last render filled (rtw_get_stats): n after
    // rtw_render / rtw_render_image_device, 1 after rtw_render_device
    uint32_t stats_ranks = 1;
    // the last multi-device render gave this rank no tile: its stats are those of no work
    bool no_work = false;
    // batched ray queries and the feature pass: their own buffers, counters and events,
    // allocated by the first of them -- nothing of the render's is touched
    QueryState* query = nullptr;
    // rtw_denoise: its own state as well, allocated by the first denoise
    DenoiseState* denoise = nullptr;
};

static inline int fail(rtw_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
static inline int hip_fail(rtw_ctx* c, hipError_t e, const char* what) {
    return fail(c, RTW_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(ctx, expr)                                   \
    do {                                                     \
        hipError_t e_ = (expr);                              \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #expr); \
    } while (0)

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// grow a device buffer to at least `bytes` (its contents are not kept)
static inline int ensure(rtw_ctx* c, void** buf, size_t* cap, size_t bytes) {
    if (*cap >= bytes) return RTW_OK;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    HIP_TRY(c, hipMalloc(buf, bytes));
    *cap = bytes;
    return RTW_OK;
}

// the caller's stream argument: NULL = the context's own stream,
// RTW_STREAM_NULL = the device's null (legacy default) stream, else a hipStream_t
static inline hipStream_t resolve_stream(const rtw_ctx* c, void* stream) {
    if (!stream) return c->stream;
    if (stream == RTW_STREAM_NULL) return nullptr;
    return reinterpret_cast<hipStream_t>(stream);
}

// the key of tile costs counted by a render of (cam, rank, nranks) on this context
static inline LptKey lpt_key(const rtw_ctx* c, const rtw_camera* cam, uint32_t rank, uint32_t nranks) {
    return LptKey{*cam, c->scene_serial, rank, nranks, c->precision == RTW_F32 ? 4u : 8u,
                  c->split.id(cam->image_width, cam->image_height, nranks)};
}

// f(R{}) for the context's precision R
template <typename F>
auto by_precision(const rtw_ctx* c, F&& f) {
    return c->precision == RTW_F32 ? f(float{}) : f(double{});
}
template <typename R>
const rtw::DevScene<R>& dev_scene(const rtw_ctx* c) {
    if constexpr (sizeof(R) == 4) return c->sc32;
    else return c->sc64;
}

// the kernel holds a lane's pixel as i | j << 16
static inline int check_image_size(rtw_ctx* c, const rtw_camera* cam) {
    if (cam->image_width > 65535 || cam->image_height > 65535)
        return fail(c, RTW_E_UNSUPPORTED, "image width or height beyond 65535");
    return RTW_OK;
}

// the end of a blocking entry point: the stats of the render it waited for
static inline int fetch_stats(rtw_ctx* c, rtw_stats* stats) {
    rtw_stats st{};
    const int rc = rtw_get_stats(c, &st);
    if (stats) *stats = st;
    return rc;
}

// multi-device: every rank alike -- f(peer context) on each peer; the first
// failure is reported on c
template <typename F>
int on_peers(rtw_ctx* c, F&& f) {
    for (rtw_ctx* pk : c->peers) {
        const int rc = f(pk);
        if (rc) return fail(c, rc, pk->err);
    }
    return RTW_OK;
}

// capi.cpp: the split (and its costs) on one rank context; tile_rank NULL: the round robin
int apply_split(rtw_ctx* c, uint32_t W, uint32_t H, uint32_t nranks, const uint32_t* tile_rank,
                const uint32_t* tile_cost, bool automatic, const rtw_camera* cam);
// capi.cpp: the stats of the last render of one rank context (rtw_get_stats sums them)
int get_stats_one(rtw_ctx* c, rtw_stats* out);
// capi_render.cpp: the device's memory, asked once (plan_chunk / plan_windows budget)
size_t device_total(rtw_ctx* c);
// capi_render.cpp: one pass of a render of this rank's tiles on `stream` (a window pass
// writes d_out when it is non-null; d_out holds the rank's packed tiles: the caller checked)
int render_pass(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t rank, uint32_t nranks, void* d_out,
                hipStream_t stream, const rtw::Pass& pass);
// capi_lpt.cpp: the task order of a render of `key` (the plan says longest tiles first
// applies) -- with costs, p.task_table; a render that counts them on the way, p.tile_cost
// skip (may be null): [local tile] 1 = provably empty, left out of the task list and
// of cost 0; cull_id: the flags' id (CullState::serial; 0: none)
template <typename R>
int lpt_prepare(rtw_ctx* c, rtw::KParams<R>& p, const rtw::RenderPlan& pl, const LptKey& key, bool split_has_costs,
                hipStream_t stream, const uint8_t* skip = nullptr, uint32_t cull_id = 0);
// capi_lpt.cpp: after the launch of a render that counts (p.tile_cost)
int lpt_counted(rtw_ctx* c, const LptKey& key, hipStream_t stream);
// capi_lpt.cpp: the tile costs the context counted for (cam, rank, nranks) under
// its split, scattered into cost[global tile]; waits for a pending counting render
int tile_costs_of(rtw_ctx* c, const rtw_camera* cam, uint32_t rank, uint32_t nranks, uint32_t* cost);
// capi_render.cpp: the assembly's map of the active split on the device (split.d_tile_slot)
int ensure_tile_slot(rtw_ctx* c, uint32_t nranks);
// capi_multi.cpp: ONE gather of the n ranks' packed buffers (`count` elements of
// elem_bytes -- 4: f32, 8: f64, 1: bytes -- each) to c->d_gather on rank 0, slot k
// from src[k] on rank k's stream after the work queued there; rank 0 (on s0) filled
// its slot in place.  RCCL, or on virtual ranks device copies on s0.
int gather_ranks(rtw_ctx* c, const std::vector<const void*>& src, size_t count, size_t elem_bytes, hipStream_t s0);
// capi_multi.cpp: after the assembly that read the gathered buffers on s0: every
// rank's next work waits for it
int gather_done(rtw_ctx* c, hipStream_t s0);
// capi_multi.cpp: rtw_destroy's part for the ranks of a multi-device context
void destroy_ranks(rtw_ctx* c);
// capi_query.cpp: rtw_destroy's part for the query state (the context's device is current)
void destroy_query(rtw_ctx* c);
// capi_query.cpp: the context's query state, allocated on first use
int query_state(rtw_ctx* c);
// capi_denoise.cpp: rtw_destroy's part for the denoise state (the context's device is current)
void destroy_denoise(rtw_ctx* c);
// capi_denoise.cpp: the context's denoise state, allocated on first use
int denoise_state(rtw_ctx* c);
