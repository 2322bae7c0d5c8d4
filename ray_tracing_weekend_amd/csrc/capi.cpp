// capi.cpp -- the C-ABI (include/rtw.h): context, tuning, scene upload, the
// rank split and stats.  The render entry points are in capi_render.cpp,
// capi_lpt.cpp (task order) and capi_adaptive.cpp (adaptive sampling, on one
// device and over the ranks), multi-device contexts in capi_multi.cpp, the
// entry points that are pure host code (camera, scene generators, encoding) in
// host/rtw_host.cpp.
#include <algorithm>
#include <new>
#include <type_traits>

#include "capi_ctx.hpp"
#include "host/bvh.hpp"

extern "C" {

int rtw_abi_version(void) { return RTW_ABI_VERSION; }

rtw_ctx* rtw_create(int device, int precision) {
    if (precision != RTW_F32 && precision != RTW_F64) return nullptr;
    rtw_ctx* c = new (std::nothrow) rtw_ctx();
    if (!c) return nullptr;
    c->device = device;
    c->precision = precision;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_counters), rtw::kCounters * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(c->d_counters, 0, rtw::kCounters * sizeof(unsigned long long)) != hipSuccess) {
        rtw_destroy(c);
        return nullptr;
    }
    for (auto& tri : c->ring)
        for (auto& e : tri)
            if (hipEventCreate(&e) != hipSuccess) {
                rtw_destroy(c);
                return nullptr;
            }
    return c;
}

void rtw_destroy(rtw_ctx* c) {
    if (!c) return;
    destroy_ranks(c);
    (void)hipSetDevice(c->device);
    if (c->gather_ev) (void)hipEventDestroy(c->gather_ev);
    if (c->d_gather) (void)hipFree(c->d_gather);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    destroy_query(c);
    destroy_denoise(c);
    if (c->d_scene) (void)hipFree(c->d_scene);
    if (c->d_partial) (void)hipFree(c->d_partial);
    if (c->d_accum) (void)hipFree(c->d_accum);
    if (c->d_adapt) (void)hipFree(c->d_adapt);
    if (c->d_adapt_img) (void)hipFree(c->d_adapt_img);
    if (c->d_moments_img) (void)hipFree(c->d_moments_img);
    if (c->h_adapt) (void)hipHostFree(c->h_adapt);
    if (c->d_out) (void)hipFree(c->d_out);
    if (c->d_img) (void)hipFree(c->d_img);
    if (c->d_counters) (void)hipFree(c->d_counters);
    if (c->lpt.d_cost) (void)hipFree(c->lpt.d_cost);
    if (c->lpt.d_tasks) (void)hipFree(c->lpt.d_tasks);
    if (c->cull.d_flags) (void)hipFree(c->cull.d_flags);
    if (c->cull.d_tasks) (void)hipFree(c->cull.d_tasks);
    if (c->split.d_tile_map) (void)hipFree(c->split.d_tile_map);
    if (c->split.d_tile_slot) (void)hipFree(c->split.d_tile_slot);
    if (c->lpt.ev) (void)hipEventDestroy(c->lpt.ev);
    for (auto& tri : c->ring)
        for (auto& e : tri)
            if (e) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* rtw_last_error(const rtw_ctx* c) { return c ? c->err.c_str() : "null context"; }
int rtw_precision(const rtw_ctx* c) { return c ? c->precision : -1; }

int rtw_set_chunk(rtw_ctx* c, uint32_t chunk) {
    if (!c) return RTW_E_INVALID;
    c->knobs.chunk = chunk;
    return on_peers(c, [&](rtw_ctx* pk) { return rtw_set_chunk(pk, chunk); });
}
int rtw_set_tuning(rtw_ctx* c, const char* key, int64_t value) {
    if (!c || !key) return RTW_E_INVALID;
    const int prc = on_peers(c, [&](rtw_ctx* pk) { return rtw_set_tuning(pk, key, value); });
    if (prc) return prc;
    const std::string k = key;
    rtw::RenderKnobs& t = c->knobs;
    if (k == "window") {   // the one key with a negative value: -1 = auto
        if (value < rtw::RenderKnobs::kWindowAuto) return fail(c, RTW_E_INVALID, "window: -1 (auto), 0 (off) or a sample count");
        t.window = std::min<int64_t>(value, 0xFFFFFFFFll);
        return RTW_OK;
    }
    if (value < 0) return fail(c, RTW_E_INVALID, "negative tuning value");
    if (k == "chunk") t.chunk = (uint32_t)value;
    else if (k == "auto_chunk") t.auto_chunk = std::max<uint32_t>(1, (uint32_t)value);
    else if (k == "robust") t.robust = (int)std::min<int64_t>(value, 2);
    else if (k == "bvh_leaf") t.bvh_leaf = (uint32_t)std::min<int64_t>(value, 15);
    else if (k == "light_leaf") t.light_leaf = (uint32_t)std::min<int64_t>(value, 15);
    else if (k == "persist") t.persist = value == 1 ? rtw::kPersistResident : (uint32_t)std::min<int64_t>(value, 1 << 20);
    else if (k == "query_grid") t.query_grid = (uint32_t)std::min<int64_t>(value, 1 << 20);
    else if (k == "light_grid") t.light_grid = (uint32_t)std::min<int64_t>(value, 1024);
    else if (k == "item_order") t.item_order = value ? 1u : 0u;
    else if (k == "hit64") t.hit64 = value ? 1u : 0u;
    else if (k == "lpt") t.lpt = (uint32_t)std::min<int64_t>(value, 2);
    else if (k == "lpt_min_spp") t.lpt_min_spp = (uint32_t)std::min<int64_t>(value, 1u << 30);
    else if (k == "lpt_inline") t.lpt_inline = value ? 1u : 0u;
    else if (k == "lpt_pilot_spp") t.lpt_pilot_spp = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 1), 64);
    else if (k == "lpt_pilot_depth") t.lpt_pilot_depth = (uint32_t)std::min<int64_t>(value, 1u << 20);
    else if (k == "light_bvh_min") t.light_bvh_min = (uint32_t)std::min<int64_t>(value, 1u << 30);
    else if (k == "max_group") { t.max_group = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 1), 4095); c->lpt.st.tab_valid = false; }
    else if (k == "grid_piece") t.grid_piece = (uint32_t)std::min<int64_t>(value, 1u << 20);
    else if (k == "partial_max") t.partial_max = std::max<size_t>(1 << 20, (size_t)value);
    else if (k == "group") t.group = (uint32_t)value;
    else if (k == "target_tasks") t.target_tasks = std::max<uint64_t>(1, (uint64_t)value);
    else if (k == "lds") t.world_pref = value ? 1 : 0;
    else if (k == "bvh_ww") t.bvh_kind = value ? 1 : 0;
    else if (k == "bvh_kind") t.bvh_kind = (int)std::min<int64_t>(value, 3);
    else if (k == "bvh_lds_max") t.bvh_lds_max = (size_t)std::min<int64_t>(value, rtw::kLdsLimit);
    else if (k == "auto_accel") t.auto_accel = (int)std::min<int64_t>(value, RTW_ACCEL_BVH);
    else if (k == "balance") t.balance = value ? 1u : 0u;
    else if (k == "cost_time") t.cost_time = value ? 1u : 0u;
    else if (k == "tile_cull") t.tile_cull = value ? 1u : 0u;
    else if (k == "denoise_lds") t.denoise_lds = (uint32_t)std::min<int64_t>(value, 2);
    else if (k == "guide_div") { t.guide_div = (uint32_t)std::min<int64_t>(value, 1 << 24); c->lpt.st.tab_valid = false; }
    else if (k == "guide_max") { t.guide_max = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 1), 4095); c->lpt.st.tab_valid = false; }
    else if (k == "guide_floor") { t.guide_floor = std::max<uint64_t>(1, (uint64_t)value); c->lpt.st.tab_valid = false; }
    else return fail(c, RTW_E_INVALID, "unknown tuning key " + k);
    return RTW_OK;
}

int rtw_set_accel(rtw_ctx* c, int accel) {
    if (!c) return RTW_E_INVALID;
    if (accel < RTW_ACCEL_AUTO || accel > RTW_ACCEL_BVH) return fail(c, RTW_E_UNSUPPORTED, "accel not available");
    c->knobs.accel = accel;
    return on_peers(c, [&](rtw_ctx* pk) { return rtw_set_accel(pk, accel); });
}

// one device's copy of a staged scene (rtw_set_scene stages once, then
// uploads to every device of the context)
static int upload_scene(rtw_ctx* c, const std::vector<unsigned char>& blob, rtw::DevScene<float> tmp32,
                        rtw::DevScene<double> tmp64, const rtw::SceneScale& scale) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->scene_bytes < blob.size()) {
        if (c->d_scene) (void)hipFree(c->d_scene);
        c->d_scene = nullptr;
        c->scene_bytes = 0;
        HIP_TRY(c, hipMalloc(&c->d_scene, blob.size()));
        c->scene_bytes = blob.size();
    }
    c->scene_used = blob.size();
    c->scale = scale;
    const uintptr_t base = reinterpret_cast<uintptr_t>(c->d_scene);
    auto rebase = [base](auto& ds) {
        auto fix = [base](auto*& ptr) {
            using T = std::remove_reference_t<decltype(ptr)>;
            ptr = reinterpret_cast<T>(reinterpret_cast<uintptr_t>(ptr) + base);
        };
        fix(ds.sph); fix(ds.sph_r); fix(ds.sph_mat); fix(ds.sph_shade); fix(ds.planes); fix(ds.plane_mat);
        fix(ds.mat_type); fix(ds.mat_p); fix(ds.lights); fix(ds.bvh); fix(ds.bsph); fix(ds.bid);
        fix(ds.bvh4); fix(ds.lbvh);
        fix(ds.lsph); fix(ds.lid); fix(ds.lg_start); fix(ds.lg_sph); fix(ds.lg_id); fix(ds.lg_rec);
        fix(ds.quads); fix(ds.quad_mat); fix(ds.lquads); fix(ds.sph64); fix(ds.pl64); fix(ds.mat64);
        if (ds.lref) fix(ds.lref);
        if constexpr (std::is_same<std::decay_t<decltype(ds)>, rtw::DevScene<double>>::value) {
            fix(ds.bvh32);
            fix(ds.bsph32);
            fix(ds.lg_sph32);
        }
        fix(ds.boxes); fix(ds.box_mat);
        if (ds.mat_tex) fix(ds.mat_tex);
        fix(ds.tex_type); fix(ds.tex_p); fix(ds.tex_refs); fix(ds.perlin_vec); fix(ds.perlin_perm);
    };
    static_assert(offsetof(rtw::DevScene<float>, n_sph) == 35 * sizeof(void*),
                  "DevScene gained a pointer: update rebase");
    if (c->precision == RTW_F32) {
        rebase(tmp32);
        c->sc32 = tmp32;
    } else {
        rebase(tmp64);
        c->sc64 = tmp64;
    }
    HIP_TRY(c, hipMemcpy(c->d_scene, blob.data(), blob.size(), hipMemcpyHostToDevice));
    c->has_scene = true;
    ++c->scene_serial;
    c->adapt_done = false;   // (rtw_adaptive_moments: the state is another scene's)
    return RTW_OK;
}

int rtw_set_scene(rtw_ctx* c, const rtw_scene* s) {
    if (!c) return RTW_E_INVALID;
    std::string msg;
    int rc = rtw::validate_scene(s, &msg);
    if (rc) return fail(c, rc, msg);
    // stage once against base 0 (upload_scene rebases the device pointers:
    // EVERY pointer member of DevScene must be listed in its `rebase`)
    rtw::DevScene<float> tmp32{};
    rtw::DevScene<double> tmp64{};
    const rtw::RenderKnobs& t = c->knobs;
    const uint32_t leaf = rtw::auto_leaf(t.bvh_leaf, s->n_spheres, c->precision == RTW_F64);
    const uint32_t light_leaf = t.light_leaf ? t.light_leaf : rtw::kLeafMax;
    // the light grid only for light lists long enough to skip the linear loop
    const double grid = s->n_lights >= t.light_bvh_min ? t.light_grid / 16.0 : 0.0;
    // f64: the classifier of provably empty tiles keeps the scene's values and the staged tree
    std::shared_ptr<rtw::CullScene> cs;
    if (c->precision == RTW_F64) cs = std::make_shared<rtw::CullScene>();
    std::vector<unsigned char> blob = c->precision == RTW_F32
                                          ? rtw::stage_scene<float>(s, &tmp32, 0, leaf, light_leaf, grid)
                                          : rtw::stage_scene<double>(s, &tmp64, 0, leaf, light_leaf, grid, &cs->bvh);
    if (cs) rtw::cull_scene_init(s, cs.get());
    const rtw::SceneScale scale = c->precision == RTW_F32 ? rtw::scene_scale(s, tmp32) : rtw::scene_scale(s, tmp64);
    for (uint32_t k = 0; k < rtw_device_count(c); ++k) {   // multi-device: the same scene on every rank
        rtw_ctx* ck = rtw_device_ctx(c, k);
        rc = upload_scene(ck, blob, tmp32, tmp64, scale);
        ck->cull_scene = cs;
        ck->cull.st.drop();
        if (rc) {
            // no rank keeps a scene: a partial update must not render one image
            // from tiles of two scenes
            for (uint32_t q = 0; q < rtw_device_count(c); ++q) rtw_device_ctx(c, q)->has_scene = false;
            if (!c->peers.empty()) (void)hipSetDevice(c->device);
            return k ? fail(c, rc, ck->err) : rc;
        }
    }
    c->has_lambertian = false;
    for (uint32_t m = 0; m < s->n_materials; ++m) c->has_lambertian |= s->mat_type[m] == RTW_LAMBERTIAN;
    if (!c->peers.empty()) HIP_TRY(c, hipSetDevice(c->device));
    return RTW_OK;
}

uint32_t rtw_tile_size(void) { return rtw::kTile; }

uint32_t rtw_tiles_for_rank(uint32_t W, uint32_t H, uint32_t rank, uint32_t nranks) {
    return rtw::tiles_for_rank(W, H, rank, nranks);
}

int rtw_split_deal(const uint32_t* tile_cost, uint32_t W, uint32_t H, uint32_t nranks, uint32_t* tile_rank) {
    return rtw::split_deal(tile_cost, W, H, nranks, tile_rank);
}
}  // extern "C"

int apply_split(rtw_ctx* c, uint32_t W, uint32_t H, uint32_t nranks, const uint32_t* tile_rank,
                const uint32_t* tile_cost, bool automatic, const rtw_camera* cam) {
    SplitState& s = c->split;
    if (!tile_rank) {
        s.rank.clear();
        s.cost.clear();
        s.W = s.H = s.n = 0;
        s.automatic = false;
        return RTW_OK;
    }
    const uint64_t n = rtw::n_tiles_of(W, H);
    s.rank.assign(tile_rank, tile_rank + n);
    if (tile_cost) s.cost.assign(tile_cost, tile_cost + n);
    else s.cost.clear();
    s.W = W;
    s.H = H;
    s.n = nranks;
    ++s.serial;
    s.automatic = automatic;
    if (cam) s.cam = *cam;
    s.scene = c->scene_serial;
    return RTW_OK;
}

extern "C" {

int rtw_set_split(rtw_ctx* c, uint32_t W, uint32_t H, uint32_t nranks, const uint32_t* tile_rank,
                  const uint32_t* tile_cost) {
    if (!c) return RTW_E_INVALID;
    const int rc = rtw::check_split(W, H, nranks, tile_rank);
    if (rc) return fail(c, rc, "bad split: every tile needs a rank < nranks, and rank r exactly "
                               "rtw_tiles_for_rank(W, H, r, nranks) tiles");
    apply_split(c, W, H, nranks, tile_rank, tile_cost, false, nullptr);
    return on_peers(c, [&](rtw_ctx* pk) { return apply_split(pk, W, H, nranks, tile_rank, tile_cost, false, nullptr); });
}

int rtw_get_split(rtw_ctx* c, uint32_t W, uint32_t H, uint32_t nranks, uint32_t* tile_rank) {
    if (!c || nranks == 0) return RTW_E_INVALID;
    if (!c->split.active(W, H, nranks)) return 0;
    if (tile_rank) memcpy(tile_rank, c->split.rank.data(), c->split.rank.size() * sizeof(uint32_t));
    return c->split.automatic ? 2 : 1;
}

uint32_t rtw_culled_tiles(rtw_ctx* c) {
    if (!c) return 0;
    uint32_t n = 0;
    for (uint32_t k = 0; k < std::min(std::max(c->stats_ranks, 1u), rtw_device_count(c)); ++k) {
        const rtw_ctx* ck = rtw_device_ctx(c, k);
        if (ck && !ck->no_work) n += ck->last_culled;
    }
    return n;
}

int rtw_last_kernel(const rtw_ctx* c) {
    if (!c) return RTW_E_INVALID;
    return c->last_variant & 0xffff;
}

int rtw_get_stats_rank(rtw_ctx* c, uint32_t k, rtw_stats* out) {
    if (!c || !out) return RTW_E_INVALID;
    rtw_ctx* ck = rtw_device_ctx(c, k);
    if (!ck) return fail(c, RTW_E_INVALID, "no rank " + std::to_string(k));
    const int rc = get_stats_one(ck, out);
    if (k && rc) c->err = ck->err;
    (void)hipSetDevice(c->device);
    return rc;
}

}  // extern "C"

int get_stats_one(rtw_ctx* c, rtw_stats* out) {
    if (c->no_work) {   // a rank without a tile in the last multi-device render
        *out = rtw_stats{};
        out->chunk = 1;
        return RTW_OK;
    }
    if (c->n_renders == 0) return fail(c, RTW_E_INVALID, "no render yet");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->ev1));
    unsigned long long h[rtw::kCounters] = {};
    HIP_TRY(c, hipMemcpy(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last.segments = h[0] + c->cull_segments;   // (a culled sample: one segment that misses)
    c->last.lambertian = h[1];
    c->last.node_visits = h[2];
    // the brute-force sweep tests every sphere on every segment
    c->last.sphere_tests = c->last.accel == RTW_ACCEL_BVH ? h[3] : h[0] * (uint64_t)c->last_n_sph;
    c->last.kernel_ms = ms;
    c->last.panic_plane_uv = h[4];
    c->last.panic_no_lights = h[5];
    // the linear light loop tests every light of the list on every Lambertian
    // bounce (hittable_list.rs:408-412); the light grid / BVH walks count theirs
    c->last.light_tests = c->last_light_bvh ? h[7] : h[1] * (uint64_t)c->last_n_list;
    c->last.grid_cells = h[8];
    *out = c->last;
    if (h[5])
        return fail(c, RTW_E_NO_LIGHTS, std::to_string(h[5]) + " samples drew a light from an empty light list "
                                        "(the reference panics: HittableList shouldn't be empty, hittable_list.rs:417)");
    if (h[4])
        return fail(c, RTW_E_PANIC, std::to_string(h[4]) + " plane tests produced a non-finite UV "
                                    "(the reference panics in Plane::hit, plane.rs:66-69)");
    return RTW_OK;
}

extern "C" {

int rtw_get_timings(rtw_ctx* c, float* render_ms, float* total_ms, int max) {
    if (!c || max < 0) return RTW_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    const int n = (int)std::min<uint64_t>({(uint64_t)max, c->n_renders, (uint64_t)rtw_ctx::kRing});
    for (int k = 0; k < n; ++k) {
        hipEvent_t* ev = c->ring[(c->n_renders - n + k) % rtw_ctx::kRing];
        HIP_TRY(c, hipEventSynchronize(ev[2]));
        float a = 0.f, b = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&a, ev[0], ev[1]));
        HIP_TRY(c, hipEventElapsedTime(&b, ev[0], ev[2]));
        if (render_ms) render_ms[k] = a;
        if (total_ms) total_ms[k] = b;
    }
    return n;
}

}  // extern "C"
