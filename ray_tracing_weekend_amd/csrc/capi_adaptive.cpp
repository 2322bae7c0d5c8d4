// capi_adaptive.cpp -- adaptive sampling (rtw_render_adaptive,
// rtw_render_adaptive_device): the passes of host/render_adaptive.hpp as
// adaptive passes of capi_render.cpp's render_pass, each followed by the fold
// with the stop vote and the compaction of the tiles that go on.
#include <algorithm>

#include "capi_ctx.hpp"
#include "host/render_adaptive.hpp"

namespace {

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

// rtw_render_adaptive_device, its arguments checked.  Per pass: the render
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
            rc = render_pass(c, cam, seed, 0, 1, nullptr, stream, rtw::adaptive_pass(s, n, list, n_active));
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

// what both forms refuse before anything else (buffers: the form's own pointers are given)
int check_adaptive(rtw_ctx* c, const rtw_camera* cam, bool buffers, uint32_t min_samples, uint32_t max_samples,
                   uint32_t window, double tolerance) {
    if (!c || !cam || !buffers) return fail(c, RTW_E_INVALID, "bad argument");
    if (c->multi) return fail(c, RTW_E_UNSUPPORTED, "adaptive sampling of a multi-device context");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    if (const char* why = rtw::adaptive_check(min_samples, max_samples, window, tolerance, c->knobs.chunk))
        return fail(c, RTW_E_INVALID, why);
    return check_image_size(c, cam);
}

}  // namespace

extern "C" {

int rtw_render_adaptive_device(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t min_samples,
                               uint32_t max_samples, uint32_t window, double tolerance, double* d_sums,
                               size_t sums_bytes, uint32_t* d_counts, size_t counts_bytes, void* stream) {
    if (const int rc = check_adaptive(c, cam, true, min_samples, max_samples, window, tolerance)) return rc;
    const size_t px = (size_t)cam->image_width * cam->image_height;
    if (px == 0) return RTW_OK;
    if (!d_sums || !d_counts) return fail(c, RTW_E_INVALID, "d_sums or d_counts is NULL");
    if (sums_bytes < px * 3 * sizeof(double) || counts_bytes < px * sizeof(uint32_t))
        return fail(c, RTW_E_INVALID, "d_sums is smaller than H*W*3 doubles or d_counts than H*W");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    c->stats_ranks = 1;
    return by_precision(c, [&](auto r) {
        return render_adaptive_t<decltype(r)>(c, cam, seed, min_samples, max_samples, window, tolerance, d_sums,
                                              d_counts, s);
    });
}

int rtw_render_adaptive(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t min_samples, uint32_t max_samples,
                        uint32_t window, double tolerance, double* sums, uint32_t* counts, rtw_stats* stats) {
    if (const int rc = check_adaptive(c, cam, sums && counts, min_samples, max_samples, window, tolerance)) return rc;
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
    return fetch_stats(c, stats);
}

}  // extern "C"
