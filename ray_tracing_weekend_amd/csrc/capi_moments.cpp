// capi_moments.cpp -- the per-pixel luminance moments of the C-ABI
// (include/rtw.h): rtw_render_window_moments and its device form, a sample
// window whose fold also keeps {S1, S2}, and rtw_adaptive_moments, the {S1, S2}
// the last adaptive render left on the context.  A moments window is the passes
// of an adaptive render without the vote: every tile, one sample per item,
// sub-windows under the chunk-sum budget (host/render_adaptive.hpp), each
// followed by fold_moments_kernel on the caller's image-order arrays.
#include <algorithm>

#include "capi_ctx.hpp"
#include "host/render_adaptive.hpp"
#include "moments_kernels.hpp"

namespace {

// what both window forms refuse before anything else
int check_window_moments(rtw_ctx* c, const rtw_camera* cam, uint32_t first, uint32_t n, bool buffers) {
    if (!c || !cam || !buffers) return fail(c, RTW_E_INVALID, "bad argument");
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "the moments of a multi-device context");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    if ((uint64_t)first + n > 0xFFFFFFFFull) return fail(c, RTW_E_INVALID, "first_sample + n_samples overflows");
    if (c->knobs.chunk > 1)
        return fail(c, RTW_E_INVALID, "a moments window renders one sample per item: rtw_set_chunk above 1");
    return check_image_size(c, cam);
}

// the sub-windows of [first, first + n) on `stream`: render, fold
template <typename R>
int window_moments_t(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t first, uint32_t n, double* d_sums,
                     double* d_moments, hipStream_t stream) {
    const uint32_t W = cam->image_width, H = cam->image_height;
    const uint32_t nt = (uint32_t)rtw::n_tiles_of(W, H);
    const uint32_t cap = rtw::adaptive_sub_samples<R>(c->knobs, nt, device_total(c));
    const uint32_t end = first + n;
    c->stats_ranks = 1;
    for (uint32_t s = first; s < end;) {
        const uint32_t m = std::min(cap, end - s);
        rtw::Pass ps = rtw::adaptive_pass(s, m, nullptr, nt);
        ps.begin = s == first;   // the stats are the window's
        const int rc = render_pass(c, cam, seed, 0, 1, nullptr, stream, ps);
        if (rc) return rc;
        rtw::MomentsFold f{};
        f.partial = c->d_partial;
        f.n_chunks = cam->max_depth ? m : 0;   // depth 0: every sample is 0
        f.n_tiles = nt;
        f.sums = d_sums;
        f.moments = d_moments;
        f.first = s;
        f.W = W;
        f.H = H;
        if (rtw::launch_fold_moments(sizeof(R) == 8, f, stream))
            return fail(c, RTW_E_DEVICE, std::string("moments fold launch failed: ") + hipGetErrorString(hipGetLastError()));
        s += m;
    }
    HIP_TRY(c, hipEventRecord(c->ev1, stream));   // the stats' time covers the last fold too
    c->last.chunk = 1;
    return RTW_OK;
}

}  // namespace

extern "C" {

int rtw_render_window_moments_device(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t first_sample,
                                     uint32_t n_samples, double* d_sums, size_t sums_bytes, double* d_moments,
                                     size_t moments_bytes, void* stream) {
    if (const int rc = check_window_moments(c, cam, first_sample, n_samples, true)) return rc;
    const size_t px = (size_t)cam->image_width * cam->image_height;
    if (px == 0 || n_samples == 0) return RTW_OK;
    if (!d_sums || !d_moments) return fail(c, RTW_E_INVALID, "d_sums or d_moments is NULL");
    if (sums_bytes < px * 3 * sizeof(double) || moments_bytes < px * 2 * sizeof(double))
        return fail(c, RTW_E_INVALID, "d_sums is smaller than H*W*3 doubles or d_moments than H*W*2");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    return by_precision(c, [&](auto r) {
        return window_moments_t<decltype(r)>(c, cam, seed, first_sample, n_samples, d_sums, d_moments, s);
    });
}

int rtw_render_window_moments(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t first_sample,
                              uint32_t n_samples, double* sums, double* moments, rtw_stats* stats) {
    if (const int rc = check_window_moments(c, cam, first_sample, n_samples, sums && moments)) return rc;
    const size_t px = (size_t)cam->image_width * cam->image_height;
    if (px == 0 || n_samples == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure(c, &c->d_moments_img, &c->moments_img_cap, px * 5 * sizeof(double));
    if (rc) return rc;
    double* d_sums = reinterpret_cast<double*>(c->d_moments_img);
    double* d_moments = d_sums + px * 3;
    if (first_sample) {
        HIP_TRY(c, hipMemcpyAsync(d_sums, sums, px * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_moments, moments, px * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    rc = rtw_render_window_moments_device(c, cam, seed, first_sample, n_samples, d_sums, px * 3 * sizeof(double),
                                          d_moments, px * 2 * sizeof(double), nullptr);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the uploads read the caller's arrays)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(sums, d_sums, px * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(moments, d_moments, px * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return fetch_stats(c, stats);
}

int rtw_adaptive_moments_device(rtw_ctx* c, double* d_moments, size_t bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "the moments of a multi-device context");
    if (!c->adapt_done || !c->d_adapt)
        return fail(c, RTW_E_INVALID, "no adaptive render on this context since rtw_set_scene");
    const uint32_t W = c->adapt_w, H = c->adapt_h;
    const size_t px = (size_t)W * H;
    if (px == 0) return RTW_OK;
    if (!d_moments) return fail(c, RTW_E_INVALID, "d_moments is NULL");
    if (bytes < px * 2 * sizeof(double)) return fail(c, RTW_E_INVALID, "d_moments is smaller than H*W*2 doubles");
    HIP_TRY(c, hipSetDevice(c->device));
    // (capi_adaptive.cpp adaptive_buffers: the colour sums of every tile, then {S1, S2})
    const double* s12 = reinterpret_cast<const double*>(c->d_adapt) + rtw::n_tiles_of(W, H) * 64 * 3;
    if (rtw::launch_unpack_moments(s12, W, H, d_moments, resolve_stream(c, stream)))
        return fail(c, RTW_E_DEVICE, std::string("moments unpack launch failed: ") + hipGetErrorString(hipGetLastError()));
    return RTW_OK;
}

int rtw_adaptive_moments(rtw_ctx* c, double* moments) {
    if (!c) return RTW_E_INVALID;
    if (!moments) return fail(c, RTW_E_INVALID, "moments is NULL");
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "the moments of a multi-device context");
    if (!c->adapt_done) return fail(c, RTW_E_INVALID, "no adaptive render on this context since rtw_set_scene");
    const size_t bytes = (size_t)c->adapt_w * c->adapt_h * 2 * sizeof(double);
    if (bytes == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure(c, &c->d_moments_img, &c->moments_img_cap, bytes);
    if (rc) return rc;
    rc = rtw_adaptive_moments_device(c, reinterpret_cast<double*>(c->d_moments_img), bytes, nullptr);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(moments, c->d_moments_img, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

}  // extern "C"
