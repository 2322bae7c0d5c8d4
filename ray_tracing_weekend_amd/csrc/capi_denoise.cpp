// capi_denoise.cpp -- the denoiser of the C-ABI (include/rtw.h): rtw_denoise,
// its device form and rtw_get_denoise_stats.  A denoise is plan
// (host/denoise_plan.hpp) -> params -> launches -> bookkeeping, on the denoise
// state's record arrays, counters and events: nothing of the render's, of a ray
// query's or of the feature pass's is touched.
#include <new>
#include <string>

#include "capi_ctx.hpp"
#include "denoise_kernels.hpp"
#include "host/denoise_plan.hpp"

void destroy_denoise(rtw_ctx* c) {
    DenoiseState* d = c->denoise;
    if (!d) return;
    if (d->d_records) (void)hipFree(d->d_records);
    if (d->d_counters) (void)hipFree(d->d_counters);
    if (d->d_sums) (void)hipFree(d->d_sums);
    if (d->d_features) (void)hipFree(d->d_features);
    if (d->d_counts) (void)hipFree(d->d_counts);
    if (d->d_moments) (void)hipFree(d->d_moments);
    if (d->d_out) (void)hipFree(d->d_out);
    if (d->ev0) (void)hipEventDestroy(d->ev0);
    if (d->ev1) (void)hipEventDestroy(d->ev1);
    delete d;
    c->denoise = nullptr;
}

int denoise_state(rtw_ctx* c) {
    if (c->denoise) return RTW_OK;
    DenoiseState* d = new (std::nothrow) DenoiseState();
    if (!d) return fail(c, RTW_E_DEVICE, "out of memory");
    c->denoise = d;
    HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&d->d_counters), 2 * sizeof(unsigned long long)));
    HIP_TRY(c, hipEventCreate(&d->ev0));
    HIP_TRY(c, hipEventCreate(&d->ev1));
    return RTW_OK;
}

namespace {

// what both forms refuse before any device call; the plan of a call that can run
int denoise_checks(rtw_ctx* c, const void* sums, const double* features, const uint32_t* counts, uint32_t spp,
                   uint32_t width, uint32_t height, const rtw_denoise_params* params, const double* out,
                   rtw::DenoisePlan* pl) {
    if (!sums) return fail(c, RTW_E_INVALID, "sums is NULL");
    if (!features) return fail(c, RTW_E_INVALID, "features is NULL");
    if (!out) return fail(c, RTW_E_INVALID, "out is NULL");
    *pl = rtw::plan_denoise(params, width, height, counts != nullptr, spp, c->knobs.denoise_lds);
    if (pl->err) return fail(c, pl->err, pl->err_text);
    return RTW_OK;
}

// the launches of a planned denoise of device arrays, on `stream`
int denoise_run(rtw_ctx* c, const rtw::DenoisePlan& pl, const void* d_sums, bool sums_f32, const double* d_features,
                const uint32_t* d_counts, uint32_t spp, uint32_t width, uint32_t height, double* d_out,
                hipStream_t stream) {
    int rc = denoise_state(c);
    if (rc) return rc;
    DenoiseState* d = c->denoise;
    rc = ensure(c, &d->d_records, &d->records_cap, pl.state_bytes);
    if (rc) return rc;
    unsigned char* base = reinterpret_cast<unsigned char*>(d->d_records);
    double2* guide = reinterpret_cast<double2*>(base);
    double2* albedo = reinterpret_cast<double2*>(base + pl.record_bytes);
    double2* colour[2] = {reinterpret_cast<double2*>(base + 2 * pl.record_bytes),
                          reinterpret_cast<double2*>(base + 3 * pl.record_bytes)};
    HIP_TRY(c, hipMemsetAsync(d->d_counters, 0, 2 * sizeof(unsigned long long), stream));
    HIP_TRY(c, hipEventRecord(d->ev0, stream));
    rtw::DenoisePrepare pp{};
    pp.sums = d_sums;
    pp.features = d_features;
    pp.counts = d_counts;
    pp.spp = spp;
    pp.demodulate = pl.params.demodulate;
    pp.pixels = pl.pixels;
    pp.guide = guide;
    pp.albedo = albedo;
    pp.colour = colour[0];
    int ran = rtw::launch_denoise_prepare(sums_f32, pp, pl.blocks, stream);
    for (uint32_t k = 0; k < pl.iterations && ran == 0; ++k) {
        rtw::DenoiseAtrous pa{};
        pa.guide = guide;
        pa.src = colour[k & 1];
        pa.dst = colour[(k + 1) & 1];
        pa.W = width;
        pa.H = height;
        pa.step = pl.steps[k].step;
        pa.m = pl.params.normal_power_log2;
        pa.colour_on = pl.params.sigma_colour != 0.0 ? 1u : 0u;
        pa.fill = pl.params.fill_nonfinite;
        pa.sc2 = pl.steps[k].sc2;
        pa.sigma_depth = pl.params.sigma_depth;
        ran = rtw::launch_denoise_atrous(pa, pl.steps[k], stream);
    }
    if (ran == 0) {
        rtw::DenoiseFinish pf{};
        pf.albedo = albedo;
        pf.colour = colour[pl.iterations & 1];
        pf.out = d_out;
        pf.pixels = pl.pixels;
        pf.counters = d->d_counters;
        ran = rtw::launch_denoise_finish(pf, pl.blocks, stream);
    }
    if (ran)
        return fail(c, RTW_E_DEVICE,
                    std::string("denoise kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    HIP_TRY(c, hipEventRecord(d->ev1, stream));
    d->last = rtw_denoise_stats{};
    d->last.iterations = pl.iterations;
    d->last.lds_iterations = pl.lds_iterations;
    d->any = true;
    return RTW_OK;
}

}  // namespace

extern "C" {

void rtw_denoise_params_default(rtw_denoise_params* out) { rtw::denoise_params_default(out); }

int rtw_denoise_device(rtw_ctx* c, const void* d_sums, int sums_precision, size_t sums_bytes, const double* d_features,
                       size_t features_bytes, const uint32_t* d_counts, size_t counts_bytes, uint32_t spp,
                       uint32_t width, uint32_t height, const rtw_denoise_params* params, double* d_out,
                       size_t out_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    if (sums_precision != RTW_F32 && sums_precision != RTW_F64)
        return fail(c, RTW_E_INVALID, "sums_precision is RTW_F32 or RTW_F64");
    rtw::DenoisePlan pl;
    int rc = denoise_checks(c, d_sums, d_features, d_counts, spp, width, height, params, d_out, &pl);
    if (rc) return rc;
    const char* wrong = rtw::denoise_check_arrays(
        pl, sums_precision == RTW_F32, reinterpret_cast<uintptr_t>(d_sums), sums_bytes,
        reinterpret_cast<uintptr_t>(d_features), features_bytes, reinterpret_cast<uintptr_t>(d_counts), counts_bytes,
        reinterpret_cast<uintptr_t>(d_out), out_bytes);
    if (wrong[0]) return fail(c, RTW_E_INVALID, wrong);
    if (pl.pixels == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    return denoise_run(c, pl, d_sums, sums_precision == RTW_F32, d_features, d_counts, spp, width, height, d_out,
                       resolve_stream(c, stream));
}

int rtw_denoise(rtw_ctx* c, const double* sums, const double* features, const uint32_t* counts, uint32_t spp,
                uint32_t width, uint32_t height, const rtw_denoise_params* params, double* out) {
    if (!c) return RTW_E_INVALID;
    rtw::DenoisePlan pl;
    int rc = denoise_checks(c, sums, features, counts, spp, width, height, params, out, &pl);
    if (rc) return rc;
    if (pl.pixels == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = denoise_state(c);
    if (rc) return rc;
    DenoiseState* d = c->denoise;
    rc = ensure(c, &d->d_sums, &d->sums_cap, pl.sums_bytes_f64);
    if (!rc) rc = ensure(c, &d->d_features, &d->features_cap, pl.features_bytes);
    if (!rc && counts) rc = ensure(c, &d->d_counts, &d->counts_cap, pl.counts_bytes);
    if (!rc) rc = ensure(c, &d->d_out, &d->out_cap, pl.out_bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(d->d_sums, sums, pl.sums_bytes_f64, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d->d_features, features, pl.features_bytes, hipMemcpyHostToDevice, c->stream));
    if (counts) HIP_TRY(c, hipMemcpyAsync(d->d_counts, counts, pl.counts_bytes, hipMemcpyHostToDevice, c->stream));
    rc = denoise_run(c, pl, d->d_sums, false, reinterpret_cast<const double*>(d->d_features),
                     counts ? reinterpret_cast<const uint32_t*>(d->d_counts) : nullptr, spp, width, height,
                     reinterpret_cast<double*>(d->d_out), c->stream);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the uploads read the caller's arrays)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(out, d->d_out, pl.out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

int rtw_get_denoise_stats(rtw_ctx* c, rtw_denoise_stats* out) {
    if (!c || !out) return fail(c, RTW_E_INVALID, "bad argument");
    DenoiseState* d = c->denoise;
    if (!d || !d->any) return fail(c, RTW_E_INVALID, "no denoise yet");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(d->ev1));
    unsigned long long h[2] = {};
    HIP_TRY(c, hipMemcpy(h, d->d_counters, sizeof h, hipMemcpyDeviceToHost));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, d->ev0, d->ev1));
    d->last.filled = h[0];
    d->last.left_nonfinite = h[1];
    d->last.kernel_ms = ms;
    *out = d->last;
    return RTW_OK;
}

}  // extern "C"
