// capi_denoise_variance.cpp -- the variance-guided denoiser of the C-ABI
// (include/rtw.h): rtw_denoise_variance and its device form.  As rtw_denoise, a
// call is plan (host/denoise_variance_plan.hpp) -> params -> launches ->
// bookkeeping on the denoise state (capi_denoise.cpp) -- its record arrays,
// counters and events, so rtw_get_denoise_stats reports the last denoise of
// either filter: nothing of the render's, of a ray query's or of the feature
// pass's is touched.
#include <string>

#include "capi_ctx.hpp"
#include "denoise_kernels.hpp"
#include "denoise_variance_kernels.hpp"
#include "host/denoise_variance_plan.hpp"

namespace {

// what both forms refuse before any device call; the plan of a call that can run
int svgf_checks(rtw_ctx* c, const void* sums, const double* features, const double* moments, const uint32_t* counts,
                uint32_t spp, uint32_t width, uint32_t height, const rtw_denoise_variance_params* params,
                const double* out, rtw::SvgfPlan* pl) {
    if (!sums) return fail(c, RTW_E_INVALID, "sums is NULL");
    if (!features) return fail(c, RTW_E_INVALID, "features is NULL");
    if (!moments) return fail(c, RTW_E_INVALID, "moments is NULL");
    if (!out) return fail(c, RTW_E_INVALID, "out is NULL");
    *pl = rtw::plan_denoise_variance(params, width, height, counts != nullptr, spp, c->knobs.denoise_lds);
    if (pl->err) return fail(c, pl->err, pl->err_text);
    return RTW_OK;
}

// the launches of a planned denoise of device arrays, on `stream`
int svgf_run(rtw_ctx* c, const rtw::SvgfPlan& pl, const void* d_sums, bool sums_f32, const double* d_features,
             const double* d_moments, const uint32_t* d_counts, uint32_t spp, uint32_t width, uint32_t height,
             double* d_out, hipStream_t stream) {
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
    double2* var[2] = {reinterpret_cast<double2*>(base + 4 * pl.record_bytes),
                       reinterpret_cast<double2*>(base + 4 * pl.record_bytes + pl.var_bytes)};
    HIP_TRY(c, hipMemsetAsync(d->d_counters, 0, 2 * sizeof(unsigned long long), stream));
    HIP_TRY(c, hipEventRecord(d->ev0, stream));
    rtw::SvgfPrepare pp{};
    pp.sums = d_sums;
    pp.features = d_features;
    pp.moments = reinterpret_cast<const double2*>(d_moments);
    pp.counts = d_counts;
    pp.spp = spp;
    pp.demodulate = pl.params.demodulate;
    pp.pixels = pl.pixels;
    pp.guide = guide;
    pp.albedo = albedo;
    pp.colour = colour[0];
    pp.var = var[0];
    int ran = rtw::launch_svgf_prepare(sums_f32, pp, pl.blocks, stream);
    for (uint32_t k = 0; k < pl.iterations && ran == 0; ++k) {
        rtw::SvgfAtrous pa{};
        pa.guide = guide;
        pa.src = colour[k & 1];
        pa.var_src = var[k & 1];
        pa.dst = colour[(k + 1) & 1];
        pa.var_dst = var[(k + 1) & 1];
        pa.W = width;
        pa.H = height;
        pa.step = pl.steps[k].step;
        pa.m = pl.params.normal_power_log2;
        pa.fill = pl.params.fill_nonfinite;
        pa.sv2 = pl.sv2;
        pa.eps = rtw::kSvgfEps;
        pa.sigma_depth = pl.params.sigma_depth;
        ran = rtw::launch_svgf_atrous(pa, pl.steps[k], stream);
    }
    if (ran == 0) {
        // rtw_denoise's finish, as it is: its inputs are the same records
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
                    std::string("variance denoise kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    HIP_TRY(c, hipEventRecord(d->ev1, stream));
    d->last = rtw_denoise_stats{};
    d->last.iterations = pl.iterations;
    d->last.lds_iterations = pl.lds_iterations;
    d->any = true;
    return RTW_OK;
}

}  // namespace

extern "C" {

void rtw_denoise_variance_params_default(rtw_denoise_variance_params* out) {
    rtw::denoise_variance_params_default(out);
}

int rtw_denoise_variance_device(rtw_ctx* c, const void* d_sums, int sums_precision, size_t sums_bytes,
                                const double* d_features, size_t features_bytes, const double* d_moments,
                                size_t moments_bytes, const uint32_t* d_counts, size_t counts_bytes, uint32_t spp,
                                uint32_t width, uint32_t height, const rtw_denoise_variance_params* params,
                                double* d_out, size_t out_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    if (sums_precision != RTW_F32 && sums_precision != RTW_F64)
        return fail(c, RTW_E_INVALID, "sums_precision is RTW_F32 or RTW_F64");
    rtw::SvgfPlan pl;
    int rc = svgf_checks(c, d_sums, d_features, d_moments, d_counts, spp, width, height, params, d_out, &pl);
    if (rc) return rc;
    const char* wrong = rtw::svgf_check_arrays(
        pl, sums_precision == RTW_F32, reinterpret_cast<uintptr_t>(d_sums), sums_bytes,
        reinterpret_cast<uintptr_t>(d_features), features_bytes, reinterpret_cast<uintptr_t>(d_moments), moments_bytes,
        reinterpret_cast<uintptr_t>(d_counts), counts_bytes, reinterpret_cast<uintptr_t>(d_out), out_bytes);
    if (wrong[0]) return fail(c, RTW_E_INVALID, wrong);
    if (pl.pixels == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    return svgf_run(c, pl, d_sums, sums_precision == RTW_F32, d_features, d_moments, d_counts, spp, width, height,
                    d_out, resolve_stream(c, stream));
}

int rtw_denoise_variance(rtw_ctx* c, const double* sums, const double* features, const double* moments,
                         const uint32_t* counts, uint32_t spp, uint32_t width, uint32_t height,
                         const rtw_denoise_variance_params* params, double* out) {
    if (!c) return RTW_E_INVALID;
    rtw::SvgfPlan pl;
    int rc = svgf_checks(c, sums, features, moments, counts, spp, width, height, params, out, &pl);
    if (rc) return rc;
    if (pl.pixels == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = denoise_state(c);
    if (rc) return rc;
    DenoiseState* d = c->denoise;
    rc = ensure(c, &d->d_sums, &d->sums_cap, pl.sums_bytes_f64);
    if (!rc) rc = ensure(c, &d->d_features, &d->features_cap, pl.features_bytes);
    if (!rc) rc = ensure(c, &d->d_moments, &d->moments_cap, pl.moments_bytes);
    if (!rc && counts) rc = ensure(c, &d->d_counts, &d->counts_cap, pl.counts_bytes);
    if (!rc) rc = ensure(c, &d->d_out, &d->out_cap, pl.out_bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(d->d_sums, sums, pl.sums_bytes_f64, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d->d_features, features, pl.features_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d->d_moments, moments, pl.moments_bytes, hipMemcpyHostToDevice, c->stream));
    if (counts) HIP_TRY(c, hipMemcpyAsync(d->d_counts, counts, pl.counts_bytes, hipMemcpyHostToDevice, c->stream));
    rc = svgf_run(c, pl, d->d_sums, false, reinterpret_cast<const double*>(d->d_features),
                  reinterpret_cast<const double*>(d->d_moments),
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

}  // extern "C"
