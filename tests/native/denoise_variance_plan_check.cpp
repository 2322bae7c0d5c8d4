// denoise_variance_plan_check.cpp -- CPU check of the variance-guided denoiser's
// plan (host/denoise_variance_plan.cpp).  Built and run by
// tests/test_denoise_variance_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> \
//       denoise_variance_plan_check.cpp <csrc>/host/denoise_variance_plan.cpp -o denoise_variance_plan_check
// (the plan unit alone: it takes constants of denoise_plan.hpp, none of its functions)
//
// The schedule of sample (W, H, iterations): steps, grids, buffer sizes, sv2;
// every refusal of the parameters, the sizes and the device arrays (moments
// among them); tuning denoise_lds 0, 1 and 2: a step is staged exactly while
// (32 + 4 step) (8 + 4 step) 80 bytes fit 160 KiB -- up to step 4 -- and falls
// back to the direct form above that.
//
// `denoise_variance_plan_check kernels` only prints the launcher's kernel table
// (denoise_variance_kernels.hpp), one "svgf <name>" line each.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>

#include "denoise_variance_kernels.hpp"
#include "host/denoise_variance_plan.hpp"

static int g_wrong = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++g_wrong;                   \
            printf("WRONG: " __VA_ARGS__); \
            printf("\n");                \
        }                                \
    } while (0)

static rtw_denoise_variance_params defaults() {
    rtw_denoise_variance_params p;
    rtw::denoise_variance_params_default(&p);
    return p;
}

static void schedule() {
    const struct { uint32_t W, H, it; } cases[] = {{1, 1, 1}, {5, 3, 3}, {37, 19, 5}, {70, 45, 7}, {1200, 800, 5},
                                                   {65535, 65535, 16}, {32, 8, 1}, {33, 9, 2}};
    for (const auto& cs : cases)
        for (double sigma : {0.0, 1.0, 1.5, 2.0, 3.0})
            for (uint32_t lds : {0u, 1u, 2u}) {
                rtw_denoise_variance_params p = defaults();
                p.iterations = cs.it;
                p.sigma_var = sigma;
                const rtw::SvgfPlan pl = rtw::plan_denoise_variance(&p, cs.W, cs.H, false, 4, lds);
                CHECK(pl.err == RTW_OK, "%ux%u it %u: refused (%s)", cs.W, cs.H, cs.it, pl.err_text);
                if (pl.err) continue;
                const uint64_t px = (uint64_t)cs.W * cs.H;
                CHECK(pl.pixels == px && pl.iterations == cs.it, "%ux%u: pixels / iterations", cs.W, cs.H);
                CHECK(pl.sv2 == sigma * sigma, "sv2 %a for sigma %a", pl.sv2, sigma);
                CHECK((uint64_t)pl.blocks * 256 >= px && ((uint64_t)pl.blocks - 1) * 256 < px, "%ux%u: %u blocks", cs.W,
                      cs.H, pl.blocks);
                CHECK(pl.record_bytes == px * 32 && pl.var_bytes == px * 16 && pl.state_bytes == px * 160,
                      "%ux%u: state bytes", cs.W, cs.H);
                CHECK(pl.sums_bytes_f32 == px * 12 && pl.sums_bytes_f64 == px * 24 && pl.features_bytes == px * 64 &&
                          pl.moments_bytes == px * 16 && pl.counts_bytes == px * 4 && pl.out_bytes == px * 24,
                      "%ux%u: array bytes", cs.W, cs.H);
                uint32_t staged = 0;
                for (uint32_t k = 0; k < cs.it; ++k) {
                    const rtw::SvgfStep& s = pl.steps[k];
                    CHECK(s.step == 1u << k, "iteration %u: step %u", k, s.step);
                    CHECK(s.grid_x == (cs.W + 31) / 32 && s.grid_y == (cs.H + 7) / 8, "iteration %u: grid %u x %u", k,
                          s.grid_x, s.grid_y);
                    const size_t bytes = (32 + 4 * (size_t)s.step) * (8 + 4 * (size_t)s.step) * 80;
                    CHECK(rtw::svgf_lds_bytes(s.step) == bytes, "step %u: %zu LDS bytes", s.step,
                          rtw::svgf_lds_bytes(s.step));
                    const bool fits = bytes <= 160 * 1024;
                    const bool want = lds == 2 || (lds == 1 && s.step <= 2);   // the default: steps 1 and 2
                    CHECK(s.lds == (want && fits ? 1u : 0u), "denoise_lds %u step %u: staged %u", lds, s.step, s.lds);
                    CHECK(s.lds ? s.lds_bytes == bytes && s.lds_bytes <= 160 * 1024 : s.lds_bytes == 0,
                          "step %u: lds_bytes %zu", s.step, s.lds_bytes);
                    staged += s.lds;
                }
                CHECK(pl.lds_iterations == staged, "lds_iterations %u, counted %u", pl.lds_iterations, staged);
                if (lds == 0) CHECK(staged == 0, "denoise_lds 0 staged %u iterations", staged);
                if (lds == 1) CHECK(staged == (cs.it < 2 ? cs.it : 2), "denoise_lds 1 staged %u of %u", staged, cs.it);
                // the halo fits up to step 4 (48 x 24 pixels of 80 bytes), not step 8 (64 x 40: 200 KiB)
                if (lds == 2) CHECK(staged == (cs.it < 3 ? cs.it : 3), "denoise_lds 2 staged %u of %u", staged, cs.it);
            }
    CHECK(rtw::svgf_lds_bytes(1) == 34560 && rtw::svgf_lds_bytes(2) == 51200 && rtw::svgf_lds_bytes(4) == 92160 &&
              rtw::svgf_lds_bytes(4) <= 160 * 1024 && rtw::svgf_lds_bytes(8) == 204800 &&
              rtw::svgf_lds_bytes(8) > 160 * 1024,
          "LDS bytes of steps 1, 2, 4, 8");
    CHECK(rtw::kSvgfEps == ldexp(1.0, -40), "eps");
    // NULL parameters: the defaults
    const rtw::SvgfPlan d = rtw::plan_denoise_variance(nullptr, 8, 8, true, 0, 1);
    CHECK(d.err == RTW_OK && d.params.iterations == 5 && d.params.normal_power_log2 == 5 && d.params.sigma_var == 2.0 &&
              d.params.sigma_depth == 0.125 && d.params.demodulate == 1 && d.params.fill_nonfinite == 1 && d.sv2 == 4.0,
          "the defaults");
}

static void refusals() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto refused = [](const rtw_denoise_variance_params& p, uint32_t W, uint32_t H, bool counts, uint32_t spp) {
        const rtw::SvgfPlan pl = rtw::plan_denoise_variance(&p, W, H, counts, spp, 1);
        return pl.err == RTW_E_INVALID && pl.err_text[0];
    };
    rtw_denoise_variance_params p = defaults();
    CHECK(!refused(p, 8, 8, false, 1), "the defaults are refused");
    for (uint32_t it : {0u, 17u, 0xFFFFFFFFu}) { p = defaults(); p.iterations = it; CHECK(refused(p, 8, 8, false, 1), "iterations %u", it); }
    for (uint32_t it : {1u, 16u}) { p = defaults(); p.iterations = it; CHECK(!refused(p, 8, 8, false, 1), "iterations %u", it); }
    p = defaults(); p.normal_power_log2 = 11; CHECK(refused(p, 8, 8, false, 1), "normal_power_log2 11");
    p = defaults(); p.normal_power_log2 = 10; CHECK(!refused(p, 8, 8, false, 1), "normal_power_log2 10");
    p = defaults(); p.normal_power_log2 = 0; CHECK(!refused(p, 8, 8, false, 1), "normal_power_log2 0");
    for (double v : {-1.0, -0.5e-300, nan, inf, -inf}) { p = defaults(); p.sigma_var = v; CHECK(refused(p, 8, 8, false, 1), "sigma_var %g", v); }
    p = defaults(); p.sigma_var = 0.0; CHECK(!refused(p, 8, 8, false, 1), "sigma_var 0");
    for (double v : {0.0, -1.0, nan, inf, -inf}) { p = defaults(); p.sigma_depth = v; CHECK(refused(p, 8, 8, false, 1), "sigma_depth %g", v); }
    p = defaults(); p.demodulate = 2; CHECK(refused(p, 8, 8, false, 1), "demodulate 2");
    p = defaults(); p.fill_nonfinite = 2; CHECK(refused(p, 8, 8, false, 1), "fill_nonfinite 2");
    p = defaults();
    CHECK(refused(p, 8, 8, false, 0), "no counts and spp 0");
    CHECK(!refused(p, 8, 8, true, 0), "counts and spp 0");
    CHECK(refused(p, 65536, 8, false, 1) && refused(p, 8, 65536, false, 1), "width or height 2^16");
    CHECK(!refused(p, 65535, 1, false, 1) && !refused(p, 1, 65535, false, 1), "width or height 2^16 - 1");
    CHECK(!refused(p, 0, 8, false, 1), "an empty image");

    // the device arrays of a 10 x 6 image: 60 pixels
    const rtw::SvgfPlan pl = rtw::plan_denoise_variance(nullptr, 10, 6, true, 0, 1);
    const uintptr_t sums = 0x10000, feat = 0x20000, mom = 0x28000, cnt = 0x30000, out = 0x40000;
    auto arrays = [&](bool f32, uintptr_t s, size_t sb, uintptr_t f, size_t fb, uintptr_t m, size_t mb, uintptr_t c,
                      size_t cb, uintptr_t o, size_t ob) {
        return rtw::svgf_check_arrays(pl, f32, s, sb, f, fb, m, mb, c, cb, o, ob)[0] != 0;
    };
    CHECK(!arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, out, 1440), "exact f64 arrays refused");
    CHECK(!arrays(true, sums, 720, feat, 3840, mom, 960, 0, 0, out, 1440), "exact f32 arrays without counts refused");
    CHECK(arrays(false, sums, 1439, feat, 3840, mom, 960, cnt, 240, out, 1440), "short f64 sums");
    CHECK(arrays(false, sums, 720, feat, 3840, mom, 960, cnt, 240, out, 1440), "f32-sized sums for f64");
    CHECK(arrays(true, sums, 719, feat, 3840, mom, 960, cnt, 240, out, 1440), "short f32 sums");
    CHECK(arrays(false, sums, 1440, feat, 3839, mom, 960, cnt, 240, out, 1440), "short features");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 959, cnt, 240, out, 1440), "short moments");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 0, cnt, 240, out, 1440), "moments of no bytes");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 239, out, 1440), "short counts");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, out, 1439), "short out");
    CHECK(arrays(false, sums + 8, 1440, feat, 3840, mom, 960, cnt, 240, out, 1440), "misaligned sums");
    CHECK(arrays(false, sums, 1440, feat + 8, 3840, mom, 960, cnt, 240, out, 1440), "misaligned features");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom + 8, 968, cnt, 240, out, 1440), "misaligned moments");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 960, cnt + 4, 240, out, 1440), "misaligned counts");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, out + 8, 1448), "misaligned out");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, sums, 1440), "out is sums");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, sums + 1424, 1440), "out overlaps the end of sums");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, feat - 16, 1440), "out overlaps the start of features");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, mom, 1440), "out is moments");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, mom + 944, 1440), "out overlaps the end of moments");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, mom - 1424, 1440), "out overlaps the start of moments");
    CHECK(arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, cnt + 224, 1440), "out overlaps counts");
    CHECK(!arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, mom + 960, 1440), "out right after moments refused");
    CHECK(!arrays(false, sums, 1440, feat, 3840, mom, 960, cnt, 240, sums + 1440, 1440), "out right after sums refused");
    // an f32 image next to out: only its 720 bytes count
    CHECK(!arrays(true, sums, 1440, feat, 3840, mom, 960, cnt, 240, sums + 720, 1440), "out after f32 sums refused");
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "kernels")) {
        for (int k = 0; k < rtw::kSvgfKernels; ++k) printf("svgf %s\n", rtw::kSvgfKernelNames[k]);
        return 0;
    }
    schedule();
    refusals();
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
