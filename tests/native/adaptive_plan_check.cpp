// adaptive_plan_check.cpp -- CPU check of host/render_adaptive.hpp: where the
// passes of an adaptive render end, how a pass is cut into sub-passes under
// the chunk-sum budget, the argument check, and the stop rule on hand cases.
// Every rule case is also printed ("RULE S1 S2 n tolerance settled", the
// doubles as hex floats), and every pass plan ("ENDS min max window ends..."),
// for the numpy restatement of
// tests/test_adaptive_plan_host.py, which builds and runs this:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> \
//       adaptive_plan_check.cpp -o adaptive_plan_check
#include <math.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "host/render_adaptive.hpp"

static int g_wrong = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++g_wrong;                   \
            printf("WRONG: " __VA_ARGS__); \
            printf("\n");                \
        }                                \
    } while (0)

static void check_bounds(uint32_t mn, uint32_t win, uint32_t mx, const std::vector<uint32_t>& want) {
    const uint32_t n = rtw::adaptive_passes(mn, mx, win);
    printf("ENDS %u %u %u", mn, mx, win);
    for (uint32_t k = 0; k < n && k < 64; ++k) printf(" %u", rtw::adaptive_pass_end(mn, mx, win, k));
    printf("\n");
    CHECK(n == want.size(), "(%u, %u, %u): %u passes, expected %zu", mn, win, mx, n, want.size());
    uint32_t before = 0;
    for (uint32_t k = 0; k < n && k < want.size(); ++k) {
        const uint32_t e = rtw::adaptive_pass_end(mn, mx, win, k);
        CHECK(e == want[k], "(%u, %u, %u): pass %u ends at %u, expected %u", mn, win, mx, k, e, want[k]);
        CHECK(e > before, "(%u, %u, %u): pass %u is empty", mn, win, mx, k);
        before = e;
    }
    CHECK(before == mx, "(%u, %u, %u): the last pass ends at %u", mn, win, mx, before);
}

// the sub-passes of [first, end) for `tiles` active tiles cover it in order, each within the budget
template <typename R>
static void check_sub(size_t partial_max, size_t dev_total, uint32_t tiles, uint32_t first, uint32_t end,
                      uint32_t want_cap) {
    rtw::RenderKnobs k;
    k.partial_max = partial_max;
    const uint32_t cap = rtw::adaptive_sub_samples<R>(k, tiles, dev_total);
    CHECK(cap == want_cap, "sizeof %zu budget %zu / %zu tiles %u: %u samples per sub-pass, expected %u", sizeof(R),
          partial_max, dev_total, tiles, cap, want_cap);
    if (cap == 0) return;
    size_t budget = partial_max;
    if (dev_total && dev_total / 2 < budget) budget = dev_total / 2;
    uint32_t s = first, subs = 0;
    while (s < end) {
        const uint32_t n = std::min(cap, end - s);
        const size_t bytes = (size_t)n * tiles * 64 * 3 * sizeof(R);
        CHECK(bytes <= budget || n == 1, "a sub-pass of %u samples takes %zu bytes of %zu", n, bytes, budget);
        s += n;
        ++subs;
    }
    CHECK(s == end && subs == ((uint64_t)(end - first) + cap - 1) / cap, "sub-passes cover [%u, %u) in %u steps", first, end, subs);
}

static void rule(double s1, double s2, uint32_t n, double tol, int want, const char* what) {
    const bool got = rtw::adaptive_settled(s1, s2, n, tol);
    printf("RULE %a %a %u %a %d\n", s1, s2, n, tol, got ? 1 : 0);
    if (want >= 0) CHECK((int)got == want, "%s: settled %d, expected %d", what, (int)got, want);
}

int main() {
    check_bounds(4, 4, 32, {4, 8, 12, 16, 20, 24, 28, 32});
    check_bounds(2, 1, 2, {2});
    check_bounds(5, 7, 20, {5, 12, 19, 20});
    check_bounds(4, 4, 4, {4});
    check_bounds(2, 0xFFFFFFFFu, 0xFFFFFFFFu, {2, 0xFFFFFFFFu});   // no overflow of min + k * window
    check_bounds(0xFFFFFFF0u, 8, 0xFFFFFFFFu, {0xFFFFFFF0u, 0xFFFFFFF8u, 0xFFFFFFFFu});

    // sub-passes: 15 tiles of f64 chunk sums are 23040 bytes per sample
    check_sub<double>(23040 * 3 + 100, 0, 15, 4, 12, 3);      // 8 samples in 3 + 3 + 2
    check_sub<double>(23040 * 8, 0, 15, 4, 12, 8);            // exactly one sub-pass
    check_sub<double>(1, 0, 15, 0, 4, 1);                     // a budget below one sample: one at a time
    check_sub<float>(23040 * 3 + 100, 0, 15, 4, 12, 6);       // f32 sums are half the size
    check_sub<double>((size_t)128 << 30, 23040 * 8, 15, 0, 9, 4);   // half the device's memory binds
    check_sub<double>((size_t)128 << 30, 0, 0, 0, 4, 0xFFFFFFFFu);  // no tiles: no division by zero

    // the argument check
    CHECK(rtw::adaptive_check(4, 32, 4, 0.125, 0) == nullptr, "(4, 32, 4, 0.125) is rejected");
    CHECK(rtw::adaptive_check(2, 2, 1, 0.0, 1) == nullptr, "(2, 2, 1, 0) at an explicit chunk 1 is rejected");
    CHECK(rtw::adaptive_check(1, 32, 4, 0.125, 0) != nullptr, "min_samples 1 is accepted");
    CHECK(rtw::adaptive_check(0, 32, 4, 0.125, 0) != nullptr, "min_samples 0 is accepted");
    CHECK(rtw::adaptive_check(8, 7, 4, 0.125, 0) != nullptr, "max_samples < min_samples is accepted");
    CHECK(rtw::adaptive_check(4, 32, 0, 0.125, 0) != nullptr, "window 0 is accepted");
    CHECK(rtw::adaptive_check(4, 32, 4, -0.125, 0) != nullptr, "a negative tolerance is accepted");
    CHECK(rtw::adaptive_check(4, 32, 4, (double)NAN, 0) != nullptr, "a NaN tolerance is accepted");
    CHECK(rtw::adaptive_check(4, 32, 4, (double)INFINITY, 0) != nullptr, "an infinite tolerance is accepted");
    CHECK(rtw::adaptive_check(4, 32, 4, 0.125, 2) != nullptr, "an explicit chunk 2 is accepted");

    // the luminance: three products and two sums, each rounded
    {
        const double r = 0.3, g = 0.7, b = 0.9;
        const double yr = 0.2126 * r, yg = 0.7152 * g, yb = 0.0722 * b;
        const double want = (yr + yg) + yb;
        CHECK(rtw::adaptive_luma(r, g, b) == want, "luma %a, expected %a", rtw::adaptive_luma(r, g, b), want);
        printf("LUMA %a %a %a %a\n", r, g, b, rtw::adaptive_luma(r, g, b));
        CHECK(rtw::adaptive_luma(1.0, 1.0, 1.0) == (0.2126 + 0.7152) + 0.0722, "luma of white");
        printf("LUMA %a %a %a %a\n", 1.0, 1.0, 1.0, rtw::adaptive_luma(1.0, 1.0, 1.0));
    }

    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // zero variance at tolerance 0: v = 0 <= bound = 0
    rule(4.0, 4.0, 4, 0.0, 1, "constant 1 x 4, tolerance 0");
    rule(0.0, 0.0, 4, 0.0, 1, "constant 0 x 4, tolerance 0");
    // any variance at tolerance 0 goes on
    rule(3.0, 5.0, 2, 0.0, 0, "samples 1 and 2, tolerance 0");
    // q - m * m slightly negative (rounding): clamped to 0, settled
    {
        const double y = 0.1, s1 = (y + y) + y, s2 = (y * y + y * y) + y * y;
        const double m = s1 / 3.0, q = s2 / 3.0;
        CHECK(q - m * m < 0.0, "the case's q - m * m = %a is not negative", q - m * m);
        rule(s1, s2, 3, 0.0, 1, "q - m * m < 0");
    }
    // n = 2: v = var / 1.  samples 0.5 and 1.5: m = 1, q = 1.25, var = 0.25; bound = 4 t^2
    rule(2.0, 2.5, 2, 0.25, 1, "n = 2 at the bound");              // 4 * 0.0625 = 0.25 >= 0.25
    rule(2.0, 2.5, 2, 0.2499999, 0, "n = 2 just over the bound");
    // m below the 2^-16 floor: the bound uses 2^-16.  m = 2^-20, samples 0 and 2^-19: var = 2^-40
    rule(0x1p-19, 0x1p-38, 2, 0x1p-13, 1, "mean under the floor, at the bound");     // 4 * 2^-26 * 2^-16 = 2^-40
    rule(0x1p-19, 0x1p-38, 2, 0x1p-14, 0, "mean under the floor, tolerance halved");
    // ... while with m itself in the bound (2^-20) the first of the two would not be settled
    CHECK(!(0x1p-40 <= ((4.0 * 0x1p-13) * 0x1p-13) * 0x1p-20), "the floor case does not tell the floor");
    // a mean above the floor scales the bound
    rule(8.0, 40.0, 4, 0.5, 1, "m = 2, var = 6, v = 2 <= 1 * 2");
    rule(8.0, 40.0, 4, 0.4, 0, "m = 2, var = 6, v = 2 > 0.64 * 2");
    // sums that are not finite are settled, whatever the tolerance
    rule(nan, 1.0, 4, 0.0, 1, "S1 NaN");
    rule(1.0, nan, 4, 0.0, 1, "S2 NaN");
    rule(inf, 1.0, 4, 0.0, 1, "S1 +inf");
    rule(-inf, 1.0, 4, 0.0, 1, "S1 -inf");
    rule(1.0, inf, 4, 0.0, 1, "S2 +inf");
    rule(1.0, -inf, 4, 0.0, 1, "S2 -inf");
    rule(nan, nan, 32, 0.125, 1, "both NaN");
    // a huge tolerance settles any sample values a render produces
    rule(3.0, 1e50, 2, 1e30, 1, "tolerance 1e30");
    // m * m overflows: q - inf = -inf, clamped to 0
    rule(1e160, 1e308, 2, 0.0, 1, "m * m overflows");
    // a sweep for the restatement
    for (uint32_t n : {2u, 3u, 4u, 31u, 32u, 500u})
        for (double tol : {0.0, 1.0 / 256, 0.125, 0.7})
            for (int i = 0; i < 12; ++i) {
                const double y0 = ldexp(1.0 + 0.37 * i, i - 9), d = y0 * ldexp(1.0, -(i % 5) * 3);
                // n / 2 samples at y0 - d, the others at y0 + d
                double s1 = 0, s2 = 0;
                for (uint32_t k = 0; k < n; ++k) {
                    const double y = k % 2 ? y0 + d : y0 - d;
                    s1 = s1 + y;
                    s2 = s2 + y * y;
                }
                rule(s1, s2, n, tol, -1, "sweep");
            }
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
