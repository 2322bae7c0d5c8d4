// window_plan_check.cpp -- CPU check of plan_windows (host/render_plan.cpp):
// how a render is cut into sample windows.  Built and run by
// tests/test_window_plan_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -I<csrc> -I<include> window_plan_check.cpp \
//       <csrc>/host/render_plan.cpp -o window_plan_check
#include <stdio.h>

#include <algorithm>

#include "host/render_plan.hpp"
#include "host/tiles.hpp"

static int g_wrong = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++g_wrong;                   \
            printf("WRONG: " __VA_ARGS__); \
            printf("\n");                \
        }                                \
    } while (0)

constexpr size_t kHbm = (size_t)288 << 30;   // an MI355X's memory

template <typename R>
static size_t bytes_of(uint32_t window, uint32_t chunk, uint32_t tiles) {
    return (size_t)((window + chunk - 1) / chunk) * tiles * 64 * 3 * sizeof(R);
}

// the windows [k * window, ...) cover [0, spp) exactly, only the last one short
static void check_cover(const rtw::WindowPlan& w, uint32_t spp, const char* name) {
    CHECK(w.chunk >= 1, "%s: chunk 0", name);
    if (spp == 0) {
        CHECK(w.n_windows == 0, "%s: %u windows of no samples", name, w.n_windows);
        return;
    }
    CHECK(w.window >= 1 && w.n_windows >= 1, "%s: window %u x %u", name, w.window, w.n_windows);
    if (w.window == 0) return;
    CHECK(w.n_windows == 1 || w.window % w.chunk == 0, "%s: window %u is no multiple of chunk %u", name, w.window,
          w.chunk);
    uint64_t done = 0;
    for (uint32_t k = 0; k < w.n_windows; ++k) {
        const uint64_t first = (uint64_t)k * w.window;
        CHECK(first == done && first < spp, "%s: window %u starts at %llu", name, k, (unsigned long long)first);
        const uint64_t n = std::min<uint64_t>(w.window, spp - first);
        CHECK(n == w.window || k + 1 == w.n_windows, "%s: window %u is short", name, k);
        done = first + n;
    }
    CHECK(done == spp, "%s: covered %llu of %u", name, (unsigned long long)done, spp);
}

template <typename R>
static void check_precision(const char* pr) {
    char name[128];
    // BASELINE shapes {W, H, spp}: C1 / C2 / C3 / C4 / C5, and a C4 share over 8 and 4 ranks
    const uint32_t shapes[][4] = {{400, 225, 100, 1},   {1200, 800, 500, 1}, {1920, 1080, 1000, 1},
                                  {3840, 2160, 4096, 1}, {1920, 1080, 64, 1}, {3840, 2160, 4096, 8},
                                  {3840, 2160, 4096, 4}};
    for (const auto& s : shapes) {
        const uint32_t tiles = rtw::tiles_for_rank(s[0], s[1], 0, s[3]);
        for (uint32_t chunk : {0u, 1u, 4u}) {
            rtw::RenderKnobs k;   // window 0: off
            k.chunk = chunk;
            for (size_t dev : {(size_t)0, kHbm}) {
                const rtw::WindowPlan w = rtw::plan_windows<R>(k, s[2], tiles, dev);
                const uint32_t c = rtw::plan_chunk<R>(k, s[2], tiles, dev);
                snprintf(name, sizeof name, "%s off %ux%ux%u/%u chunk %u", pr, s[0], s[1], s[2], s[3], chunk);
                CHECK(w.chunk == c && w.window == s[2] && w.n_windows == 1 && w.partial_bytes == bytes_of<R>(s[2], c, tiles),
                      "%s: chunk %u window %u x %u bytes %zu (plan_chunk %u)", name, w.chunk, w.window, w.n_windows,
                      w.partial_bytes, c);
                check_cover(w, s[2], name);
            }
        }
    }
    // an explicit window: rounded up to a multiple of an explicit chunk, the last window short
    struct {
        int64_t window;
        uint32_t chunk, spp, want_chunk, want_window, want_n;
    } ex[] = {
        {100, 0, 500, 1, 100, 5}, {250, 0, 500, 1, 250, 2}, {4, 0, 10, 1, 4, 3},    {5, 2, 12, 2, 6, 2},
        {4, 8, 20, 8, 8, 3},      {7, 3, 7, 3, 7, 1},       {500, 0, 500, 1, 500, 1}, {600, 4, 500, 4, 500, 1},
        {3, 4, 4, 4, 4, 1},       {1, 0, 3, 1, 1, 3},
    };
    for (const auto& e : ex) {
        rtw::RenderKnobs k;
        k.window = e.window;
        k.chunk = e.chunk;
        const rtw::WindowPlan w = rtw::plan_windows<R>(k, e.spp, 1000, kHbm);
        snprintf(name, sizeof name, "%s window %lld chunk %u spp %u", pr, (long long)e.window, e.chunk, e.spp);
        CHECK(w.chunk == e.want_chunk && w.window == e.want_window && w.n_windows == e.want_n,
              "%s: chunk %u window %u x %u, expected %u %u x %u", name, w.chunk, w.window, w.n_windows, e.want_chunk,
              e.want_window, e.want_n);
        CHECK(w.partial_bytes == bytes_of<R>(w.window, w.chunk, 1000), "%s: %zu bytes", name, w.partial_bytes);
        check_cover(w, e.spp, name);
    }
    // auto: a C4 share over 4 ranks (2 073 600 px -> 32 400 tiles, 4096 spp) is over the
    // one-shot budget; the window keeps one sample per item within it
    {
        rtw::RenderKnobs k;
        const uint32_t tiles = 32400, spp = 4096;
        CHECK(rtw::tiles_for_rank(3840, 2160, 0, 4) == tiles, "%s: a C4 N = 4 share has %u tiles", pr,
              rtw::tiles_for_rank(3840, 2160, 0, 4));
        const size_t budget = std::min(k.partial_max, kHbm / 2);
        if (sizeof(R) == 8)
            CHECK(rtw::plan_chunk<R>(k, spp, tiles, kHbm) > 1, "f64: the C4 N = 4 share fits the budget at chunk 1");
        k.window = rtw::RenderKnobs::kWindowAuto;
        const rtw::WindowPlan w = rtw::plan_windows<R>(k, spp, tiles, kHbm);
        snprintf(name, sizeof name, "%s auto C4 N = 4", pr);
        printf("%s: chunk %u window %u x %u, %zu bytes (budget %zu)\n", name, w.chunk, w.window, w.n_windows,
               w.partial_bytes, budget);
        CHECK(w.chunk == 1 && w.partial_bytes <= budget, "%s: chunk %u, %zu bytes over %zu", name, w.chunk,
              w.partial_bytes, budget);
        CHECK(w.partial_bytes == bytes_of<R>(w.window, 1, tiles), "%s: bytes", name);
        // the largest: one more chunk would not fit (or the render is one window)
        CHECK(w.n_windows == 1 || bytes_of<R>(w.window + 1, 1, tiles) > budget, "%s: a larger window fits", name);
        check_cover(w, spp, name);
        // ... and the same at any spp, with the device's size unknown too
        for (uint32_t more : {100000u, 0xFFFFFFFFu}) {
            const rtw::WindowPlan m = rtw::plan_windows<R>(k, more, tiles, 0);
            CHECK(m.chunk == 1 && m.partial_bytes <= k.partial_max, "%s at %u spp: chunk %u", name, more, m.chunk);
            check_cover(m, more, name);
        }
        // the whole render fits: one window, the one-shot plan
        const rtw::WindowPlan small = rtw::plan_windows<R>(k, 500, 15000, kHbm);
        CHECK(small.n_windows == 1 && small.window == 500 && small.chunk == 1, "%s: C2 fits, got %u x %u", pr,
              small.window, small.n_windows);
        // an explicit chunk under auto: the window is a multiple of it
        k.chunk = 3;
        k.partial_max = (size_t)1 << 30;
        const rtw::WindowPlan c3 = rtw::plan_windows<R>(k, spp, tiles, kHbm);
        CHECK(c3.chunk == 3 && c3.window % 3 == 0 && c3.partial_bytes <= k.partial_max && c3.n_windows > 1,
              "%s chunk 3: window %u x %u", name, c3.window, c3.n_windows);
        check_cover(c3, spp, name);
    }
    // nothing to render: no division by zero
    for (int64_t window : {(int64_t)0, (int64_t)4, rtw::RenderKnobs::kWindowAuto})
        for (uint32_t spp : {0u, 7u})
            for (uint32_t tiles : {0u, 3u}) {
                if (spp && tiles) continue;
                rtw::RenderKnobs k;
                k.window = window;
                const rtw::WindowPlan w = rtw::plan_windows<R>(k, spp, tiles, 0);
                snprintf(name, sizeof name, "%s window %lld spp %u tiles %u", pr, (long long)window, spp, tiles);
                CHECK(w.partial_bytes == bytes_of<R>(w.window, w.chunk, tiles), "%s: %zu bytes", name, w.partial_bytes);
                check_cover(w, spp, name);
            }
}

int main() {
    check_precision<float>("f32");
    check_precision<double>("f64");
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
