// adaptive_mirror_check.cpp -- Camera::render_adaptive of the C++ host mirror
// (host/rtw_host.hpp) on the GPU: scenes::simple, 36 x 20, depth 8, render
// seed 11, min 4 / window 4 / max 32 at tolerance 0.125 in f64, written to
// argv[1] as H * W records of four doubles {sum r, g, b, count}.  Built against
// librtw.so and compared with the restated rule by tests/test_gpu_adaptive.py.
#include <stdio.h>

#include <vector>

#include "host/rtw_host.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    try {
        auto [world, lights, builder] = rtw::scenes::simple(0x5EED0001ULL, 11);
        rtw::Camera cam = builder.with_image_width(36).with_image_height(20).with_samples_per_pixel(1)
                              .with_max_depth(8).build();
        rtw::RenderOptions opt;
        opt.seed = 11;
        opt.precision = RTW_F64;
        const auto rows = cam.render_adaptive(world, lights, 4, 32, 4, 0.125, opt);
        std::vector<double> out;
        for (const auto& row : rows)
            for (const auto& px : row) out.insert(out.end(), {px.sum.x, px.sum.y, px.sum.z, (double)px.spp});
        // a rejected argument throws before any device work
        bool threw = false;
        try {
            cam.render_adaptive(world, lights, 1, 32, 4, 0.125, opt);
        } catch (const rtw::Error& e) {
            threw = e.code() == RTW_E_INVALID;
        }
        if (!threw) {
            fprintf(stderr, "min_samples 1 was not rejected with RTW_E_INVALID\n");
            return 1;
        }
        FILE* f = fopen(argv[1], "wb");
        if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 1;
        fclose(f);
    } catch (const rtw::Error& e) {
        fprintf(stderr, "rtw: %s (code %d)\n", e.what(), e.code());
        return 1;
    }
    return 0;
}
