// nee_check.cpp -- the C++ host mirror's occluded / light_sample
// (host/ray_queries.cpp) on scenes::simple: prints what it asked and what came
// back, in hex floats, one camera ray per line:
//   ray <6 values> tmax <value> occ <0 / 1> origin <3 values> dir <3 values> pdf <value> light <index>
// The origins of the light samples are the camera rays' points at t = 3.
// tests/test_gpu_nee_mirror.py builds it against librtw.so, runs it on the GPU
// and asks the Python mirror the same questions.
#include <math.h>
#include <stdio.h>

#include <tuple>
#include <vector>

#include "host/rtw_host.hpp"

int main() {
    try {
        const auto scene = rtw::scenes::simple(0x5EED0001, 11);
        const rtw::HittableList& world = std::get<0>(scene);
        const rtw::HittableList& lights = std::get<1>(scene);
        rtw::CameraBuilder b = std::get<2>(scene);
        const rtw_camera cam = b.with_image_width(12).with_image_height(8).build().raw();
        std::vector<double> rays, t_max, origins;
        for (uint32_t j = 0; j < cam.image_height; ++j)
            for (uint32_t i = 0; i < cam.image_width; ++i) {
                double r[6];
                for (int a = 0; a < 3; ++a) {
                    r[a] = cam.center[a];
                    r[a + 3] = cam.pixel00_loc[a] + i * cam.pixel_delta_u[a] + j * cam.pixel_delta_v[a] - cam.center[a];
                }
                rays.insert(rays.end(), r, r + 6);
                const size_t k = t_max.size();
                t_max.push_back(k % 3 == 0 ? INFINITY : (k % 3 == 1 ? 1.0 + 0.5 * (double)k : 0.25));
                for (int a = 0; a < 3; ++a) origins.push_back(r[a] + 3.0 * r[a + 3]);
            }
        const std::vector<uint8_t> occ = rtw::occluded(world, lights, rays, t_max);
        const std::vector<uint8_t> occ_inf = rtw::occluded(world, lights, rays);
        const rtw::LightSamples s = rtw::light_sample(world, lights, origins, 7, 100, 2);
        const rtw::LightSamples plain = rtw::light_sample(world, lights, origins, 7, 100, 2, false);
        if (!plain.pdf.empty() || plain.directions != s.directions || plain.light != s.light) {
            fprintf(stderr, "nee_check: the samples without the pdf differ\n");
            return 3;
        }
        for (size_t k = 0; k < occ.size(); ++k) {
            printf("ray");
            for (int a = 0; a < 6; ++a) printf(" %a", rays[6 * k + a]);
            printf(" tmax %a occ %d %d origin %a %a %a dir %a %a %a pdf %a light %d\n", t_max[k], occ[k], occ_inf[k],
                   origins[3 * k], origins[3 * k + 1], origins[3 * k + 2], s.directions[3 * k], s.directions[3 * k + 1],
                   s.directions[3 * k + 2], s.pdf[k], s.light[k]);
        }
    } catch (const rtw::Error& e) {
        fprintf(stderr, "nee_check: %s (code %d)\n", e.what(), e.code());
        return 2;
    }
    return 0;
}
