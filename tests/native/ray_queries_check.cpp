// ray_queries_check.cpp -- the C++ host mirror's hit_rays / light_pdf
// (host/ray_queries.cpp) on scenes::simple: prints the rays it asked about and
// what came back, in hex floats, one ray per line:
//   ray <6 values> hit <object> <material> <front> <kind> <t p normal u v: 9 values> pdf <value>
// tests/test_gpu_query_mirror.py builds it against librtw.so, runs it on the
// GPU and asks the Python mirror the same rays.
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
        std::vector<double> rays;
        for (uint32_t j = 0; j < cam.image_height; ++j)
            for (uint32_t i = 0; i < cam.image_width; ++i)
                for (int a = 0; a < 6; ++a)
                    rays.push_back(a < 3 ? cam.center[a]
                                         : cam.pixel00_loc[a - 3] + i * cam.pixel_delta_u[a - 3] +
                                               j * cam.pixel_delta_v[a - 3] - cam.center[a - 3]);
        const std::vector<rtw::RayHit> hits = rtw::hit_rays(world, lights, rays);
        // the light pdf of the rays that leave the hit points along the normal
        std::vector<double> bounce;
        for (const rtw::RayHit& h : hits) {
            const double v[6] = {h.p.x, h.p.y, h.p.z, h.normal.x, h.normal.y + 0.25, h.normal.z};
            bounce.insert(bounce.end(), v, v + 6);
        }
        const std::vector<double> pdf = rtw::light_pdf(world, lights, bounce);
        for (size_t k = 0; k < hits.size(); ++k) {
            const rtw::RayHit& h = hits[k];
            printf("ray");
            for (int a = 0; a < 6; ++a) printf(" %a", rays[6 * k + a]);
            printf(" hit %d %d %d %d %a %a %a %a %a %a %a %a %a pdf %a\n", h.object, h.material, h.front_face ? 1 : 0,
                   h.kind, h.t, h.p.x, h.p.y, h.p.z, h.normal.x, h.normal.y, h.normal.z, h.u, h.v, pdf[k]);
        }
    } catch (const rtw::Error& e) {
        fprintf(stderr, "ray_queries_check: %s (code %d)\n", e.what(), e.code());
        return 2;
    }
    return 0;
}
