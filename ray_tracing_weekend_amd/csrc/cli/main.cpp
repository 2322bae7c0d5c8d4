// rtw -- the reference's bin/ (bin/src/main.rs:54-105) on the C++ host mirror:
// reads ./Config.toml's [image] table (bin/src/config.rs:3-107), builds the
// scene, applies main.rs:72-79's camera overrides, renders on the GPU and
// writes image.ppm (P3, rows top to bottom).
//
//   rtw <scene> [--debug] [--seed N] [--f64] [--device N | --device-mask M] [--config PATH] [--out PATH]
//       [--features PREFIX] [--denoise PATH [--denoise-variance]]
//
// --features PREFIX also writes the denoising guides of the render
// (rtw_render_features, on one device): PREFIX_albedo.ppm, the albedo sums with
// the sample count, and PREFIX_normal.ppm, (mean normal + 1) / 2 -- squared
// before the writer's sqrt, so that the displayed value is linear.
//
// --denoise PATH also writes the denoised image (rtw_denoise over the render's
// sums and its feature pass, with the default parameters); it implies the
// feature pass and runs on one device like --features.  With --denoise-variance
// the denoised image is the variance-guided filter's instead
// (rtw_render_window_moments of all the samples, then rtw_denoise_variance with
// the default parameters).
//
// <scene> is one of clap's ValueEnum names of main.rs:29-38 (cornell-box,
// debug, checkered-spheres, perlin-spheres, plane, simple, simple-light,
// simple-transform; snake_case accepted too).  --seed drives simple's
// generator and the Perlin tables (the reference uses thread_rng).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <functional>
#include <map>
#include <sstream>
#include <string>

#include "host/rtw_host.hpp"

namespace {

std::string trim(const std::string& s) {
    size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
    return a == std::string::npos ? "" : s.substr(a, b - a + 1);
}

// A minimal reader for the [image] table of Config.toml.
bool read_config(const std::string& path, std::map<std::string, std::string>* kv) {
    std::ifstream f(path);
    if (!f) return false;
    std::string line, section;
    while (std::getline(f, line)) {
        size_t hash = line.find('#');
        if (hash != std::string::npos) line = line.substr(0, hash);
        line = trim(line);
        if (line.empty()) continue;
        if (line.front() == '[') {
            section = trim(line.substr(1, line.find(']') - 1));
            continue;
        }
        size_t eq = line.find('=');
        if (eq == std::string::npos || section != "image") continue;
        (*kv)[trim(line.substr(0, eq))] = trim(line.substr(eq + 1));
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    std::string scene, config = "Config.toml", out = "image.ppm", features, denoised;
    bool variance = false;
    rtw::RenderOptions opt;
    for (int a = 1; a < argc; ++a) {
        std::string s = argv[a];
        if (s == "--debug") continue;  // render_debug == render on the GPU
        else if (s == "--seed" && a + 1 < argc) opt.seed = strtoull(argv[++a], nullptr, 0);
        else if (s == "--f64") opt.precision = RTW_F64;   // (the default)
        else if (s == "--f32") opt.precision = RTW_F32;   // the speed mode
        else if (s == "--device" && a + 1 < argc) opt.device = atoi(argv[++a]);
        else if (s == "--device-mask" && a + 1 < argc) opt.device_mask = strtoull(argv[++a], nullptr, 0);
        else if (s == "--config" && a + 1 < argc) config = argv[++a];
        else if (s == "--out" && a + 1 < argc) out = argv[++a];
        else if (s == "--features" && a + 1 < argc) features = argv[++a];
        else if (s == "--denoise" && a + 1 < argc) denoised = argv[++a];
        else if (s == "--denoise-variance") variance = true;
        else if (scene.empty()) scene = s;
        else { fprintf(stderr, "unexpected argument %s\n", s.c_str()); return 2; }
    }
    if (variance && denoised.empty()) {
        fprintf(stderr, "--denoise-variance goes with --denoise PATH\n");
        return 2;
    }
    for (char& ch : scene)
        if (ch == '-') ch = '_';
    using Gen = std::function<std::tuple<rtw::HittableList, rtw::HittableList, rtw::CameraBuilder>()>;
    const uint64_t seed = opt.seed;
    const std::map<std::string, Gen> gens = {
        {"cornell_box", [] { return rtw::scenes::cornell_box(); }},
        {"debug", [seed] { return rtw::scenes::debugging_scene(seed); }},
        {"checkered_spheres", [] { return rtw::scenes::checkered_spheres(); }},
        {"perlin_spheres", [seed] { return rtw::scenes::perlin_spheres(seed); }},
        {"plane", [] { return rtw::scenes::plane(); }},
        {"simple", [seed] { return rtw::scenes::simple(seed); }},
        {"simple_light", [seed] { return rtw::scenes::simple_light(seed); }},
        {"simple_transform", [seed] { return rtw::scenes::simple_transform(seed); }},
    };
    if (!gens.count(scene)) {
        fprintf(stderr, "unknown scene '%s' (cornell-box, debug, checkered-spheres, perlin-spheres, plane, "
                        "simple, simple-light, simple-transform)\n", scene.c_str());
        return 2;
    }
    std::map<std::string, std::string> kv;
    if (!read_config(config, &kv)) {
        fprintf(stderr, "cannot read %s\n", config.c_str());
        return 1;
    }
    // PreImage::fix (config.rs:60-98): two of aspect/width/height are needed
    bool ha = kv.count("aspect_ratio"), hw = kv.count("image_width"), hh = kv.count("image_height");
    double aspect = ha ? atof(kv["aspect_ratio"].c_str()) : 0.0;
    uint32_t W = hw ? (uint32_t)atol(kv["image_width"].c_str()) : 0;
    uint32_t H = hh ? (uint32_t)atol(kv["image_height"].c_str()) : 0;
    if ((int)ha + (int)hw + (int)hh < 2) {
        fprintf(stderr, "Config.toml [image] needs two of aspect_ratio/image_width/image_height\n");
        return 1;
    }
    if (!ha) aspect = (double)W / (double)H;
    else if (!hh) H = (uint32_t)((double)W / aspect);
    else if (!hw) W = (uint32_t)((double)H * aspect);
    const uint32_t spp = (uint32_t)atol(kv["samples_per_pixel"].c_str());
    const uint32_t depth = (uint32_t)atol(kv["max_depth"].c_str());

    auto [world, lights, builder] = gens.at(scene)();
    try {
        rtw::Camera cam = builder.with_vfov(40.0)
                              .with_aspect_ratio(aspect)
                              .with_max_depth(depth)
                              .with_image_width(W)
                              .with_image_height(H)
                              .with_samples_per_pixel(spp)
                              .build();
        auto rows = cam.render(world, lights, opt);
        std::vector<double> sums((size_t)W * H * 3);
        for (uint32_t j = 0; j < H; ++j)
            for (uint32_t i = 0; i < W; ++i) {
                double* d = &sums[((size_t)j * W + i) * 3];
                d[0] = rows[j][i].sum.x;
                d[1] = rows[j][i].sum.y;
                d[2] = rows[j][i].sum.z;
            }
        if (rtw_write_ppm(out.c_str(), sums.data(), W, H, spp) < 0) {
            fprintf(stderr, "cannot write %s\n", out.c_str());
            return 1;
        }
        if (!features.empty() || !denoised.empty()) {
            rtw::RenderOptions fopt = opt;
            fopt.device_mask = 0;   // the feature pass runs on one device
            const std::vector<double> f = cam.render_features(world, lights, 0, spp, {}, nullptr, fopt);
            if (!denoised.empty()) {
                rtw_denoise_stats st{};
                std::vector<double> mean;
                if (variance) {
                    std::vector<double> wsums, moments;
                    cam.render_window_moments(world, lights, 0, spp, wsums, moments, fopt);
                    mean = rtw::denoise_variance(wsums, f, moments, {}, spp, W, H, nullptr, &st, fopt);
                } else {
                    mean = rtw::denoise(sums, f, {}, spp, W, H, nullptr, &st, fopt);
                }
                if (rtw_write_ppm(denoised.c_str(), mean.data(), W, H, 1) < 0) {
                    fprintf(stderr, "cannot write %s\n", denoised.c_str());
                    return 1;
                }
                fprintf(stderr, "denoise: %llu pixels filled, %llu left non-finite, %.3f ms\n",
                        (unsigned long long)st.filled, (unsigned long long)st.left_nonfinite, st.kernel_ms);
            }
            if (features.empty()) return 0;
            std::vector<double> albedo((size_t)W * H * 3), normal((size_t)W * H * 3);
            for (size_t px = 0; px < (size_t)W * H; ++px) {
                const double* v = &f[px * 8];
                const double len = sqrt((v[3] * v[3] + v[4] * v[4]) + v[5] * v[5]);
                for (int c = 0; c < 3; ++c) {
                    albedo[px * 3 + c] = v[c];
                    const double shown = ((len > 0.0 ? v[3 + c] / len : 0.0) + 1.0) / 2.0;
                    normal[px * 3 + c] = shown * shown;
                }
            }
            const std::string fa = features + "_albedo.ppm", fn = features + "_normal.ppm";
            if (rtw_write_ppm(fa.c_str(), albedo.data(), W, H, spp) < 0 ||
                rtw_write_ppm(fn.c_str(), normal.data(), W, H, 1) < 0) {
                fprintf(stderr, "cannot write %s / %s\n", fa.c_str(), fn.c_str());
                return 1;
            }
        }
    } catch (const rtw::Error& e) {
        fprintf(stderr, "rtw: %s (code %d)\n", e.what(), e.code());
        return 1;
    }
    return 0;
}
