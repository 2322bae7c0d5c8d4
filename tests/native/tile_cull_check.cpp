// tile_cull_check.cpp -- CPU check of the tile classifier (host/tile_cull.hpp)
// and of the fold's constant (rtw_kernels.h fold_constant).  Built and run by
// tests/test_tile_cull_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -ffunction-sections -Wl,--gc-sections \
//       -I<csrc> -I<include> tile_cull_check.cpp <csrc>/host/{tile_cull,bvh,rtw_host,render_plan,stage_scene}.cpp \
//       -o tile_cull_check        (rtw_host.cpp's entry points that need the device half are unused: dropped)
//   tile_cull_check                 the checks below; the last line is "<n> wrong"
//   tile_cull_check flags <file>    the flags of the cameras of a scene file (the oracle's
//                                   side of the soundness test is Python's): u32 n_spheres,
//                                   n_planes, n_cameras, then the spheres (4 doubles each), the
//                                   planes (6), the cameras (rtw_camera); one line of 0 / 1
//                                   per camera, by global tile
//   tile_cull_check time            the classifier's host time: `simple` at 1200x800, and a
//                                   field of 10^6 spheres
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <random>
#include <vector>

#include "host/render_plan.hpp"
#include "host/tile_cull.hpp"
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

using rtw::Beam;
using rtw::CullScene;

struct Scene {
    std::vector<double> sph, pl;
    CullScene cs;
    void finish() {
        rtw_scene s{};
        s.n_spheres = (uint32_t)(sph.size() / 4);
        s.spheres = sph.data();
        s.n_planes = (uint32_t)(pl.size() / 6);
        s.planes = pl.data();
        rtw::cull_scene_init(&s, &cs);
        cs.bvh = rtw::build_bvh(sph.data(), s.n_spheres, 1e-12, 4);
    }
};

static Scene simple_scene() {
    Scene sc;
    rtw_world* w = rtw_scene_simple(0x5EED0001ull, 11);
    const rtw_scene* s = rtw_world_scene(w);
    sc.sph.assign(s->spheres, s->spheres + 4 * (size_t)s->n_spheres);
    sc.pl.assign(s->planes, s->planes + 6 * (size_t)s->n_planes);
    rtw_world_free(w);
    sc.finish();
    return sc;
}

static rtw_camera_builder simple_builder(uint32_t W, uint32_t H) {
    rtw_world* w = rtw_scene_simple(0x5EED0001ull, 11);
    rtw_camera_builder b;
    rtw_world_camera_builder(w, &b);
    rtw_world_free(w);
    b.has_image_width = b.has_image_height = 1;
    b.image_width = W;
    b.image_height = H;
    b.samples_per_pixel = 4;
    return b;
}
static rtw_camera build(const rtw_camera_builder& b) {
    rtw_camera cam;
    const int rc = rtw_camera_build(&b, &cam);
    CHECK(rc == RTW_OK, "rtw_camera_build: %d", rc);
    return cam;
}

static uint32_t count(const std::vector<uint8_t>& f) {
    uint32_t n = 0;
    for (uint8_t x : f) n += x;
    return n;
}

// Sphere::hit's discriminant for the ray (o, d), in long double
static bool exact_hits(const double* o, const double* d, const double* s) {
    long double oc[3], a = 0, hb = 0, cc = 0;
    for (int k = 0; k < 3; ++k) {
        oc[k] = (long double)o[k] - s[k];
        a += (long double)d[k] * d[k];
        hb += (long double)d[k] * oc[k];
        cc += oc[k] * oc[k];
    }
    cc -= (long double)s[3] * s[3];
    const long double disc = hb * hb - a * cc;
    if (!(disc > 0)) return false;
    const long double sq = sqrtl(disc), t1 = (-hb - sq) / a, t2 = (-hb + sq) / a;
    return t1 >= 2.220446049250313e-16L || t2 >= 2.220446049250313e-16L;
}

// the pinhole ray through (i + ox, j + oy)
static void pinhole(const rtw_camera& c, double u, double v, double* d) {
    for (int a = 0; a < 3; ++a)
        d[a] = c.pixel00_loc[a] + c.pixel_delta_u[a] * u + c.pixel_delta_v[a] * v - c.center[a];
}

static void check_counts() {
    Scene sc = simple_scene();
    const rtw_camera cam = build(simple_builder(121, 83));
    std::vector<uint8_t> f;
    const uint32_t n = rtw::classify_tiles(sc.cs, cam, &f);
    printf("simple 121x83: %u of %zu tiles proved empty\n", n, f.size());
    CHECK(f.size() == 176 && n >= 30 && n < 176 && n == count(f), "simple 121x83: %u of %zu", n, f.size());
    // the tree only prunes: what it proves, the loop over every sphere proves
    uint32_t brute = 0;
    const uint32_t tiles_x = rtw::tiles_across(cam.image_width);
    for (uint32_t T = 0; T < f.size(); ++T) {
        const uint32_t i0 = T % tiles_x * 8, j0 = T / tiles_x * 8;
        const Beam b = rtw::tile_beam(cam, i0, std::min(i0 + 8, cam.image_width), j0, std::min(j0 + 8, cam.image_height));
        bool miss = b.ok;
        for (size_t k = 0; miss && k < sc.pl.size() / 6; ++k) miss = rtw::beam_misses_plane(b, sc.pl.data() + 6 * k);
        for (size_t k = 0; miss && k < sc.sph.size() / 4; ++k)
            miss = rtw::beam_misses_sphere(b, sc.sph.data() + 4 * k, sc.sph[4 * k + 3]);
        brute += miss;
        CHECK(!f[T] || miss, "tile %u: the tree proves what the loop does not", T);
    }
    printf("simple 121x83: %u by the loop over every sphere\n", brute);
    // looking away from everything, above the one-sided ground: the plane condition
    // (b) holds for every tile, and every tile is culled
    rtw_camera_builder away = simple_builder(121, 83);
    away.lookat[0] = 2 * away.lookfrom[0];
    away.lookat[1] = away.lookfrom[1] + 30.0;
    away.lookat[2] = 2 * away.lookfrom[2];
    const uint32_t na = rtw::classify_tiles(sc.cs, build(away), &f);
    CHECK(na == 176, "looking away: %u of 176", na);
    // inside the sphere field: some tile sees a sphere
    rtw_camera_builder in = simple_builder(121, 83);
    in.lookfrom[0] = 2.0; in.lookfrom[1] = 0.6; in.lookfrom[2] = 2.5;
    in.lookat[0] = -6.0; in.lookat[1] = 3.0; in.lookat[2] = -4.0;
    const uint32_t ni = rtw::classify_tiles(sc.cs, build(in), &f);
    printf("inside the field: %u of 176\n", ni);
    CHECK(ni > 0 && ni < 176, "inside the field: %u culled", ni);
}

// one sphere at distance r (1 + k margin) from a tile's corner ray
static void check_adversarial() {
    const rtw_camera cam = build(simple_builder(121, 83));
    const uint32_t tiles_x = rtw::tiles_across(cam.image_width);
    const uint32_t T = 5 * tiles_x + 7, i0 = 7 * 8, j0 = 5 * 8;
    const Beam b = rtw::tile_beam(cam, i0, i0 + 8, j0, j0 + 8);
    CHECK(b.ok, "adversarial: no beam");
    const double uv[4][2] = {{i0 - 0.5, j0 - 0.5}, {i0 + 7.5, j0 - 0.5}, {i0 - 0.5, j0 + 7.5}, {i0 + 7.5, j0 + 7.5}};
    int kept_in = 0, culled_out = 0;
    for (int corner = 0; corner < 4; ++corner) {
        double d[3], dl = 0, e[3], el = 0, along = 0;
        pinhole(cam, uv[corner][0], uv[corner][1], d);
        for (int a = 0; a < 3; ++a) dl += d[a] * d[a];
        dl = sqrt(dl);
        for (int a = 0; a < 3; ++a) along += d[a] / dl * b.axis[a];
        // e: unit, perpendicular to the ray, pointing away from the beam's axis
        for (int a = 0; a < 3; ++a) e[a] = d[a] / dl * along - b.axis[a];
        for (int a = 0; a < 3; ++a) el += e[a] * e[a];
        el = sqrt(el);
        // (make it perpendicular to d exactly enough: remove the component along d)
        double ed = 0;
        for (int a = 0; a < 3; ++a) ed += e[a] / el * d[a] / dl;
        for (int a = 0; a < 3; ++a) e[a] = e[a] / el - ed * d[a] / dl;
        for (double r : {0.05, 0.7, 40.0}) {
            for (double s : {0.5, 3.0, 25.0}) {   // where along the ray the sphere comes closest (x |d|)
                const double F = s * dl + r, margin = 0x1p-41 * F * F / (r * r);   // l = r (1 + margin): l^2 ~ r^2 + 2^-40 F^2
                for (double k : {-1e12, -1e6, -16.0, -1.0, 0.0, 0.25, 0.5, 0.9, 1.5, 4.0, 1e3, 1e6, 1e9, 1e13}) {
                    // (k < 0: inside the sphere, down to its far side at most)
                    const double dist = r * (1.0 + std::max(k * margin, -1.9));
                    Scene sc;
                    for (int a = 0; a < 3; ++a) sc.sph.push_back(cam.center[a] + d[a] * s + e[a] * dist);
                    sc.sph.push_back(r);
                    sc.finish();
                    std::vector<uint8_t> f;
                    rtw::classify_tiles(sc.cs, cam, &f);
                    const bool hit = exact_hits(cam.center, d, sc.sph.data());
                    if (k < 1.0 || hit) {
                        CHECK(!f[T], "corner %d r %g s %g k %g: culled inside the margin (exact hit %d)", corner, r, s, k, (int)hit);
                        kept_in += !f[T];
                    }
                    CHECK(!(hit && k > 1.0), "corner %d r %g s %g k %g: the exact ray hits outside the margin", corner, r, s, k);
                    if (k >= 1e13) {
                        culled_out += f[T];
                    }
                }
            }
        }
    }
    printf("adversarial: %d kept inside the margin, %d culled far outside\n", kept_in, culled_out);
    CHECK(kept_in >= 200 && culled_out >= 12, "adversarial: vacuous (%d, %d)", kept_in, culled_out);
}

static void check_degenerate() {
    const rtw_camera cam = build(simple_builder(121, 83));
    const uint32_t tiles_x = rtw::tiles_across(cam.image_width);
    std::vector<uint8_t> f;
    double mid[3];
    pinhole(cam, 60.0, 41.0, mid);   // the centre pixel's ray: tile (7, 5)
    const uint32_t Tmid = 5 * tiles_x + 7;
    // no sphere, no plane: every tile
    {
        Scene sc;
        sc.finish();
        CHECK(rtw::classify_tiles(sc.cs, cam, &f) == 176, "empty scene: %u", count(f));
    }
    // a negative radius counts as |r|; coincident spheres
    for (int variant = 0; variant < 2; ++variant) {
        Scene sc;
        for (int n = 0; n < (variant ? 9 : 1); ++n) {
            for (int a = 0; a < 3; ++a) sc.sph.push_back(cam.center[a] + mid[a] * 0.6);
            sc.sph.push_back(variant ? 0.3 : -0.3);
        }
        sc.finish();
        const uint32_t n = rtw::classify_tiles(sc.cs, cam, &f);
        CHECK(!f[Tmid] && n > 100 && n < 176, "%s: centre tile %d, %u culled", variant ? "coincident" : "negative radius",
              (int)f[Tmid], n);
    }
    // a sphere that contains the camera
    {
        Scene sc;
        for (int a = 0; a < 3; ++a) sc.sph.push_back(cam.center[a] + 0.25);
        sc.sph.push_back(3.0);
        sc.finish();
        CHECK(rtw::classify_tiles(sc.cs, cam, &f) == 0, "camera inside a sphere: %u culled", count(f));
    }
    // a NaN or infinite sphere value, far off screen
    for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY, 0x1p131}) {
        for (int slot = 0; slot < 4; ++slot) {
            Scene sc;
            sc.sph = {-50.0, 80.0, -50.0, 0.5, 1e3, 1e3, 1e3, 1.0};
            sc.sph[4 + slot] = bad;
            sc.finish();
            CHECK(rtw::classify_tiles(sc.cs, cam, &f) == 0, "sphere value %g in slot %d: %u culled", bad, slot, count(f));
        }
        Scene sc;
        sc.pl = {0, 0, 0, 0, 1, 0};
        sc.pl[1] = bad;
        sc.finish();
        CHECK(rtw::classify_tiles(sc.cs, cam, &f) == 0, "plane value %g: %u culled", bad, count(f));
        // ... or camera value
        Scene ok;
        ok.finish();
        double* fields[] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        rtw_camera c2 = cam;
        fields[0] = c2.center; fields[1] = c2.pixel00_loc; fields[2] = c2.pixel_delta_u; fields[3] = c2.pixel_delta_v;
        fields[4] = c2.defocus_disk_u; fields[5] = c2.defocus_disk_v; fields[6] = c2.background;
        for (int q = 0; q < 7; ++q) {
            c2 = cam;
            fields[q][1] = bad;
            CHECK(rtw::classify_tiles(ok.cs, c2, &f) == 0, "camera field %d = %g: %u culled", q, bad, count(f));
        }
    }
    // a camera below the one-sided ground (normal up): a ray that goes up meets it
    {
        Scene sc;
        sc.pl = {0, 0, 0, 0, 1, 0};
        sc.finish();
        rtw_camera_builder b = simple_builder(121, 83);
        b.lookfrom[1] = -5.0;
        b.lookat[1] = -5.0;
        const rtw_camera below = build(b);
        const uint32_t n = rtw::classify_tiles(sc.cs, below, &f);
        uint32_t see = 0, blind = 0;
        for (uint32_t T = 0; T < f.size(); ++T) {
            const uint32_t i0 = T % tiles_x * 8, j0 = T / tiles_x * 8;
            bool up = false;
            for (int q = 0; q < 81; ++q) {
                double d[3];
                pinhole(below, i0 - 0.5 + q % 9, j0 - 0.5 + q / 9, d);
                up = up || d[1] > 0.0;
            }
            if (up) {
                ++see;
                CHECK(!f[T], "below the plane: tile %u sees it and is culled", T);
            } else {
                blind += f[T];
            }
        }
        printf("below the plane: %u culled, %u tiles see the plane, %u look down and are culled\n", n, see, blind);
        CHECK(see > 20 && blind > 20, "below the plane: vacuous");
    }
    // a quad or a texture: never
    {
        Scene sc;
        sc.finish();
        rtw_scene s{};
        const double quad[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
        s.n_quads = 1;
        s.quads = quad;
        rtw::cull_scene_init(&s, &sc.cs);
        CHECK(sc.cs.other_prims && rtw::classify_tiles(sc.cs, cam, &f) == 0, "a quad: %u culled", count(f));
        rtw_scene t{};
        const uint32_t tex[1] = {0};
        t.mat_tex = tex;
        rtw::cull_scene_init(&t, &sc.cs);
        CHECK(sc.cs.other_prims && rtw::classify_tiles(sc.cs, cam, &f) == 0, "a texture: %u culled", count(f));
        rtw_scene e{};
        const uint32_t mt[1] = {RTW_DIFFUSE_LIGHT};
        e.n_materials = 1;
        e.mat_type = mt;
        rtw::cull_scene_init(&e, &sc.cs);
        CHECK(sc.cs.other_prims, "an emitter");
    }
}

// every point of every ray of a tile lies in the volume its beam stands for
static void check_lemma() {
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    // (the lens radius is focus_dist * tan(defocus_angle / 2) with the angle taken as it is,
    // camera.rs: 0.02 at 10 is a lens of 0.1; 2.0 one of 15.6, wider than any beam bounds)
    for (int variant = 0; variant < 4; ++variant) {
        rtw_camera_builder bld = simple_builder(121, 83);
        if (variant >= 1) {
            bld.defocus_angle = variant == 1 ? 0.02 : variant == 2 ? 0.1 : 2.0;
            bld.focus_dist = variant == 2 ? 2.5 : 10.0;
        }
        const rtw_camera cam = build(bld);
        const uint32_t tiles_x = rtw::tiles_across(cam.image_width);
        uint32_t beams = 0, outside = 0;
        for (uint32_t T = 0; T < 176; ++T) {
            const uint32_t i0 = T % tiles_x * 8, j0 = T / tiles_x * 8;
            const uint32_t i1 = std::min(i0 + 8, cam.image_width), j1 = std::min(j0 + 8, cam.image_height);
            const Beam b = rtw::tile_beam(cam, i0, i1, j0, j1);
            if (!b.ok) continue;
            ++beams;
            for (int n = 0; n < 400; ++n) {
                const double u = i0 + (uint32_t)(U(rng) * (i1 - i0)) + (n % 5 == 0 ? (n % 2 ? 0.5 : -0.5) : U(rng) - 0.5);
                const double v = j0 + (uint32_t)(U(rng) * (j1 - j0)) + (n % 7 == 0 ? (n % 2 ? 0.5 : -0.5) : U(rng) - 0.5);
                double px, pz;   // the lens point: the unit disk, its rim now and then
                do {
                    px = 2 * U(rng) - 1;
                    pz = 2 * U(rng) - 1;
                } while (px * px + pz * pz > 1.0);
                if (n % 3 == 0) {
                    const double l = sqrt(px * px + pz * pz);
                    if (l > 0) { px /= l; pz /= l; }
                }
                const double t = n % 4 == 0 ? -3.0 * U(rng) : (n % 4 == 1 ? 1.0 + 1e3 * U(rng) : 2.0 * U(rng));
                double x[3];
                for (int a = 0; a < 3; ++a) {
                    const double o = variant ? cam.center[a] + cam.defocus_disk_u[a] * px + cam.defocus_disk_v[a] * pz
                                             : cam.center[a];
                    const double target = cam.pixel00_loc[a] + cam.pixel_delta_u[a] * u + cam.pixel_delta_v[a] * v;
                    x[a] = o + t * (target - o);
                }
                outside += !rtw::beam_contains(b, x);
            }
        }
        CHECK(beams == (variant == 3 ? 0u : 176u) && outside == 0, "lemma, variant %d: %u beams, %u points outside", variant,
              beams, outside);
    }
}

// the kernels' addition sequence on a constant, against a plain sample-by-sample fold
template <typename R>
static void check_fold(const char* pr) {
    for (double bg : {1.0, 0.7, 0.1, 1e-300, -0.0, 0.0, 3.0000000001}) {
        const R col = rtw::miss_colour<R>((R)bg);
        CHECK(col == (R)bg && !std::signbit(col) == !(std::signbit((R)bg) && (R)bg != 0), "%s: miss colour of %g", pr, bg);
        // one sample per item (the default): the reference's sequential fold, at any spp
        for (uint32_t spp : {1u, 8u, 500u}) {
            double plain = 0;
            for (uint32_t s = 0; s < spp; ++s) plain = plain + (double)((R)0 + col);
            CHECK(rtw::fold_constant<R>(0.0, col, spp, 1) == plain, "%s bg %g spp %u chunk 1", pr, bg, spp);
            // windows of 3 at chunk 1 carry the sum: the same additions
            double w = 0;
            for (uint32_t first = 0; first < spp; first += 3) w = rtw::fold_constant<R>(w, col, std::min(3u, spp - first), 1);
            CHECK(w == plain, "%s bg %g spp %u windows of 3", pr, bg, spp);
        }
        // chunk 3, spp 8: chunk sums ((0 + c) + c) + c twice, then the short (0 + c) + c, in R;
        // the running sum in f64, in chunk order
        const R c3 = (((R)0 + col) + col) + col, c2 = ((R)0 + col) + col;
        const double want = ((0.0 + (double)c3) + (double)c3) + (double)c2;
        CHECK(rtw::fold_constant<R>(0.0, col, 8, 3) == want, "%s bg %g chunk 3", pr, bg);
        // ... in two windows of 6 and 2 (a window starts on an item boundary)
        CHECK(rtw::fold_constant<R>(rtw::fold_constant<R>(0.0, col, 6, 3), col, 2, 3) == want, "%s bg %g chunk 3 windows", pr, bg);
        // where every sum is exact the association cannot matter: the plain fold again
        if (bg == 1.0 || bg == 0.0) {
            double plain = 0;
            for (int s = 0; s < 8; ++s) plain = plain + (double)col;
            CHECK(want == plain, "%s bg %g chunk 3 against the plain fold", pr, bg);
        }
    }
}

static rtw::LptKey key_of(const rtw_camera& cam) {
    rtw::LptKey k{};
    k.cam = cam;
    k.scene_serial = 1;
    k.nranks = 1;
    k.prec = 8;
    return k;
}

static void check_keys_and_tasks() {
    Scene sc = simple_scene();
    rtw_camera_builder bb = simple_builder(121, 83);
    const rtw_camera A = build(bb);
    bb.lookat[1] = 3.0;
    bb.vfov = 25.0;
    const rtw_camera B = build(bb);
    std::vector<uint8_t> fa, fb;
    const uint32_t na = rtw::classify_tiles(sc.cs, A, &fa), nb = rtw::classify_tiles(sc.cs, B, &fb);
    CHECK(fa != fb && na && nb, "two cameras, the same flags");
    std::vector<uint32_t> tiles;
    rtw::local_tiles(nullptr, 121, 83, 0, 1, tiles);
    rtw::CullState st;
    CHECK(!st.has(key_of(A)), "a new state has flags");
    rtw::cull_classify(st, key_of(A), sc.cs, tiles);
    const uint32_t serial_a = st.serial;
    CHECK(st.has(key_of(A)) && !st.has(key_of(B)) && st.flags == fa && st.n_culled == na, "camera A");
    rtw::cull_classify(st, key_of(B), sc.cs, tiles);
    CHECK(st.has(key_of(B)) && !st.has(key_of(A)) && st.flags == fb && st.n_culled == nb && st.serial != serial_a &&
              !st.tab_valid, "camera B after A");
    rtw::cull_classify(st, key_of(A), sc.cs, tiles);
    CHECK(st.has(key_of(A)) && st.flags == fa && st.serial != serial_a, "camera A again");
    rtw::LptKey other = key_of(A);
    other.scene_serial = 2;
    CHECK(!st.has(other), "another scene, the same flags");
    st.drop();
    CHECK(!st.has(key_of(A)) && st.flags.empty() && !st.n_culled, "dropped");
    // a rank's share: its own tiles' flags, and the pixels inside the image
    std::vector<uint32_t> t1;
    rtw::local_tiles(nullptr, 121, 83, 1, 3, t1);
    rtw::LptKey k1 = key_of(A);
    k1.rank = 1;
    k1.nranks = 3;
    rtw::cull_classify(st, k1, sc.cs, t1);
    uint64_t px = 0;
    for (size_t lt = 0; lt < t1.size(); ++lt) {
        CHECK(st.flags[lt] == fa[t1[lt]], "rank 1 of 3: local tile %zu", lt);
        if (st.flags[lt]) px += (uint64_t)std::min(8u, 121 - t1[lt] % 16 * 8) * std::min(8u, 83 - t1[lt] / 16 * 8);
    }
    CHECK(st.culled_pixels == px && px > 0, "rank 1 of 3: %llu pixels, expected %llu", (unsigned long long)st.culled_pixels,
          (unsigned long long)px);
    CHECK(rtw::RenderKnobs{}.tile_cull == 1, "tile_cull is not on by default");
    // the task lists: no task of a flagged tile, every other (tile, chunk) once
    std::vector<uint32_t> cost(fa.size());
    for (size_t k = 0; k < cost.size(); ++k) cost[k] = fa[k] ? 0u : (uint32_t)(k * 37 % 11);   // zero costs among the kept, too
    rtw::RenderKnobs knobs;
    for (int which = 0; which < 3; ++which) {
        const uint32_t n_chunks = which == 2 ? 8 : 500;
        const std::vector<uint32_t> tab = which == 0   ? rtw::plain_task_list(fa, n_chunks, 32)
                                          : which == 1 ? rtw::build_task_list(cost, n_chunks, 0, rtw::kAutoTasks, knobs, fa.data())
                                                       : rtw::build_task_list(cost, n_chunks, 3, rtw::kAutoTasks, knobs, fa.data());
        std::vector<uint32_t> seen(fa.size() * n_chunks, 0);
        for (size_t k = 0; k + 1 < tab.size(); k += 2) {
            const uint32_t lt = tab[k], cb = tab[k + 1] & 0xFFFFFu, g = tab[k + 1] >> 20;
            CHECK(lt < fa.size() && !fa[lt] && g >= 1 && cb + g <= n_chunks, "list %d: entry %zu", which, k / 2);
            for (uint32_t c = cb; c < cb + g && lt < fa.size() && c < n_chunks; ++c) ++seen[lt * n_chunks + c];
        }
        bool once = true;
        for (size_t lt = 0; lt < fa.size(); ++lt)
            for (uint32_t c = 0; c < n_chunks; ++c) once = once && seen[lt * n_chunks + c] == (fa[lt] ? 0u : 1u);
        CHECK(once, "list %d: a chunk of a kept tile is missing or doubled, or a culled tile has a task", which);
    }
    // every tile flagged: no task at all
    CHECK(rtw::plain_task_list(std::vector<uint8_t>(5, 1), 8, 4).empty() &&
              rtw::build_task_list(std::vector<uint32_t>(5, 0), 8, 0, rtw::kAutoTasks, knobs, std::vector<uint8_t>(5, 1).data()).empty(),
          "all culled: tasks");
}

static int print_flags(const char* path) {
    FILE* fp = fopen(path, "rb");
    if (!fp) return 2;
    uint32_t n[3];
    if (fread(n, 4, 3, fp) != 3) return 2;
    Scene sc;
    sc.sph.resize(4 * (size_t)n[0]);
    sc.pl.resize(6 * (size_t)n[1]);
    if (fread(sc.sph.data(), 8, sc.sph.size(), fp) != sc.sph.size() || fread(sc.pl.data(), 8, sc.pl.size(), fp) != sc.pl.size())
        return 2;
    sc.finish();
    for (uint32_t k = 0; k < n[2]; ++k) {
        rtw_camera cam;
        if (fread(&cam, sizeof cam, 1, fp) != 1) return 2;
        std::vector<uint8_t> f;
        rtw::classify_tiles(sc.cs, cam, &f);
        for (uint8_t x : f) putchar(x ? '1' : '0');
        putchar('\n');
    }
    fclose(fp);
    return 0;
}

static void print_times() {
    auto ms = [](auto t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    std::vector<uint8_t> f;
    {
        Scene sc = simple_scene();
        rtw_camera_builder b = simple_builder(1200, 800);
        const rtw_camera cam = build(b);
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t n = rtw::classify_tiles(sc.cs, cam, &f);
        printf("simple 1200x800: %u of %zu tiles proved empty in %.2f ms\n", n, f.size(), ms(t0));
        const rtw_camera small = build(simple_builder(400, 225));
        printf("simple 400x225: %u of %llu\n", rtw::classify_tiles(sc.cs, small, &f),
               (unsigned long long)rtw::n_tiles_of(400, 225));
    }
    {
        // 10^6 small spheres on a 1000 x 1000 ground grid, the camera pulled back as for the large synthetic scenes
        Scene sc;
        std::mt19937_64 rng(7);
        std::uniform_real_distribution<double> U(0.0, 0.9);
        for (int a = -500; a < 500; ++a)
            for (int c = -500; c < 500; ++c) {
                sc.sph.insert(sc.sph.end(), {a + U(rng), 0.2, c + U(rng), 0.2});
            }
        sc.pl = {0, 0, 0, 0, 1, 0};
        auto t0 = std::chrono::steady_clock::now();
        sc.finish();
        printf("10^6 spheres: scene + tree in %.0f ms (the tree is the staged one in the library)\n", ms(t0));
        rtw_camera_builder b = simple_builder(1200, 800);
        const double k = 500.0 / 11.0;
        b.lookfrom[0] = 10.0 * k; b.lookfrom[1] = 5.0 * k; b.lookfrom[2] = 10.0 * k;
        b.vfov = 40.0;
        const rtw_camera cam = build(b);
        t0 = std::chrono::steady_clock::now();
        const uint32_t n = rtw::classify_tiles(sc.cs, cam, &f);
        printf("10^6 spheres 1200x800: %u of %zu tiles proved empty in %.2f ms\n", n, f.size(), ms(t0));
    }
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "flags")) return print_flags(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "time")) {
        print_times();
        return 0;
    }
    check_counts();
    check_adversarial();
    check_degenerate();
    check_lemma();
    check_fold<double>("f64");
    check_fold<float>("f32");
    check_keys_and_tasks();
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
