// tile_cull.cpp -- see tile_cull.hpp.  Every comparison is written so that a
// NaN keeps the tile, and every bound carries an explicit guard factor
// (kUp / kDown, 2^-30 relative) on the side that keeps it: the few ulps of the
// arithmetic here are far below them.
#include "tile_cull.hpp"

#include <math.h>

#include <algorithm>

#include "tiles.hpp"

namespace rtw {

namespace {

constexpr double kUp = 1.0 + 0x1p-30, kDown = 1.0 - 0x1p-30;
constexpr double kMargin = 0x1p-40;      // the discriminant's margin, relative to F^2
constexpr double kSide = 0x1p-28;        // a sign is proven only this far from 0 (relative)
constexpr double kMinLen = 0x1p-130;

inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline double len3(const double* a) { return sqrt(dot3(a, a)); }
inline void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
inline bool in_range(double x) { return fabs(x) <= kCullMaxAbs; }   // (false for a NaN)

// v = x - apex: its length L, and cos / sin of its angle to the beam's axis
struct Polar {
    double L, ca, sa;
};
inline Polar polar(const Beam& b, const double* x) {
    const double v[3] = {x[0] - b.apex[0], x[1] - b.apex[1], x[2] - b.apex[2]};
    double cr[3];
    cross3(v, b.axis, cr);
    Polar p;
    p.L = len3(v);
    p.ca = dot3(v, b.axis) / p.L;
    p.sa = len3(cr) / p.L;
    return p;
}

// a lower bound of the distance from x to the beam's double cone (<= 0: none)
inline double cone_distance(const Beam& b, const Polar& p) {
    const double s = p.sa * b.cos_t - fabs(p.ca) * b.sin_t;   // sin(angle to the nearer nappe - half angle)
    if (!(s > kSide)) return 0.0;
    return p.L * s * kDown;
}

bool plane_uv_finite(const double* pl) {
    // Plane::get_plane_uv's constants as stage_scene computes them: k = normalize(n x (0, 1, 0))
    const double c[3] = {pl[4] * 0.0 - pl[5] * 1.0, pl[5] * 0.0 - pl[3] * 0.0, pl[3] * 1.0 - pl[4] * 0.0};
    const double clen = len3(c);
    const double theta = atan2(clen, pl[3] * 0.0 + pl[4] * 1.0 + pl[5] * 0.0);
    if (theta <= 2.220446049250313080847e-16) return true;
    return isfinite(c[0] / clen) && isfinite(c[1] / clen) && isfinite(c[2] / clen);
}

// the beam misses every sphere below `node` (a child link of the BVH)
bool misses_subtree(const Beam& b, const CullScene& sc, int32_t link) {
    if (link < 0) {
        const uint32_t code = (uint32_t)~link, first = code >> 4, count = code & 15u;
        for (uint32_t k = first; k < first + count; ++k) {
            const double* s = sc.spheres.data() + 4 * (size_t)sc.bvh.order[k];
            if (!beam_misses_sphere(b, s, s[3])) return false;
        }
        return true;
    }
    const BvhBuild::Node& n = sc.bvh.nodes[(size_t)link];
    for (int ch = 0; ch < 2; ++ch) {
        const double* lo = n.lo[ch];
        const double* hi = n.hi[ch];
        if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) {
            // an empty box (nothing below), or a NaN (then nothing is proven)
            if (lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) continue;
            return false;
        }
        // the box's bounding ball: what misses it misses every sphere inside
        const double c[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
        const double h[3] = {hi[0] - c[0], hi[1] - c[1], hi[2] - c[2]};
        const double g[3] = {c[0] - lo[0], c[1] - lo[1], c[2] - lo[2]};
        const double e[3] = {std::max(h[0], g[0]), std::max(h[1], g[1]), std::max(h[2], g[2])};
        if (beam_misses_sphere(b, c, len3(e) * kUp)) continue;
        if (!misses_subtree(b, sc, n.child[ch])) return false;
    }
    return true;
}

bool camera_in_range(const rtw_camera& cam) {
    const double* v[] = {cam.center, cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v, cam.defocus_disk_u,
                         cam.defocus_disk_v, cam.background};
    for (const double* p : v)
        for (int a = 0; a < 3; ++a)
            if (!in_range(p[a])) return false;
    return isfinite(cam.defocus_angle);
}

// no ray of the pixels [i0, i1) x [j0, j1) (clipped to the image) hits anything
bool rect_empty(const CullScene& sc, const rtw_camera& cam, uint32_t i0, uint32_t i1, uint32_t j0, uint32_t j1) {
    const Beam b = tile_beam(cam, i0, std::min(i1, cam.image_width), j0, std::min(j1, cam.image_height));
    if (!b.ok) return false;
    for (size_t k = 0; k * 6 < sc.planes.size(); ++k)
        if (!beam_misses_plane(b, sc.planes.data() + 6 * k)) return false;
    return sc.bvh.nodes.empty() ? sc.spheres.empty() : misses_subtree(b, sc, 0);
}

// Tiles are asked block by block first: the beam of a block of kBlockTiles x kBlockTiles
// tiles holds every ray of its tiles, so a block that is proven empty settles
// them all with one walk (C2's sky); the tiles of any other block are asked one
// by one.  Blocks are classified on demand (a rank asks for its own tiles only).
constexpr uint32_t kBlockTiles = 8;
struct Blocks {
    const CullScene& sc;
    const rtw_camera& cam;
    uint32_t tiles_x, blocks_x;
    std::vector<uint8_t> state;   // per block: 0 not asked yet, 1 proven empty, 2 not proven
    Blocks(const CullScene& s, const rtw_camera& c)
        : sc(s), cam(c), tiles_x(tiles_across(c.image_width)), blocks_x((tiles_x + kBlockTiles - 1) / kBlockTiles),
          state((size_t)blocks_x * ((tiles_across(c.image_height) + kBlockTiles - 1) / kBlockTiles), 0) {}
    bool tile_empty(uint32_t T) {
        const uint32_t tx = T % tiles_x, ty = T / tiles_x, bx = tx / kBlockTiles, by = ty / kBlockTiles;
        uint8_t& st = state[(size_t)by * blocks_x + bx];
        if (!st) {
            const uint32_t px = kBlockTiles * kTile;
            st = rect_empty(sc, cam, bx * px, (bx + 1) * px, by * px, (by + 1) * px) ? 1 : 2;
        }
        if (st == 1) return true;
        return rect_empty(sc, cam, tx * kTile, (tx + 1) * kTile, ty * kTile, (ty + 1) * kTile);
    }
};

bool cullable(const CullScene& sc, const rtw_camera& cam) {
    return sc.in_range && !sc.other_prims && camera_in_range(cam) && cam.image_width && cam.image_height;
}

}  // namespace

void cull_scene_init(const rtw_scene* s, CullScene* out) {
    out->spheres.assign(s->spheres, s->spheres + 4 * (size_t)s->n_spheres);
    out->planes.assign(s->planes, s->planes + 6 * (size_t)s->n_planes);
    bool emit = false;
    for (uint32_t m = 0; m < s->n_materials; ++m) emit = emit || s->mat_type[m] == RTW_DIFFUSE_LIGHT;
    out->other_prims = s->n_quads || s->n_boxes || s->n_light_quads || s->n_light_other || s->mat_tex || emit;
    bool ok = true;
    for (double x : out->spheres) ok = ok && in_range(x);
    for (double x : out->planes) ok = ok && in_range(x);
    out->in_range = ok;
}

Beam tile_beam(const rtw_camera& cam, uint32_t i0, uint32_t i1, uint32_t j0, uint32_t j1) {
    Beam b;
    if (!camera_in_range(cam) || i1 <= i0 || j1 <= j0) return b;
    // the targets: p00 + du (i + ox) + dv (j + oy), ox, oy in [-1/2, 1/2] (a little more)
    const double u[2] = {(double)i0 - 0.5 - 0x1p-20, (double)i1 - 0.5 + 0x1p-20};
    const double v[2] = {(double)j0 - 0.5 - 0x1p-20, (double)j1 - 0.5 + 0x1p-20};
    double d[4][3], dl[4], sum[3] = {0, 0, 0};
    for (int k = 0; k < 4; ++k) {
        for (int a = 0; a < 3; ++a)
            d[k][a] = cam.pixel00_loc[a] + cam.pixel_delta_u[a] * u[k & 1] + cam.pixel_delta_v[a] * v[k >> 1] -
                      cam.center[a];
        dl[k] = len3(d[k]);
        if (!(dl[k] >= kMinLen)) return b;
        for (int a = 0; a < 3; ++a) sum[a] += d[k][a] / dl[k];
    }
    const double sl = len3(sum);
    if (!(sl >= 1.0)) return b;   // (four unit vectors within 60 degrees of their mean sum to >= 2)
    for (int a = 0; a < 3; ++a) {
        b.apex[a] = cam.center[a];
        b.axis[a] = sum[a] / sl;
    }
    // the pinhole cone: the corners' largest angle to the axis (the targets are
    // their convex hull, the cone is convex); proj: the shortest target distance
    double sin_t = 0.0, proj = INFINITY;
    for (int k = 0; k < 4; ++k) {
        double cr[3];
        cross3(b.axis, d[k], cr);
        const double along = dot3(b.axis, d[k]);
        if (!(along >= 0.5 * dl[k])) return b;
        sin_t = std::max(sin_t, len3(cr) / dl[k]);
        proj = std::min(proj, along);
    }
    if (!(proj >= kMinLen)) return b;
    // the lens ball: |origin - center| <= |disk_u| + |disk_v| (defocus on: camera.rs get_ray)
    const bool defocus = cam.defocus_angle > 2.220446049250313080847e-16;
    b.lens = defocus ? (len3(cam.defocus_disk_u) + len3(cam.defocus_disk_v)) * kUp : 0.0;
    // the rounding of get_ray's target and direction, as an angle: 64 u (the magnitudes) / proj
    const double mag = len3(cam.pixel00_loc) + ((double)cam.image_width + 1.0) * len3(cam.pixel_delta_u) +
                       ((double)cam.image_height + 1.0) * len3(cam.pixel_delta_v) + len3(cam.center) + b.lens;
    const double rounding = 64.0 * 0x1p-53 * mag / proj;
    // half angle: the pinhole cone + the lens (asin(lens / proj)) + the rounding
    b.sin_t = (sin_t + b.lens / proj + rounding) * (1.0 + 0x1p-20) + 0x1p-45;
    if (!(b.sin_t <= 0.5)) return b;
    b.cos_t = sqrt(1.0 - b.sin_t * b.sin_t) * kDown;
    b.ok = true;
    return b;
}

bool beam_contains(const Beam& b, const double x[3]) {
    if (!b.ok) return true;
    const Polar p = polar(b, x);
    if (!(p.L > 0.0)) return true;
    const double s = p.sa * b.cos_t - fabs(p.ca) * b.sin_t;
    return !(p.L * s > b.lens);
}

bool beam_misses_sphere(const Beam& b, const double c[3], double r) {
    if (!b.ok) return false;
    r = fabs(r);
    const Polar p = polar(b, c);
    if (!(p.L > 0.0) || !in_range(p.L) || !in_range(r)) return false;
    const double F = p.L + b.lens + r;                     // >= |o - c| and r over the beam
    const double need = r * r * kUp + kMargin * F * F;     // l^2 >= need: disc <= -a margin F^2
    // the forward cone: the largest cos of a ray direction's angle to c - apex
    const double s_fwd = p.sa * b.cos_t - p.ca * b.sin_t;  // sin(angle(axis, c) - half angle)
    if (!(s_fwd > kSide)) return false;                    // the axis region: a ray may point at c
    const double c_fwd = p.ca * b.cos_t + p.sa * b.sin_t;  // cos of it: every direction's cos is below
    if (p.L * c_fwd + b.lens <= -kSide * F) {
        // every ray points away from c (d . (o - c) > 0 by a margin): cc > 0 puts both roots below 0
        const double l = p.L * kDown - b.lens;
        return l > 0.0 && l * l * kDown >= need;
    }
    // the ray's line against the sphere: the distance to the double cone, less the lens
    const double l = cone_distance(b, p) - b.lens;
    return l > 0.0 && l * l * kDown >= need;
}

bool beam_misses_plane(const Beam& b, const double* pl) {
    if (!b.ok) return false;
    const double nl = len3(pl + 3);
    if (!(nl >= kMinLen) || !in_range(nl)) return false;
    const double n[3] = {pl[3] / nl, pl[4] / nl, pl[5] / nl};
    // (a) the one-sided test fails for every direction: d . n < 0 by a margin
    double cr[3];
    cross3(b.axis, n, cr);
    const double an = dot3(b.axis, n), sn = len3(cr);
    if (sn * b.cos_t - an * b.sin_t > kSide && an * b.cos_t + sn * b.sin_t <= -kSide) return true;
    // (b) it may pass, but every origin is strictly on the far side: t = -((o - p) . n) / (d . n) < 0
    // (the UV of that point, computed before the range test, must be finite: plane.rs:66-69)
    const double v[3] = {b.apex[0] - pl[0], b.apex[1] - pl[1], b.apex[2] - pl[2]};
    const double h = dot3(v, n);
    if (!plane_uv_finite(pl)) return false;
    return h - b.lens >= kSide * (len3(v) + b.lens + kMinLen);
}

uint32_t classify_tiles(const CullScene& sc, const rtw_camera& cam, std::vector<uint8_t>* flags) {
    const uint64_t n = n_tiles_of(cam.image_width, cam.image_height);
    flags->assign((size_t)n, 0);
    if (!cullable(sc, cam)) return 0;
    uint32_t culled = 0;
    Blocks blocks(sc, cam);
    for (uint64_t T = 0; T < n; ++T) {
        (*flags)[(size_t)T] = blocks.tile_empty((uint32_t)T) ? 1 : 0;
        culled += (*flags)[(size_t)T];
    }
    return culled;
}

void cull_classify(CullState& st, const LptKey& key, const CullScene& sc, const std::vector<uint32_t>& tiles) {
    st.drop();
    st.key = key;
    st.valid = true;
    ++st.serial;
    if (!st.serial) ++st.serial;
    st.flags.assign(tiles.size(), 0);
    const rtw_camera& cam = key.cam;
    if (!cullable(sc, cam)) return;
    const uint32_t tiles_x = tiles_across(cam.image_width);
    Blocks blocks(sc, cam);
    for (size_t lt = 0; lt < tiles.size(); ++lt) {
        if (!blocks.tile_empty(tiles[lt])) continue;
        st.flags[lt] = 1;
        ++st.n_culled;
        const uint32_t tx = tiles[lt] % tiles_x, ty = tiles[lt] / tiles_x;
        st.culled_pixels += (uint64_t)std::min(kTile, cam.image_width - tx * kTile) *
                            std::min(kTile, cam.image_height - ty * kTile);
    }
}

std::vector<uint32_t> plain_task_list(const std::vector<uint8_t>& flags, uint32_t n_chunks, uint32_t group) {
    std::vector<uint32_t> tab;
    group = std::max(1u, std::min(group, 4095u));   // (the entry holds the chunk count in 12 bits)
    for (uint32_t lt = 0; lt < (uint32_t)flags.size(); ++lt) {
        if (flags[lt]) continue;
        for (uint32_t cb = 0; cb < n_chunks; cb += group) {
            tab.push_back(lt);
            tab.push_back(cb | (std::min(group, n_chunks - cb) << 20));
        }
    }
    return tab;
}

}  // namespace rtw
