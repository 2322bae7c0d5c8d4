// tile_cull.hpp -- tiles whose camera beam provably misses the scene: for a
// scene of spheres and planes and a camera, which 8x8 tiles can be answered
// without tracing -- every ray Camera::get_ray can generate for any of the
// tile's pixels misses every primitive, so every sample is 1 * background + 0
// (DESIGN.md §4 has the proof and its margins; rtw_kernels.h fold_constant is
// the fold kernels' addition sequence on that constant).  Host only, no HIP call: capi_render.cpp keeps the flags under the task-order key.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../../include/rtw.h"
#include "bvh.hpp"
#include "lpt_state.hpp"

namespace rtw {

// What the classifier reads of a scene: kept by the context at rtw_set_scene
// (f64 contexts only).  spheres: n x {cx, cy, cz, r} as given; planes: n x
// {point, normal}; bvh: build_bvh over `spheres` (boxes hold |r|).
struct CullScene {
    std::vector<double> spheres, planes;
    BvhBuild bvh;
    bool other_prims = false;   // quads, cuboids, textures or emitters: never culled
    bool in_range = false;      // every value finite and |x| <= kCullMaxAbs
};
constexpr double kCullMaxAbs = 0x1p130;   // beyond it (or below 2^-130 in length) nothing is culled

// scene values -> CullScene (the BVH is the caller's: stage_scene's own build)
void cull_scene_init(const rtw_scene* s, CullScene* out);

// The conservative volume of a tile's rays: every point o + t (target - o), any
// real t, of every ray the camera can generate for the tile lies within `lens`
// of the double cone of apex `apex`, unit axis `axis` and half angle asin(sin_t)
// (sin_t <= 1/2); every ray direction lies within that angle of the axis.
struct Beam {
    bool ok = false;            // false: no bound (the tile is kept)
    double apex[3], axis[3];
    double sin_t, cos_t;        // the half angle, rounded outward (sin up, cos down)
    double lens;                // lens ball radius (0: defocus off)
};
// the beam of pixels [i0, i1) x [j0, j1) of `cam`
Beam tile_beam(const rtw_camera& cam, uint32_t i0, uint32_t i1, uint32_t j0, uint32_t j1);
// x lies inside the beam's volume (the lemma's check: tests/native/tile_cull_check.cpp)
bool beam_contains(const Beam& b, const double x[3]);
// no ray of the beam can hit the sphere {c, r}: the discriminant of Sphere::hit is
// negative by the margin, or both roots are behind the origin
bool beam_misses_sphere(const Beam& b, const double c[3], double r);
// ... or the plane {point, normal}: Plane::hit's one-sided test fails, or t < 0
bool beam_misses_plane(const Beam& b, const double* plane);

// flags[T] = 1 for every global tile T of the image that is provably empty.
// Nothing is flagged for a scene with other primitives, a value out of range,
// or a camera that is not finite.  Returns the number of flagged tiles.
uint32_t classify_tiles(const CullScene& sc, const rtw_camera& cam, std::vector<uint8_t>* flags);

// The flags of a context's last classified key, by LOCAL tile of the rank, and
// the plain-order task list without the flagged tiles.  Kept under the same key
// as the task order (LptKey) and never carried across a key change: a stale
// flag is a wrong image.
struct CullState {
    bool valid = false;
    LptKey key{};
    uint32_t serial = 0;              // ++ per classification: the id a task list was built for (0: none)
    std::vector<uint8_t> flags;       // [local tile]
    uint32_t n_culled = 0;
    uint64_t culled_pixels = 0;       // the pixels inside the image of the flagged tiles
    // the plain-order task list of (flags, tab_chunks, tab_group)
    bool tab_valid = false;
    uint32_t tab_chunks = 0, tab_group = 0;
    std::vector<uint32_t> h_tasks;

    bool has(const LptKey& k) const { return valid && key == k; }
    void drop() { valid = tab_valid = false; n_culled = 0; culled_pixels = 0; flags.clear(); }
};
// (re)classify for `key`: the rank's tiles `tiles` (global, in packed order) of the key's camera
void cull_classify(CullState& st, const LptKey& key, const CullScene& sc, const std::vector<uint32_t>& tiles);

// The plain tile order without the flagged tiles: {local tile, first chunk |
// chunks << 20} of every task of `group` chunks (the order of a render without
// a task table, t = tile * n_groups + group)
std::vector<uint32_t> plain_task_list(const std::vector<uint8_t>& flags, uint32_t n_chunks, uint32_t group);

}  // namespace rtw
