// stage_scene.cpp -- see stage_scene.hpp.  Built with -ffp-contract=off: the
// derived records are computed in the oracle's operation order.
#include "stage_scene.hpp"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "bvh.hpp"

namespace rtw {

namespace {

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// x rounded into T towards -inf / +inf: boxes round outward (they only ever cull)
template <typename T>
T round_down(double x) {
    T r = (T)x;
    return (double)r > x ? std::nextafter(r, (T)-INFINITY) : r;
}
template <typename T>
T round_up(double x) {
    T r = (T)x;
    return (double)r < x ? std::nextafter(r, (T)INFINITY) : r;
}

// both child boxes of a binary node rounded outward into T
template <typename T>
BvhNode<T> pack_node(const BvhBuild::Node& n) {
    BvhNode<T> d{};
    for (int c = 0; c < 2; ++c) {
        d.lo_x[c] = round_down<T>(n.lo[c][0]);
        d.lo_y[c] = round_down<T>(n.lo[c][1]);
        d.lo_z[c] = round_down<T>(n.lo[c][2]);
        d.hi_x[c] = round_up<T>(n.hi[c][0]);
        d.hi_y[c] = round_up<T>(n.hi[c][1]);
        d.hi_z[c] = round_up<T>(n.hi[c][2]);
        d.child[c] = n.child[c];
    }
    return d;
}

}  // namespace

// Quad::new (quadrilateral.rs:37-56) in f64, in the oracle's operation order
// (rtw_oracle.c quad_new): out = {Q, u, v, w, normal, area, box lo, box hi}.
void quad_derive(const double* p, double* out) {
    const double q[3] = {p[0], p[1], p[2]}, u[3] = {p[3], p[4], p[5]}, v[3] = {p[6], p[7], p[8]};
    // AABBox::from_points([q + (u + v) * 0.5, q, q + v, q + u, q + u + v]),
    // each enclose followed by pad_to_minimum (aabox.rs:129-175)
    double pts[5][3];
    for (int a = 0; a < 3; ++a) {
        pts[0][a] = q[a] + (u[a] + v[a]) * 0.5;
        pts[1][a] = q[a];
        pts[2][a] = q[a] + v[a];
        pts[3][a] = q[a] + u[a];
        pts[4][a] = (q[a] + u[a]) + v[a];
    }
    double mn[3], mx[3];
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = pts[0][a];
    for (int i = 1; i < 5; ++i) {
        for (int a = 0; a < 3; ++a) {
            mn[a] = fmin(mn[a], pts[i][a]);
            mx[a] = fmax(mx[a], pts[i][a]);
        }
        for (int a = 0; a < 3; ++a)
            if (mx[a] - mn[a] < 0.0001) {
                mn[a] -= 0.0001;
                mx[a] += 0.0001;
            }
    }
    const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const double n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const double area = sqrt(n2);
    for (int a = 0; a < 3; ++a) {
        out[a] = q[a];
        out[3 + a] = u[a];
        out[6 + a] = v[a];
        out[9 + a] = n[a] / n2;
        out[12 + a] = n[a] / area;
        out[16 + a] = mn[a];
        out[19 + a] = mx[a];
    }
    out[15] = area;
    out[22] = out[23] = 0.0;
}

// Transformed<Cuboid> derived record in f64, in the oracle's operation order
// (rtw_oracle.c box_new); layout rtw_kernels.h kBoxR.
void box_derive(const double* b, double* out) {
    auto enclose_pad = [](double* mn, double* mx, const double* pmn, const double* pmx) {
        for (int a = 0; a < 3; ++a) {
            mn[a] = fmin(mn[a], pmn[a]);
            mx[a] = fmax(mx[a], pmx[a]);
        }
        for (int a = 0; a < 3; ++a)
            if (mx[a] - mn[a] < 0.0001) {
                mn[a] -= 0.0001;
                mx[a] += 0.0001;
            }
    };
    // Cuboid::new: the padded box of p and q, then the six quads
    double mn[3] = {b[0], b[1], b[2]}, mx[3] = {b[0], b[1], b[2]};
    enclose_pad(mn, mx, b + 3, b + 3);
    const double delta[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
    const double dx[3] = {delta[0], 0.0, 0.0}, dy[3] = {0.0, delta[1], 0.0}, dz[3] = {0.0, 0.0, delta[2]};
    const double ndx[3] = {-dx[0], -dx[1], -dx[2]}, ndy[3] = {-dy[0], -dy[1], -dy[2]},
                 ndz[3] = {-dz[0], -dz[1], -dz[2]};
    const double* args[6][3] = {{mn, dx, dy}, {mn, dy, dz}, {mn, dx, dz}, {mx, ndx, ndy}, {mx, ndy, ndz}, {mx, ndx, ndz}};
    double cmn[3] = {0, 0, 0}, cmx[3] = {0, 0, 0};
    for (int i = 0; i < 6; ++i) {
        double q[9];
        for (int a = 0; a < 3; ++a) {
            q[a] = args[i][0][a];
            q[3 + a] = args[i][1][a];
            q[6 + a] = args[i][2][a];
        }
        double* Q = out + rtw::kQuadR * i;
        quad_derive(q, Q);
        // Cuboid::get_aabbox: fold of the quads' boxes
        if (i == 0) {
            for (int a = 0; a < 3; ++a) {
                cmn[a] = Q[16 + a];
                cmx[a] = Q[19 + a];
            }
        } else {
            enclose_pad(cmn, cmx, Q + 16, Q + 19);
        }
    }
    double* Rm = out + rtw::kBoxRot;
    for (int k = 0; k < 9; ++k) Rm[k] = b[6 + k];
    for (int a = 0; a < 3; ++a) out[rtw::kBoxT + a] = b[15 + a];
    auto mul = [&](const double* M, const double* p, double* o) {
        for (int r = 0; r < 3; ++r) o[r] = M[3 * r] * p[0] + M[3 * r + 1] * p[1] + M[3 * r + 2] * p[2];
    };
    // world AABB: from_points of the cuboid box corners (get_points order) mapped by R p + T
    const double* lo = cmn;
    const double* hi = cmx;
    const double corners[8][3] = {{lo[0], lo[1], lo[2]}, {lo[0], hi[1], lo[2]}, {lo[0], lo[1], hi[2]},
                                  {lo[0], hi[1], hi[2]}, {hi[0], lo[1], lo[2]}, {hi[0], hi[1], lo[2]},
                                  {hi[0], lo[1], hi[2]}, {hi[0], hi[1], hi[2]}};
    double wmn[3], wmx[3];
    for (int i = 0; i < 8; ++i) {
        double w[3];
        mul(Rm, corners[i], w);
        for (int a = 0; a < 3; ++a) w[a] = w[a] + b[15 + a];
        if (i == 0) {
            for (int a = 0; a < 3; ++a) wmn[a] = wmx[a] = w[a];
        } else {
            enclose_pad(wmn, wmx, w, w);
        }
    }
    for (int a = 0; a < 3; ++a) {
        out[rtw::kBoxLo + a] = wmn[a];
        out[rtw::kBoxHi + a] = wmx[a];
    }
    // Matrix3::inverse (matrix3.rs:9-28), Transformation::inverse
    const double a = Rm[0], bb = Rm[1], c = Rm[2], d = Rm[3], e = Rm[4], f = Rm[5], g = Rm[6], h = Rm[7],
                 i = Rm[8];
    const double det = a * (e * i - f * h) + bb * (f * g - d * i) + c * (d * h - e * g);
    out[rtw::kBoxOk] = std::isnormal(det) ? 1.0 : 0.0;
    const double A = e * i - f * h, Bc = f * g - d * i, C = d * h - e * g;
    const double D = c * h - bb * i, E = a * i - c * g, F = bb * g - a * h;
    const double G = bb * f - c * e, H = c * d - a * f, I = a * e - bb * d;
    double* Ri = out + rtw::kBoxInv;
    Ri[0] = A / det; Ri[1] = D / det; Ri[2] = G / det;
    Ri[3] = Bc / det; Ri[4] = E / det; Ri[5] = H / det;
    Ri[6] = C / det; Ri[7] = F / det; Ri[8] = I / det;
    double rt[3];
    mul(Ri, b + 15, rt);
    for (int a2 = 0; a2 < 3; ++a2) out[rtw::kBoxTi + a2] = -rt[a2];
    out[rtw::kBoxOk + 1] = 0.0;
}

// Convert the caller's f64 SoA into the device layout of precision R, in one
// host staging blob, and fill the DevScene pointers relative to `base`.
template <typename R>
std::vector<unsigned char> stage_scene(const rtw_scene* s, rtw::DevScene<R>* ds, uintptr_t base,
                                       uint32_t leaf_max, uint32_t light_leaf, double grid_density,
                                       rtw::BvhBuild* keep_bvh) {
    using R4 = rtw::R4<R>;
    size_t off = 0;
    auto reserve = [&](size_t bytes) {
        size_t o = align_up(off, 64);
        off = o + bytes;
        return o;
    };
    const size_t o_sph = reserve(sizeof(R4) * s->n_spheres);
    // the f64 copies read by the f32 kernels' kOptHit64 parts only
    constexpr bool k64 = std::is_same<R, float>::value;
    const size_t o_s64 = reserve(k64 ? sizeof(double) * 4 * s->n_spheres : 0);
    const size_t o_pl64 = reserve(k64 ? sizeof(double) * 8 * s->n_planes : 0);
    // the per-material f64 scatter record: both precisions (the f64 kernels' one-pass
    // Metal / Dielectric scatter reads it too)
    const size_t o_m64 = reserve(sizeof(double) * 4 * s->n_materials);
    const size_t o_r = reserve(sizeof(R) * s->n_spheres);
    const size_t o_smat = reserve(sizeof(uint32_t) * s->n_spheres);
    const size_t o_sshade = reserve(sizeof(R4) * s->n_spheres);
    const size_t o_pl = reserve(sizeof(R) * rtw::kPlaneR * s->n_planes);
    const size_t o_quads = reserve(sizeof(R) * rtw::kQuadR * s->n_quads);
    const size_t o_qmat = reserve(sizeof(uint32_t) * s->n_quads);
    const size_t o_lquads = reserve(sizeof(R) * rtw::kQuadR * s->n_light_quads);
    const uint32_t n_list = s->n_lights + s->n_light_quads + s->n_light_other;
    const size_t o_lref = reserve(sizeof(uint32_t) * n_list);
    const size_t o_boxes = reserve(sizeof(R) * rtw::kBoxR * s->n_boxes);
    const size_t o_bmat = reserve(sizeof(uint32_t) * s->n_boxes);
    const size_t o_pmat = reserve(sizeof(uint32_t) * s->n_planes);
    const size_t o_mt = reserve(sizeof(uint32_t) * s->n_materials);
    const size_t o_mp = reserve(sizeof(R4) * s->n_materials);
    const size_t o_li = reserve(sizeof(R4) * s->n_lights);
    const bool tex = s->mat_tex != nullptr;
    const size_t o_mtex = reserve(sizeof(uint32_t) * (tex ? s->n_materials : 0));
    const size_t o_ttype = reserve(sizeof(uint32_t) * (tex ? s->n_textures : 0));
    const size_t o_tp = reserve(sizeof(R4) * (tex ? s->n_textures : 0));
    const size_t o_trefs = reserve(sizeof(uint32_t) * 2 * (tex ? s->n_textures : 0));
    const size_t o_pvec = reserve(sizeof(R4) * 256 * (tex ? s->n_perlin : 0));
    const size_t o_pperm = reserve(sizeof(uint32_t) * 768 * (tex ? s->n_perlin : 0));
    // BVH over the spheres; boxes padded outward by a margin that absorbs the
    // rounding of the slab test in precision R (it only ever culls)
    const rtw::BvhBuild bb = rtw::build_bvh(s->spheres, s->n_spheres,
                                            std::is_same<R, float>::value ? 1e-5 : 1e-12, leaf_max);
    const size_t o_nodes = reserve(sizeof(rtw::BvhNode<R>) * bb.nodes.size());
    // f64: the same tree in f32 (boxes rounded outward), which the while-while
    // traversal culls on with an error slack (bvh_traverse_ww)
    const size_t o_nodes32 = reserve(std::is_same<R, double>::value ? sizeof(rtw::BvhNode<float>) * bb.nodes.size() : 0);
    // f64: the leaf spheres {c, r^2} rounded to f32, the leaf pre-pass of the f64 kernels
    const size_t o_bsph32 = reserve(std::is_same<R, double>::value ? sizeof(rtw::R4<float>) * s->n_spheres : 0);
    const size_t o_bsph = reserve(sizeof(R4) * s->n_spheres);
    const size_t o_bid = reserve(sizeof(uint32_t) * s->n_spheres);
    // isolated spheres (self-hit shortcut): bit 31 of sphere_mat.  The margin
    // covers the rounding of the hit point the next segment starts from and
    // of the precision-R sphere tests of nearby spheres (grazing hits).
    double scale = 0.0;
    for (uint32_t k = 0; k < s->n_spheres; ++k)
        for (int a = 0; a < 3; ++a) scale = std::max(scale, fabs(s->spheres[4 * k + a]) + fabs(s->spheres[4 * k + 3]));
    const double iso_margin = std::is_same<R, float>::value ? 1e-2 + 1e-5 * scale : 1e-6 + 1e-12 * scale;
    const std::vector<uint8_t> iso = rtw::isolated_spheres(s->spheres, s->n_spheres, bb, iso_margin);
    const rtw::Bvh4Build b4 = rtw::collapse_bvh4(bb);
    const size_t o_nodes4 = reserve(sizeof(rtw::Bvh4Node<R>) * 8 * b4.nodes.size());
    // BVH over the light spheres for the light pdf (a query for EVERY light
    // the ray hits, so boxes only cull; the sum itself keeps list order in f64)
    const rtw::BvhBuild lb = rtw::build_bvh(s->lights, s->n_lights,
                                            std::is_same<R, float>::value ? 1e-5 : 1e-12, light_leaf);
    const size_t o_lnodes = reserve(sizeof(rtw::BvhNode<R>) * lb.nodes.size());
    const size_t o_lsph = reserve(sizeof(R4) * s->n_lights);
    const size_t o_lid = reserve(sizeof(uint32_t) * s->n_lights);
    // uniform grid over the light spheres (grid_density cells per light; 0: none)
    const rtw::LightGrid lg = grid_density > 0 ? rtw::build_light_grid(s->lights, s->n_lights, grid_density)
                                               : rtw::LightGrid{};
    const size_t o_lgs = reserve(sizeof(uint32_t) * lg.start.size());
    const size_t o_lgsph = reserve(sizeof(R4) * lg.items.size());
    const size_t o_lgid = reserve(sizeof(uint32_t) * lg.items.size());
    // f64: the grid's lights rounded to f32 with |r| -- the f64 kernels' walk runs
    // in f32 on them (light_pdf.hpp lights_pdf_grid_coop64)
    const size_t o_lgsph32 = reserve(std::is_same<R, double>::value ? sizeof(rtw::R4<float>) * lg.items.size() : 0);
    // the cells' records (light_grid.hpp light_grid_walk_piece_rec): 64 B per cell
    const size_t n_cells = lg.start.empty() ? 0 : lg.start.size() - 1;
    const size_t o_lgrec = reserve(sizeof(rtw::R4<float>) * rtw::kGridRecSlots * n_cells);
    std::vector<unsigned char> blob(align_up(off, 64) + 64, 0);
    unsigned char* b = blob.data();
    for (uint32_t k = 0; k < s->n_spheres; ++k) {
        const double* p = s->spheres + 4 * k;
        R r = (R)p[3];
        // a negative radius inverts the sphere's AABB, which bounded_hit never
        // passes (sphere.rs:42-45): r^2 = -inf makes the discriminant -inf
        reinterpret_cast<R4*>(b + o_sph)[k] = R4{(R)p[0], (R)p[1], (R)p[2], p[3] < 0 ? (R)-INFINITY : r * r};
        reinterpret_cast<R*>(b + o_r)[k] = r;
        if (k64)
            for (int a = 0; a < 4; ++a) reinterpret_cast<double*>(b + o_s64)[4 * k + a] = p[a];
        const uint32_t m = s->sphere_mat[k], t = s->mat_type[m];
        reinterpret_cast<uint32_t*>(b + o_smat)[k] = m | (t << 24);
        const double* mp = s->mat_params + 5 * m;
        const double w = t == RTW_METAL ? mp[3] : (t == RTW_DIELECTRIC ? mp[4] : 0.0);
        reinterpret_cast<R4*>(b + o_sshade)[k] = R4{(R)mp[0], (R)mp[1], (R)mp[2], (R)w};
    }
    for (uint32_t k = 0; k < s->n_spheres; ++k)
        if (iso[k]) reinterpret_cast<uint32_t*>(b + o_smat)[k] |= 0x80000000u;
    for (uint32_t k = 0; k < s->n_planes; ++k) {
        // {point, normal, AABB lo, AABB hi}: Plane::get_aabbox (plane.rs:218-242)
        // pins the normal axis at 0 and leaves the others infinite
        const double* pl = s->planes + 6 * k;
        const double e = 2.220446049250313080847e-16;
        const bool fx = fabs(pl[5]) < e && fabs(pl[4]) < e, fy = fabs(pl[3]) < e && fabs(pl[5]) < e,
                   fz = fabs(pl[3]) < e && fabs(pl[4]) < e;
        const double box[6] = {fx ? 0.0 : -INFINITY, fy ? 0.0 : -INFINITY, fz ? 0.0 : -INFINITY,
                               fx ? 0.0 : INFINITY, fy ? 0.0 : INFINITY, fz ? 0.0 : INFINITY};
        R* dst = reinterpret_cast<R*>(b + o_pl) + rtw::kPlaneR * k;
        for (int q = 0; q < 6; ++q) dst[q] = (R)pl[q];
        for (int q = 0; k64 && q < 3; ++q) {
            reinterpret_cast<double*>(b + o_pl64)[8 * k + q] = pl[q];
            reinterpret_cast<double*>(b + o_pl64)[8 * k + 4 + q] = pl[3 + q];
        }
        for (int q = 0; q < 6; ++q) dst[6 + q] = (R)box[q];
        // Plane::get_plane_uv's constants (plane.rs:40-54), computed as the
        // oracle's plane_uv does: theta = atan2(|n x V|, n . V), V = (0, 1, 0)
        const double c[3] = {pl[4] * 0.0 - pl[5] * 1.0, pl[5] * 0.0 - pl[3] * 0.0, pl[3] * 1.0 - pl[4] * 0.0};
        const double clen = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        const double theta = atan2(clen, pl[3] * 0.0 + pl[4] * 1.0 + pl[5] * 0.0);
        const double kv[3] = {c[0] / clen, c[1] / clen, c[2] / clen};
        const bool kfin = std::isfinite(kv[0]) && std::isfinite(kv[1]) && std::isfinite(kv[2]);
        dst[12] = theta <= e ? (R)0 : (kfin ? (R)1 : (R)2);
        dst[13] = (R)cos(theta);
        dst[14] = (R)sin(theta);
        for (int q = 0; q < 3; ++q) dst[15 + q] = kfin ? (R)kv[q] : (R)0;
        dst[18] = dst[19] = (R)0;
    }
    for (uint32_t k = 0; k < s->n_planes; ++k) reinterpret_cast<uint32_t*>(b + o_pmat)[k] = s->plane_mat[k];
    // an f64 record's AABB (lo at lo_at, hi at hi_at) rounded outward into R (a cull only)
    auto outward = [](const double* src, R* dst, uint32_t lo_at, uint32_t hi_at) {
        for (int a = 0; a < 3; ++a) {
            dst[lo_at + a] = round_down<R>(src[lo_at + a]);
            dst[hi_at + a] = round_up<R>(src[hi_at + a]);
        }
    };
    // quads: derived in f64
    auto put_quad = [&](const double* src, R* dst) {
        double q[rtw::kQuadR];
        quad_derive(src, q);
        for (uint32_t a = 0; a < rtw::kQuadR; ++a) dst[a] = (R)q[a];
        outward(q, dst, 16, 19);
    };
    for (uint32_t k = 0; k < s->n_quads; ++k) {
        put_quad(s->quads + 9 * k, reinterpret_cast<R*>(b + o_quads) + rtw::kQuadR * k);
        reinterpret_cast<uint32_t*>(b + o_qmat)[k] = s->quad_mat[k];
    }
    for (uint32_t k = 0; k < s->n_light_quads; ++k)
        put_quad(s->light_quads + 9 * k, reinterpret_cast<R*>(b + o_lquads) + rtw::kQuadR * k);
    for (uint32_t k = 0; k < s->n_boxes; ++k) {
        double bx[rtw::kBoxR];
        box_derive(s->boxes + 18 * k, bx);
        R* dst = reinterpret_cast<R*>(b + o_boxes) + rtw::kBoxR * k;
        for (uint32_t a = 0; a < rtw::kBoxR; ++a) dst[a] = (R)bx[a];
        outward(bx, dst, rtw::kBoxLo, rtw::kBoxHi);
        for (uint32_t qd = 0; qd < 6; ++qd) outward(bx, dst, rtw::kQuadR * qd + 16, rtw::kQuadR * qd + 19);
        reinterpret_cast<uint32_t*>(b + o_bmat)[k] = s->box_mat[k];
    }
    {
        uint32_t ns = 0, nq = 0;
        for (uint32_t k = 0; k < n_list; ++k) {
            const uint32_t kind = s->light_kinds ? s->light_kinds[k] : (k >= s->n_lights ? 1u : 0u);
            reinterpret_cast<uint32_t*>(b + o_lref)[k] =
                kind == RTW_LIGHT_QUAD ? (rtw::kLrefQuad | nq++) : (kind == RTW_LIGHT_DEFAULT ? rtw::kLrefDefault : ns++);
        }
    }
    if (tex) {
        for (uint32_t k = 0; k < s->n_materials; ++k) reinterpret_cast<uint32_t*>(b + o_mtex)[k] = s->mat_tex[k];
        for (uint32_t k = 0; k < s->n_textures; ++k) {
            const double* tp = s->tex_params + 4 * k;
            reinterpret_cast<uint32_t*>(b + o_ttype)[k] = s->tex_type[k];
            reinterpret_cast<R4*>(b + o_tp)[k] = R4{(R)tp[0], (R)tp[1], (R)tp[2], (R)tp[3]};
            reinterpret_cast<uint32_t*>(b + o_trefs)[2 * k] = s->tex_refs[2 * k];
            reinterpret_cast<uint32_t*>(b + o_trefs)[2 * k + 1] = s->tex_refs[2 * k + 1];
        }
        for (uint32_t k = 0; k < 256 * s->n_perlin; ++k) {
            const double* v = s->perlin_vec + 3 * k;
            reinterpret_cast<R4*>(b + o_pvec)[k] = R4{(R)v[0], (R)v[1], (R)v[2], (R)0};
        }
        for (uint32_t k = 0; k < 768 * s->n_perlin; ++k)
            reinterpret_cast<uint32_t*>(b + o_pperm)[k] = s->perlin_perm[k];
    }
    ds->mat_tex = tex ? reinterpret_cast<const uint32_t*>(base + o_mtex) : nullptr;
    ds->tex_type = reinterpret_cast<const uint32_t*>(base + o_ttype);
    ds->tex_p = reinterpret_cast<const R4*>(base + o_tp);
    ds->tex_refs = reinterpret_cast<const uint32_t*>(base + o_trefs);
    ds->perlin_vec = reinterpret_cast<const R4*>(base + o_pvec);
    ds->perlin_perm = reinterpret_cast<const uint32_t*>(base + o_pperm);
    ds->light_flags = s->light_flags;
    ds->emissive = 0;
    for (uint32_t k = 0; k < s->n_materials; ++k)
        if (s->mat_type[k] == RTW_DIFFUSE_LIGHT) ds->emissive = 1;
    for (uint32_t k = 0; k < s->n_materials; ++k) {
        const double* m = s->mat_params + 5 * k;
        const uint32_t t = s->mat_type[k];
        // the f64 scatter constants of kOptHit64 (dielectric_dir64): Dialectric's
        // index_of_refraction.recip() and reflectance's r0 for both faces, with the
        // reference's operations (material.rs:450-454, 464-468); Metal's fuzz
        double* m64 = reinterpret_cast<double*>(b + o_m64) + 4 * k;
        if (t == RTW_DIELECTRIC) {
            const double ior = m[4], rf = 1.0 / ior;
            const double r0f = (1.0 - rf) / (1.0 + rf), r0b = (1.0 - ior) / (1.0 + ior);
            m64[0] = rf;
            m64[1] = r0f * r0f;
            m64[2] = r0b * r0b;
            m64[3] = ior;
        } else {
            m64[0] = m64[1] = m64[2] = 0.0;
            m64[3] = t == RTW_METAL ? m[3] : 0.0;
        }
        reinterpret_cast<uint32_t*>(b + o_mt)[k] = t;
        const double w = t == RTW_METAL ? m[3] : (t == RTW_DIELECTRIC ? m[4] : 0.0);
        reinterpret_cast<R4*>(b + o_mp)[k] = R4{(R)m[0], (R)m[1], (R)m[2], (R)w};
    }
    for (uint32_t k = 0; k < s->n_lights; ++k) {
        const double* p = s->lights + 4 * k;
        reinterpret_cast<R4*>(b + o_li)[k] = R4{(R)p[0], (R)p[1], (R)p[2], (R)p[3]};
    }
    ds->sph = reinterpret_cast<const R4*>(base + o_sph);
    ds->sph_r = reinterpret_cast<const R*>(base + o_r);
    ds->sph64 = reinterpret_cast<const rtw::R4<double>*>(base + o_s64);
    ds->pl64 = reinterpret_cast<const rtw::R4<double>*>(base + o_pl64);
    ds->mat64 = reinterpret_cast<const rtw::R4<double>*>(base + o_m64);
    ds->sph_mat = reinterpret_cast<const uint32_t*>(base + o_smat);
    ds->sph_shade = reinterpret_cast<const R4*>(base + o_sshade);
    ds->planes = reinterpret_cast<const R*>(base + o_pl);
    ds->plane_mat = reinterpret_cast<const uint32_t*>(base + o_pmat);
    ds->mat_type = reinterpret_cast<const uint32_t*>(base + o_mt);
    ds->mat_p = reinterpret_cast<const R4*>(base + o_mp);
    ds->lights = reinterpret_cast<const R4*>(base + o_li);
    ds->quads = reinterpret_cast<const R*>(base + o_quads);
    ds->quad_mat = reinterpret_cast<const uint32_t*>(base + o_qmat);
    ds->lquads = reinterpret_cast<const R*>(base + o_lquads);
    ds->lref = (s->n_light_quads || s->n_light_other) ? reinterpret_cast<const uint32_t*>(base + o_lref) : nullptr;
    ds->n_quads = s->n_quads;
    ds->n_lquads = s->n_light_quads;
    ds->n_list = n_list;
    ds->boxes = reinterpret_cast<const R*>(base + o_boxes);
    ds->box_mat = reinterpret_cast<const uint32_t*>(base + o_bmat);
    ds->n_boxes = s->n_boxes;
    // box bounds round outward into precision R
    for (size_t k = 0; k < bb.nodes.size(); ++k)
        reinterpret_cast<rtw::BvhNode<R>*>(b + o_nodes)[k] = pack_node<R>(bb.nodes[k]);
    if constexpr (std::is_same<R, double>::value)
        for (size_t k = 0; k < bb.nodes.size(); ++k)
            reinterpret_cast<rtw::BvhNode<float>*>(b + o_nodes32)[k] = pack_node<float>(bb.nodes[k]);
    for (uint32_t k = 0; k < s->n_spheres; ++k) {
        const uint32_t id = bb.order[k];
        const R4 sk = reinterpret_cast<const R4*>(b + o_sph)[id];
        reinterpret_cast<R4*>(b + o_bsph)[k] = sk;
        reinterpret_cast<uint32_t*>(b + o_bid)[k] = id;
        if constexpr (std::is_same<R, double>::value)
            reinterpret_cast<rtw::R4<float>*>(b + o_bsph32)[k] =
                rtw::R4<float>{(float)sk.x, (float)sk.y, (float)sk.z, (float)sk.w};
    }
    // 4-wide tree, one copy per ray octant: slots in that octant's
    // front-to-back order, slab planes pre-selected as near/far (see Bvh4Node)
    const size_t n4 = b4.nodes.size();
    for (int oct = 0; oct < 8; ++oct) {
        for (size_t k = 0; k < n4; ++k) {
            const rtw::Bvh4Build::Node& n = b4.nodes[k];
            rtw::Bvh4Node<R> d{};
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t slot = n.order[oct][q];
                const bool valid = q < n.n;
                R nr[3], fr[3];
                for (int a = 0; a < 3; ++a) {
                    const bool neg = (oct >> a) & 1;
                    const R lo = valid ? round_down<R>(n.lo[slot][a]) : (R)INFINITY;
                    const R hi = valid ? round_up<R>(n.hi[slot][a]) : (R)-INFINITY;
                    // a ray going -a enters through hi and leaves through lo;
                    // an empty slot maps to near = +inf, far = -inf in ray space
                    nr[a] = neg ? hi : lo;
                    fr[a] = neg ? lo : hi;
                }
                const int32_t link = valid ? n.child[slot] : rtw::leaf_code(0, 0);
                R lr = 0;   // the link's bits in an R slot (low 32 bits for double)
                if constexpr (sizeof(R) == 4) {
                    memcpy(&lr, &link, 4);
                } else {
                    const int64_t l64 = (int64_t)(uint32_t)link;
                    memcpy(&lr, &l64, 8);
                }
                d.a[q] = rtw::R4<R>{nr[0], nr[1], nr[2], fr[0]};
                d.b[q] = rtw::R4<R>{fr[1], fr[2], lr, (R)0};
            }
            reinterpret_cast<rtw::Bvh4Node<R>*>(b + o_nodes4)[oct * n4 + k] = d;
        }
    }
    for (size_t k = 0; k < lb.nodes.size(); ++k)
        reinterpret_cast<rtw::BvhNode<R>*>(b + o_lnodes)[k] = pack_node<R>(lb.nodes[k]);
    for (uint32_t k = 0; k < s->n_lights; ++k) {
        const uint32_t id = lb.order[k];
        reinterpret_cast<R4*>(b + o_lsph)[k] = reinterpret_cast<const R4*>(b + o_li)[id];
        reinterpret_cast<uint32_t*>(b + o_lid)[k] = id;
    }
    ds->lbvh = reinterpret_cast<const rtw::BvhNode<R>*>(base + o_lnodes);
    ds->lsph = reinterpret_cast<const R4*>(base + o_lsph);
    ds->lid = reinterpret_cast<const uint32_t*>(base + o_lid);
    ds->n_lnodes = (uint32_t)lb.nodes.size();
    ds->lbvh_depth = lb.depth;
    if (!lg.start.empty())
        memcpy(b + o_lgs, lg.start.data(), sizeof(uint32_t) * lg.start.size());
    for (size_t k = 0; k < lg.items.size(); ++k) {
        const uint32_t id = lg.items[k];
        reinterpret_cast<R4*>(b + o_lgsph)[k] = reinterpret_cast<const R4*>(b + o_li)[id];
        reinterpret_cast<uint32_t*>(b + o_lgid)[k] = id;
        if constexpr (std::is_same<R, double>::value) {
            const double* l = s->lights + 4 * (size_t)id;
            reinterpret_cast<rtw::R4<float>*>(b + o_lgsph32)[k] =
                rtw::R4<float>{(float)l[0], (float)l[1], (float)l[2], fabsf((float)l[3])};
        }
    }
    if (n_cells) {   // each cell's lights as the f32 walk reads them (f32: lg_sph; f64: lg_sph32)
        const std::vector<float> rec = rtw::light_grid_records(lg, s->lights, std::is_same<R, double>::value);
        memcpy(b + o_lgrec, rec.data(), sizeof(float) * rec.size());
    }
    ds->lg_rec = reinterpret_cast<const rtw::R4<float>*>(base + o_lgrec);
    ds->lg_start = reinterpret_cast<const uint32_t*>(base + o_lgs);
    ds->lg_sph = reinterpret_cast<const R4*>(base + o_lgsph);
    ds->lg_id = reinterpret_cast<const uint32_t*>(base + o_lgid);
    for (int a = 0; a < 3; ++a) {
        ds->lg_lo[a] = (R)lg.lo[a];
        ds->lg_hi[a] = (R)(lg.lo[a] + lg.n[a] * lg.cell[a]);
        ds->lg_cell[a] = (R)lg.cell[a];
        ds->lg_inv[a] = (R)(1.0 / lg.cell[a]);
        ds->lg_n[a] = lg.n[a];
    }
    ds->lg_big = lg.n_big;
    ds->lg_on = lg.start.empty() ? 0u : 1u;
    ds->bvh4 = reinterpret_cast<const rtw::Bvh4Node<R>*>(base + o_nodes4);
    ds->n_nodes4 = (uint32_t)n4;
    ds->bvh4_stack = b4.max_stack;
    ds->bvh = reinterpret_cast<const rtw::BvhNode<R>*>(base + o_nodes);
    if constexpr (std::is_same<R, double>::value) {
        ds->bvh32 = reinterpret_cast<const rtw::BvhNode<float>*>(base + o_nodes32);
        ds->bsph32 = reinterpret_cast<const rtw::R4<float>*>(base + o_bsph32);
        ds->lg_sph32 = reinterpret_cast<const rtw::R4<float>*>(base + o_lgsph32);
    }
    ds->bsph = reinterpret_cast<const R4*>(base + o_bsph);
    ds->bid = reinterpret_cast<const uint32_t*>(base + o_bid);
    ds->n_sph = s->n_spheres;
    ds->n_planes = s->n_planes;
    ds->n_mat = s->n_materials;
    ds->n_lights = s->n_lights;
    ds->n_nodes = (uint32_t)bb.nodes.size();
    ds->bvh_depth = bb.depth;
    if (keep_bvh) *keep_bvh = bb;
    return blob;
}

template std::vector<unsigned char> stage_scene<float>(const rtw_scene*, DevScene<float>*, uintptr_t, uint32_t,
                                                       uint32_t, double, BvhBuild*);
template std::vector<unsigned char> stage_scene<double>(const rtw_scene*, DevScene<double>*, uintptr_t, uint32_t,
                                                        uint32_t, double, BvhBuild*);

int validate_scene(const rtw_scene* s, std::string* msg) {
    auto fail = [msg](int code, const char* text) {
        *msg = text;
        return code;
    };
    if (!s) return fail(RTW_E_INVALID, "scene is NULL");
    if ((s->n_spheres && (!s->spheres || !s->sphere_mat)) || (s->n_planes && (!s->planes || !s->plane_mat)) ||
        (s->n_materials && (!s->mat_type || !s->mat_params)) || (s->n_lights && !s->lights) ||
        (s->n_quads && (!s->quads || !s->quad_mat)) || (s->n_light_quads && !s->light_quads) ||
        (s->n_boxes && (!s->boxes || !s->box_mat)))
        return fail(RTW_E_INVALID, "scene array pointer is NULL");
    const uint32_t n_list = s->n_lights + s->n_light_quads + s->n_light_other;
    if (s->light_kinds) {
        uint32_t cnt[3] = {0, 0, 0};
        for (uint32_t k = 0; k < n_list; ++k) {
            if (s->light_kinds[k] > RTW_LIGHT_DEFAULT) return fail(RTW_E_INVALID, "unknown light kind");
            ++cnt[s->light_kinds[k]];
        }
        if (cnt[0] != s->n_lights || cnt[1] != s->n_light_quads || cnt[2] != s->n_light_other)
            return fail(RTW_E_INVALID, "light_kinds does not match the light counts");
    } else if (s->n_light_other) {
        return fail(RTW_E_INVALID, "n_light_other needs light_kinds");
    }
    if (s->light_flags & ~(uint32_t)RTW_LIGHTS_BVH_LEAF) return fail(RTW_E_INVALID, "unknown light_flags");
    if ((s->light_flags & RTW_LIGHTS_BVH_LEAF) && n_list > 5)
        return fail(RTW_E_UNSUPPORTED, "a BVH light list of more than 5 entries is not a leaf: the reference's "
                                          "BVH aux_random indexes it inconsistently (bvh.rs:78-92)");
    for (uint32_t k = 0; k < s->n_materials; ++k)
        if (s->mat_type[k] > RTW_DIFFUSE_LIGHT) return fail(RTW_E_INVALID, "unknown material type");
    if (s->n_materials >= (1u << 24)) return fail(RTW_E_UNSUPPORTED, "more than 2^24 materials");
    if (s->mat_tex) {
        if ((s->n_textures && (!s->tex_type || !s->tex_params || !s->tex_refs)) ||
            (s->n_perlin && (!s->perlin_vec || !s->perlin_perm)))
            return fail(RTW_E_INVALID, "texture array pointer is NULL");
        for (uint32_t k = 0; k < s->n_materials; ++k)
            if (s->mat_tex[k] >= s->n_textures) return fail(RTW_E_INVALID, "material texture id out of range");
        for (uint32_t k = 0; k < s->n_textures; ++k) {
            const uint32_t t = s->tex_type[k];
            if (t > RTW_TEX_NOISE) return fail(RTW_E_INVALID, "unknown texture type");
            if (t == RTW_TEX_CHECKER && (s->tex_refs[2 * k] >= s->n_textures || s->tex_refs[2 * k + 1] >= s->n_textures))
                return fail(RTW_E_INVALID, "checker texture id out of range");
            if (t == RTW_TEX_NOISE && s->tex_refs[2 * k] >= s->n_perlin)
                return fail(RTW_E_INVALID, "noise texture Perlin table id out of range");
        }
        // nested checkers must bottom out (the reference's Arc<dyn Texture> tree)
        for (uint32_t k = 0; k < s->n_textures; ++k) {
            std::vector<uint32_t> stack{k};
            uint32_t steps = 0;
            while (!stack.empty()) {
                const uint32_t t = stack.back();
                stack.pop_back();
                if (++steps > 4096) return fail(RTW_E_INVALID, "checker textures form a cycle or are too deep");
                if (s->tex_type[t] == RTW_TEX_CHECKER) {
                    stack.push_back(s->tex_refs[2 * t]);
                    stack.push_back(s->tex_refs[2 * t + 1]);
                }
            }
        }
        for (uint32_t k = 0; k < 768 * s->n_perlin; ++k)
            if (s->perlin_perm[k] > 255) return fail(RTW_E_INVALID, "Perlin permutation entry > 255");
    }
    for (uint32_t k = 0; k < s->n_spheres; ++k)
        if (s->sphere_mat[k] >= s->n_materials) return fail(RTW_E_INVALID, "sphere material id out of range");
    for (uint32_t k = 0; k < s->n_planes; ++k)
        if (s->plane_mat[k] >= s->n_materials) return fail(RTW_E_INVALID, "plane material id out of range");
    for (uint32_t k = 0; k < s->n_quads; ++k)
        if (s->quad_mat[k] >= s->n_materials) return fail(RTW_E_INVALID, "quad material id out of range");
    for (uint32_t k = 0; k < s->n_boxes; ++k)
        if (s->box_mat[k] >= s->n_materials) return fail(RTW_E_INVALID, "box material id out of range");
    return RTW_OK;
}

template <typename R>
SceneScale scene_scale(const rtw_scene* s, const DevScene<R>& ds) {
    SceneScale sc;
    // the closest-hit working set (tree + leaf spheres + ids): what the lpt
    // heuristic weighs against an XCD's L2
    sc.tree_bytes = std::is_same<R, float>::value
                        ? (size_t)ds.n_nodes * sizeof(BvhNode<float>) + (size_t)ds.n_sph * (sizeof(R4<float>) + 4)
                        : (size_t)ds.n_nodes * (sizeof(BvhNode<double>) + sizeof(BvhNode<float>)) +
                              (size_t)ds.n_sph * (sizeof(R4<double>) + 4);
    // scale of the scene for the f32 test choice (plan_render)
    sc.extent = 0.0;
    sc.min_radius = INFINITY;
    for (uint32_t k = 0; k < s->n_spheres; ++k) {
        const double* q = s->spheres + 4 * k;
        const double r = fabs(q[3]);
        sc.extent = std::max(sc.extent, std::max(fabs(q[0]), std::max(fabs(q[1]), fabs(q[2]))) + r);
        if (r > 0) sc.min_radius = std::min(sc.min_radius, r);
    }
    for (uint32_t k = 0; k < s->n_lights; ++k) {
        const double r = fabs(s->lights[4 * k + 3]);
        if (r > 0) sc.min_radius = std::min(sc.min_radius, r);
    }
    return sc;
}
template SceneScale scene_scale<float>(const rtw_scene*, const DevScene<float>&);
template SceneScale scene_scale<double>(const rtw_scene*, const DevScene<double>&);

// auto leaf size: 4; 8 from 100k spheres (C5: +12 %); f64 with a tree too
// large for LDS (>= 4096 spheres): 2 -- its sphere tests are f64, its node
// tests f32 (C3 f64 1006 -> 998 ms: 2.8 -> 1.7 sphere tests and 7.2 -> 7.9
// node visits per segment; 3: 1003; C2's LDS tree and f32 lose with 2,
// profiles/r06t_ab_leaf_c3_f64.jsonl, r06u_ab_leaf.jsonl)
uint32_t auto_leaf(uint32_t bvh_leaf, uint32_t n_spheres, bool f64) {
    return bvh_leaf ? bvh_leaf : (n_spheres >= 100000 ? 8u : (f64 && n_spheres >= 4096 ? 2u : 4u));
}

}  // namespace rtw
