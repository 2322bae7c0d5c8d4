// denoise_variance_kernels.hpp -- the variance-guided a-trous filter of
// rtw_denoise_variance (include/rtw.h holds the filter operation by operation;
// the schedule is host/denoise_variance_plan.hpp's).  svgf_prepare_kernel turns
// the colour sums, the feature sums, the luminance moments and the counts into
// rtw_denoise's three 32-byte records per pixel plus a 16-byte variance record,
// svgf_atrous_kernel runs one iteration from one colour and variance array into
// the other; the finish is denoise.hip's denoise_finish_kernel, launched as it
// is on the same records.  Compiled by denoise_variance.hip alone, without FMA
// contraction: every operation is an f64 operation that rounds on its own, in
// the written order, whatever the context's precision.
//
// The records are denoise_kernels.hpp's (guide {Nx, Ny, Nz, d}, albedo {a0, a1,
// a2, flags}, colour {e0, e1, e2, state}) and
//   var     {ve, has_var}      ve: the variance of the mean of the irradiance's
//                              luminance (0 without has_var); has_var 1 or 0, fixed
//                              by the prepare kernel
// A tap is a source exactly when its colour state is 1, so a tap reads the
// colour record and, for a source, the guide and the variance records.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host/denoise_variance_plan.hpp"

namespace rtw {

struct SvgfPrepare {
    const void* sums;            // H*W*3 float or double
    const double* features;      // H*W*8
    const double2* moments;      // H*W {S1, S2}
    const uint32_t* counts;      // H*W, or null: spp
    uint32_t spp, demodulate;
    uint64_t pixels;
    double2 *guide, *albedo, *colour, *var;
};

struct SvgfAtrous {
    const double2* guide;
    const double2* src;          // the colour records of the iteration before
    const double2* var_src;      // ... and its variance records
    double2* dst;
    double2* var_dst;
    uint32_t W, H, step, m;      // m: normal_power_log2
    uint32_t fill;
    double sv2, eps, sigma_depth;
};

// the kernels denoise_variance.hip holds, as its launches name them
enum SvgfKernel { kSvgfPrepareF32, kSvgfPrepareF64, kSvgfAtrousDirect, kSvgfAtrousLds, kSvgfKernels };
constexpr const char* kSvgfKernelNames[kSvgfKernels] = {"svgf_prepare_kernel<float>", "svgf_prepare_kernel<double>",
                                                        "svgf_atrous_kernel<false>", "svgf_atrous_kernel<true>"};

// denoise_variance.hip: 0, or -1 when the launch failed
int launch_svgf_prepare(bool sums_f32, const SvgfPrepare& p, uint32_t blocks, hipStream_t stream);
int launch_svgf_atrous(const SvgfAtrous& p, const SvgfStep& s, hipStream_t stream);

// the kernels: for denoise_variance.hip alone (the C-ABI unit includes the host side only)
#ifdef RTW_SVGF_KERNELS
namespace dev {

struct SvRec {
    double x, y, z, w;
};

__device__ inline SvRec sv_load(const double2* a, size_t at) {
    const double2 lo = a[2 * at], hi = a[2 * at + 1];
    return SvRec{lo.x, lo.y, hi.x, hi.y};
}
__device__ inline void sv_store(double2* a, size_t at, const SvRec& r) {
    a[2 * at] = make_double2(r.x, r.y);
    a[2 * at + 1] = make_double2(r.z, r.w);
}
__device__ inline bool sv_finite(double v) { return fabs(v) < __builtin_huge_val(); }
// ((0.2126 x) + (0.7152 y)) + (0.0722 z)
__device__ inline double sv_luma(double x, double y, double z) {
    const double yr = 0.2126 * x, yg = 0.7152 * y, yb = 0.0722 * z;
    const double s = yr + yg;
    return s + yb;
}

// rtw_denoise's prepare, and the variance record
template <typename S>
__global__ void __launch_bounds__(kDenoiseBlock) svgf_prepare_kernel(SvgfPrepare p) {
    const uint64_t px = (uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x;
    if (px >= p.pixels) return;
    const S* s = reinterpret_cast<const S*>(p.sums) + px * 3;
    const double S0 = (double)s[0], S1 = (double)s[1], S2 = (double)s[2];
    const double2* f = reinterpret_cast<const double2*>(p.features) + px * 4;
    const double2 f01 = f[0], f23 = f[1], f45 = f[2], f67 = f[3];
    const double F[8] = {f01.x, f01.y, f23.x, f23.y, f45.x, f45.y, f67.x, f67.y};
    const double2 mom = p.moments[px];
    const uint32_t n = p.counts ? p.counts[px] : p.spp;
    const double nd = (double)n;
    bool guide_ok = n > 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) guide_ok = guide_ok && sv_finite(F[k]);
    SvRec g{0.0, 0.0, 0.0, 0.0}, a{1.0, 1.0, 1.0, 0.0}, c{0.0, 0.0, 0.0, 0.0};
    double ve = 0.0, has_var = 0.0;
    if (n > 0) {
        c.x = S0 / nd;
        c.y = S1 / nd;
        c.z = S2 / nd;
    }
    if (guide_ok) {
        const bool valid = sv_finite(c.x) && sv_finite(c.y) && sv_finite(c.z);
        double aY = 1.0;
        if (p.demodulate) {
            const double lo = 0.0009765625;   // 2^-10
            const double a0 = F[0] / nd, a1 = F[1] / nd, a2 = F[2] / nd;
            a.x = a0 > lo ? a0 : lo;
            a.y = a1 > lo ? a1 : lo;
            a.z = a2 > lo ? a2 : lo;
            aY = sv_luma(a.x, a.y, a.z);
        }
        a.w = valid ? 3.0 : 1.0;
        if (valid) {
            c.x = c.x / a.x;
            c.y = c.y / a.y;
            c.z = c.z / a.z;
        }
        c.w = valid ? 1.0 : 2.0;
        const double len = sqrt((F[3] * F[3] + F[4] * F[4]) + F[5] * F[5]);
        if (len > 0.0) {
            g.x = F[3] / len;
            g.y = F[4] / len;
            g.z = F[5] / len;
        }
        g.w = F[7] > 0.0 ? F[6] / F[7] : 0.0;
        // (a NaN variance would pass the "> 0" select as 0: the moments are asked first)
        if (valid && n > 1 && sv_finite(mom.x) && sv_finite(mom.y)) {
            const double m = mom.x / nd;
            const double q = mom.y / nd;
            double var = q - m * m;
            var = var > 0.0 ? var : 0.0;
            const double v = var / (nd - 1.0);
            const double e = v / (aY * aY);
            if (sv_finite(e)) {
                ve = e;
                has_var = 1.0;
            }
        }
    }
    sv_store(p.guide, px, g);
    sv_store(p.albedo, px, a);
    sv_store(p.colour, px, c);
    p.var[px] = make_double2(ve, has_var);
}

// One centre of one iteration: the arithmetic of both forms.  colour_at(i, j),
// guide_at(i, j) and var_at(i, j) read a pixel inside the image.  *vp: the
// centre's variance record, replaced by the iteration's.
template <typename LoadColour, typename LoadGuide, typename LoadVar>
__device__ inline SvRec svgf_filter_pixel(const SvgfAtrous& p, int i, int j, const SvRec& gp, const SvRec& cp,
                                          double2* vp, LoadColour colour_at, LoadGuide guide_at, LoadVar var_at) {
    if (cp.w == 0.0) return cp;   // not guide_ok: as it is
    const bool valid = cp.w == 1.0;
    const bool has_var = vp->y != 0.0;
    const bool p_zero = gp.x == 0.0 && gp.y == 0.0 && gp.z == 0.0;
    const double thr = p.sv2 * vp->x + p.eps;
    const double yp = sv_luma(cp.x, cp.y, cp.z);
    constexpr double h[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    double num0 = 0.0, num1 = 0.0, num2 = 0.0, den = 0.0, vnum = 0.0;
    const int step = (int)p.step;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qj = j + dy * step;
        if (qj < 0 || qj >= (int)p.H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qi = i + dx * step;
            if (qi < 0 || qi >= (int)p.W) continue;
            const SvRec cq = colour_at(qi, qj);
            if (cq.w != 1.0) continue;   // not a source (now)
            const SvRec gq = guide_at(qi, qj);
            const double2 vq = var_at(qi, qj);
            double wn;
            if (p_zero && gq.x == 0.0 && gq.y == 0.0 && gq.z == 0.0) {
                wn = 1.0;
            } else {
                double t = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                t = t > 0.0 ? t : 0.0;
                for (uint32_t e = 0; e < p.m; ++e) t = t * t;
                wn = t;
            }
            double wd;
            const double mx = gp.w > gq.w ? gp.w : gq.w;
            if (mx > 0.0) {
                const double r = fabs(gp.w - gq.w) / mx;
                const double x = r / p.sigma_depth;
                double u = 1.0 - x * x;
                u = u > 0.0 ? u : 0.0;
                wd = u * u;
            } else {
                wd = 1.0;
            }
            double wc = 1.0;
            if (has_var) {
                const double g = yp - sv_luma(cq.x, cq.y, cq.z);
                const double s = g * g;
                wc = 1.0 / (1.0 + s / thr);
            }
            const double w = (((h[dy + 2] * h[dx + 2]) * wn) * wd) * wc;
            num0 = num0 + w * cq.x;
            num1 = num1 + w * cq.y;
            num2 = num2 + w * cq.z;
            den = den + w;
            vnum = vnum + (w * w) * vq.x;
        }
    }
    if (valid || (p.fill && den > 0.0)) {
        if (has_var) vp->x = vnum / (den * den);
        return SvRec{num0 / den, num1 / den, num2 / den, 1.0};
    }
    return cp;
}

// One iteration: a workgroup filters a tile of kDenoiseTileW x kDenoiseTileH
// pixels, one per lane.  kLds: the tile and its 2 * step halo of guide, colour
// and variance records are staged into dynamic LDS once (pixels outside the
// image as zeros, which are no sources) and the taps read from there; otherwise
// the taps read global memory.
template <bool kLds>
__global__ void __launch_bounds__(kDenoiseTileW* kDenoiseTileH) svgf_atrous_kernel(SvgfAtrous p) {
    const int i = (int)(blockIdx.x * kDenoiseTileW + threadIdx.x), j = (int)(blockIdx.y * kDenoiseTileH + threadIdx.y);
    const bool inside = i < (int)p.W && j < (int)p.H;
    if constexpr (kLds) {
        extern __shared__ __attribute__((aligned(16))) unsigned char sv_smem[];
        const int halo = 2 * (int)p.step;
        const int tw = (int)kDenoiseTileW + 2 * halo, th = (int)kDenoiseTileH + 2 * halo;
        const int ox = (int)(blockIdx.x * kDenoiseTileW) - halo, oy = (int)(blockIdx.y * kDenoiseTileH) - halo;
        double2* l_guide = reinterpret_cast<double2*>(sv_smem);
        double2* l_colour = l_guide + 2 * tw * th;
        double2* l_var = l_colour + 2 * tw * th;
        const int tid = (int)(threadIdx.y * kDenoiseTileW + threadIdx.x);
        for (int idx = tid; idx < 2 * tw * th; idx += (int)(kDenoiseTileW * kDenoiseTileH)) {
            const int pos = idx >> 1, half = idx & 1;
            const int ly = pos / tw, lx = pos - ly * tw;
            const int gx = ox + lx, gy = oy + ly;
            const bool in = gx >= 0 && gx < (int)p.W && gy >= 0 && gy < (int)p.H;
            double2 g = make_double2(0.0, 0.0), c = make_double2(0.0, 0.0);
            if (in) {
                const size_t at = 2 * ((size_t)gy * p.W + gx) + half;
                g = p.guide[at];
                c = p.src[at];
            }
            l_guide[idx] = g;
            l_colour[idx] = c;
            if (half == 0) l_var[pos] = in ? p.var_src[(size_t)gy * p.W + gx] : make_double2(0.0, 0.0);
        }
        __syncthreads();
        if (!inside) return;
        auto colour_at = [&](int qi, int qj) { return sv_load(l_colour, (size_t)((qj - oy) * tw + (qi - ox))); };
        auto guide_at = [&](int qi, int qj) { return sv_load(l_guide, (size_t)((qj - oy) * tw + (qi - ox))); };
        auto var_at = [&](int qi, int qj) { return l_var[(qj - oy) * tw + (qi - ox)]; };
        double2 v = var_at(i, j);
        const SvRec out = svgf_filter_pixel(p, i, j, guide_at(i, j), colour_at(i, j), &v, colour_at, guide_at, var_at);
        sv_store(p.dst, (size_t)j * p.W + i, out);
        p.var_dst[(size_t)j * p.W + i] = v;
    } else {
        if (!inside) return;
        auto colour_at = [&](int qi, int qj) { return sv_load(p.src, (size_t)qj * p.W + qi); };
        auto guide_at = [&](int qi, int qj) { return sv_load(p.guide, (size_t)qj * p.W + qi); };
        auto var_at = [&](int qi, int qj) { return p.var_src[(size_t)qj * p.W + qi]; };
        double2 v = var_at(i, j);
        const SvRec out = svgf_filter_pixel(p, i, j, guide_at(i, j), colour_at(i, j), &v, colour_at, guide_at, var_at);
        sv_store(p.dst, (size_t)j * p.W + i, out);
        p.var_dst[(size_t)j * p.W + i] = v;
    }
}

}  // namespace dev
#endif  // RTW_SVGF_KERNELS

}  // namespace rtw
