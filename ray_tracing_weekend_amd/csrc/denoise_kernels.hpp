// denoise_kernels.hpp -- the edge-avoiding a-trous filter of rtw_denoise
// (include/rtw.h holds the filter operation by operation; the schedule is
// host/denoise_plan.hpp's).  denoise_prepare_kernel turns the colour sums, the
// feature sums and the counts into three 32-byte records per pixel,
// denoise_atrous_kernel runs one iteration from one colour array into the
// other, denoise_finish_kernel remodulates and counts.  Compiled by denoise.hip
// alone, without FMA contraction: every operation is an f64 operation that
// rounds on its own, in the written order, whatever the context's precision.
//
// The records (4 doubles, read and written as two 16-byte halves):
//   guide   {Nx, Ny, Nz, d}
//   albedo  {a0, a1, a2, flags}    flags 0: not guide_ok, 1: guide_ok, 3: and valid at the start
//   colour  {e0, e1, e2, state}    state 0: not guide_ok (e = the output), 1: valid (e = the
//                                  irradiance), 2: guide_ok, not valid (e = S / n)
// A tap is a source exactly when its colour state is 1, so a tap reads the
// colour record and, for a source, the guide record.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host/denoise_plan.hpp"

namespace rtw {

struct DenoisePrepare {
    const void* sums;            // H*W*3 float or double
    const double* features;      // H*W*8
    const uint32_t* counts;      // H*W, or null: spp
    uint32_t spp, demodulate;
    uint64_t pixels;
    double2 *guide, *albedo, *colour;
};

struct DenoiseAtrous {
    const double2* guide;
    const double2* src;          // the colour records of the iteration before
    double2* dst;
    uint32_t W, H, step, m;      // m: normal_power_log2
    uint32_t colour_on, fill;
    double sc2, sigma_depth;
};

struct DenoiseFinish {
    const double2* albedo;
    const double2* colour;
    double* out;                 // H*W*3 means
    uint64_t pixels;
    unsigned long long* counters;   // {filled, left non-finite}
};

// the kernels denoise.hip holds, as its launches name them
enum DenoiseKernel { kDnPrepareF32, kDnPrepareF64, kDnAtrousDirect, kDnAtrousLds, kDnFinish, kDnKernels };
constexpr const char* kDenoiseKernelNames[kDnKernels] = {
    "denoise_prepare_kernel<float>", "denoise_prepare_kernel<double>", "denoise_atrous_kernel<false>",
    "denoise_atrous_kernel<true>", "denoise_finish_kernel"};

// denoise.hip: 0, or -1 when the launch failed
int launch_denoise_prepare(bool sums_f32, const DenoisePrepare& p, uint32_t blocks, hipStream_t stream);
int launch_denoise_atrous(const DenoiseAtrous& p, const DenoiseStep& s, hipStream_t stream);
int launch_denoise_finish(const DenoiseFinish& p, uint32_t blocks, hipStream_t stream);

// the kernels: for denoise.hip alone (the C-ABI unit includes the host side only)
#ifdef RTW_DENOISE_KERNELS
namespace dev {

struct DnRec {
    double x, y, z, w;
};

__device__ inline DnRec dn_load(const double2* a, size_t at) {
    const double2 lo = a[2 * at], hi = a[2 * at + 1];
    return DnRec{lo.x, lo.y, hi.x, hi.y};
}
__device__ inline void dn_store(double2* a, size_t at, const DnRec& r) {
    a[2 * at] = make_double2(r.x, r.y);
    a[2 * at + 1] = make_double2(r.z, r.w);
}
__device__ inline bool dn_finite(double v) { return fabs(v) < __builtin_huge_val(); }

template <typename S>
__global__ void __launch_bounds__(kDenoiseBlock) denoise_prepare_kernel(DenoisePrepare p) {
    const uint64_t px = (uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x;
    if (px >= p.pixels) return;
    const S* s = reinterpret_cast<const S*>(p.sums) + px * 3;
    const double S0 = (double)s[0], S1 = (double)s[1], S2 = (double)s[2];
    const double2* f = reinterpret_cast<const double2*>(p.features) + px * 4;
    const double2 f01 = f[0], f23 = f[1], f45 = f[2], f67 = f[3];
    const double F[8] = {f01.x, f01.y, f23.x, f23.y, f45.x, f45.y, f67.x, f67.y};
    const uint32_t n = p.counts ? p.counts[px] : p.spp;
    const double nd = (double)n;
    bool guide_ok = n > 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) guide_ok = guide_ok && dn_finite(F[k]);
    DnRec g{0.0, 0.0, 0.0, 0.0}, a{1.0, 1.0, 1.0, 0.0}, c{0.0, 0.0, 0.0, 0.0};
    if (n > 0) {
        c.x = S0 / nd;
        c.y = S1 / nd;
        c.z = S2 / nd;
    }
    if (guide_ok) {
        const bool valid = dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z);
        if (p.demodulate) {
            const double lo = 0.0009765625;   // 2^-10
            const double a0 = F[0] / nd, a1 = F[1] / nd, a2 = F[2] / nd;
            a.x = a0 > lo ? a0 : lo;
            a.y = a1 > lo ? a1 : lo;
            a.z = a2 > lo ? a2 : lo;
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
    }
    dn_store(p.guide, px, g);
    dn_store(p.albedo, px, a);
    dn_store(p.colour, px, c);
}

// One centre of one iteration: the arithmetic of both forms.  colour_at(i, j)
// and guide_at(i, j) read a pixel inside the image.
template <typename LoadColour, typename LoadGuide>
__device__ inline DnRec denoise_filter_pixel(const DenoiseAtrous& p, int i, int j, const DnRec& gp, const DnRec& cp,
                                             LoadColour colour_at, LoadGuide guide_at) {
    if (cp.w == 0.0) return cp;   // not guide_ok: as it is
    const bool valid = cp.w == 1.0;
    const bool colour = p.colour_on && valid;
    const bool p_zero = gp.x == 0.0 && gp.y == 0.0 && gp.z == 0.0;
    constexpr double h[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    double num0 = 0.0, num1 = 0.0, num2 = 0.0, den = 0.0;
    const int step = (int)p.step;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qj = j + dy * step;
        if (qj < 0 || qj >= (int)p.H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qi = i + dx * step;
            if (qi < 0 || qi >= (int)p.W) continue;
            const DnRec cq = colour_at(qi, qj);
            if (cq.w != 1.0) continue;   // not a source (now)
            const DnRec gq = guide_at(qi, qj);
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
            if (colour) {
                const double g0 = cp.x - cq.x, g1 = cp.y - cq.y, g2 = cp.z - cq.z;
                const double s = (g0 * g0 + g1 * g1) + g2 * g2;
                wc = 1.0 / (1.0 + s / p.sc2);
            }
            const double w = (((h[dy + 2] * h[dx + 2]) * wn) * wd) * wc;
            num0 = num0 + w * cq.x;
            num1 = num1 + w * cq.y;
            num2 = num2 + w * cq.z;
            den = den + w;
        }
    }
    if (valid || (p.fill && den > 0.0)) return DnRec{num0 / den, num1 / den, num2 / den, 1.0};
    return cp;
}

// One iteration: a workgroup filters a tile of kDenoiseTileW x kDenoiseTileH
// pixels, one per lane.  kLds: the tile and its 2 * step halo of guide and
// colour records are staged into dynamic LDS once (pixels outside the image as
// zeros, which are no sources) and the taps read from there; otherwise the taps
// read global memory.
template <bool kLds>
__global__ void __launch_bounds__(kDenoiseTileW* kDenoiseTileH) denoise_atrous_kernel(DenoiseAtrous p) {
    const int i = (int)(blockIdx.x * kDenoiseTileW + threadIdx.x), j = (int)(blockIdx.y * kDenoiseTileH + threadIdx.y);
    const bool inside = i < (int)p.W && j < (int)p.H;
    if constexpr (kLds) {
        extern __shared__ __attribute__((aligned(16))) unsigned char dn_smem[];
        const int halo = 2 * (int)p.step;
        const int tw = (int)kDenoiseTileW + 2 * halo, th = (int)kDenoiseTileH + 2 * halo;
        const int ox = (int)(blockIdx.x * kDenoiseTileW) - halo, oy = (int)(blockIdx.y * kDenoiseTileH) - halo;
        double2* l_guide = reinterpret_cast<double2*>(dn_smem);
        double2* l_colour = l_guide + 2 * tw * th;
        const int tid = (int)(threadIdx.y * kDenoiseTileW + threadIdx.x);
        for (int idx = tid; idx < 2 * tw * th; idx += (int)(kDenoiseTileW * kDenoiseTileH)) {
            const int pos = idx >> 1, half = idx & 1;
            const int ly = pos / tw, lx = pos - ly * tw;
            const int gx = ox + lx, gy = oy + ly;
            double2 g = make_double2(0.0, 0.0), c = make_double2(0.0, 0.0);
            if (gx >= 0 && gx < (int)p.W && gy >= 0 && gy < (int)p.H) {
                const size_t at = 2 * ((size_t)gy * p.W + gx) + half;
                g = p.guide[at];
                c = p.src[at];
            }
            l_guide[idx] = g;
            l_colour[idx] = c;
        }
        __syncthreads();
        if (!inside) return;
        auto colour_at = [&](int qi, int qj) { return dn_load(l_colour, (size_t)((qj - oy) * tw + (qi - ox))); };
        auto guide_at = [&](int qi, int qj) { return dn_load(l_guide, (size_t)((qj - oy) * tw + (qi - ox))); };
        const DnRec out = denoise_filter_pixel(p, i, j, guide_at(i, j), colour_at(i, j), colour_at, guide_at);
        dn_store(p.dst, (size_t)j * p.W + i, out);
    } else {
        if (!inside) return;
        auto colour_at = [&](int qi, int qj) { return dn_load(p.src, (size_t)qj * p.W + qi); };
        auto guide_at = [&](int qi, int qj) { return dn_load(p.guide, (size_t)qj * p.W + qi); };
        const DnRec out = denoise_filter_pixel(p, i, j, guide_at(i, j), colour_at(i, j), colour_at, guide_at);
        dn_store(p.dst, (size_t)j * p.W + i, out);
    }
}

// The means: a valid pixel's irradiance times its albedo, any other pixel's
// colour record as it is.  Each wave counts its filled pixels (guide_ok, not
// valid at the start, valid now) and its pixels with a non-finite output by
// ballot and popcount, and its first lane adds them.
__global__ void __launch_bounds__(kDenoiseBlock) denoise_finish_kernel(DenoiseFinish p) {
    const uint64_t px = (uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x;
    bool filled = false, left = false;
    if (px < p.pixels) {
        const DnRec a = dn_load(p.albedo, px), c = dn_load(p.colour, px);
        double o0 = c.x, o1 = c.y, o2 = c.z;
        if (c.w == 1.0) {
            o0 = c.x * a.x;
            o1 = c.y * a.y;
            o2 = c.z * a.z;
        }
        double* out = p.out + px * 3;
        out[0] = o0;
        out[1] = o1;
        out[2] = o2;
        filled = a.w == 1.0 && c.w == 1.0;
        left = !(dn_finite(o0) && dn_finite(o1) && dn_finite(o2));
    }
    const unsigned long long mf = __ballot(filled), ml = __ballot(left);
    if ((threadIdx.x & 63) == 0) {
        if (mf) atomicAdd(&p.counters[0], (unsigned long long)__popcll(mf));
        if (ml) atomicAdd(&p.counters[1], (unsigned long long)__popcll(ml));
    }
}

}  // namespace dev
#endif  // RTW_DENOISE_KERNELS

}  // namespace rtw
