// path_kernel.hpp -- the two ends of a path segment that the megakernel holds
// inline, as batched queries, one ray per lane:
//   camera_rays_kernel<R>                Camera::get_ray (camera.rs:274-293) for chosen
//                                        pixels and one sample index, with the stream's
//                                        state after its draws
//   shade_rays_kernel<R, path, robust>   one iteration of ray_colour_tail_call after
//                                        world.hit (camera.rs:480-521): emitted, scatter,
//                                        the MixturePdf direction, its pdf value and
//                                        scattering_pdf; RNG state in, RNG state out
// With hit_rays_kernel between them a caller's loop is a wavefront path tracer.
// Both call the render kernel's device functions (rtw_device.hpp, render_kernel.hpp,
// light_pdf.hpp): per lane the words drawn and the operations are render_kernel's
// bounce, so the f64 results are its bits.  The bounce reads no world geometry: the
// record of rtw_hit_rays, the material and texture tables and the light list.
//
// Divergence: Metal and Dialectric run in one pass (f64: specular_dir64), the
// Lambertian lanes draw their directions, and only then the light pdf is taken --
// every Lambertian lane of the wave walks the list together.
// Memory: each record is read and written with the widest aligned accesses its
// stride allows (path_kernels.h record_align); the 32-byte RNG state stays in
// registers between its load and its store.
#pragma once

#include "path_kernels.h"
#include "query_kernel.hpp"

namespace rtw {

namespace dev {

// kN values of a record whose array starts kAlign-byte aligned and whose stride
// allows kAlign-byte accesses (record_align), from / to element offset 0 of the record
template <uint32_t kAlign, typename T, int kN>
__device__ __forceinline__ void load_rec(const T* __restrict__ p, T (&v)[kN]) {
    constexpr int kPer = (int)(kAlign / sizeof(T));
    if constexpr (kPer >= 2) {
        typedef T VT __attribute__((ext_vector_type(kPer)));
        constexpr int kFull = kN / kPer * kPer;
#pragma unroll
        for (int q = 0; q < kFull; q += kPer) {
            const VT x = *reinterpret_cast<const VT*>(p + q);
#pragma unroll
            for (int e = 0; e < kPer; ++e) v[q + e] = x[e];
        }
#pragma unroll
        for (int q = kFull; q < kN; ++q) v[q] = p[q];
    } else {
#pragma unroll
        for (int q = 0; q < kN; ++q) v[q] = p[q];
    }
}
template <uint32_t kAlign, typename T, int kN>
__device__ __forceinline__ void store_rec(T* __restrict__ p, const T (&v)[kN]) {
    constexpr int kPer = (int)(kAlign / sizeof(T));
    if constexpr (kPer >= 2) {
        typedef T VT __attribute__((ext_vector_type(kPer)));
        constexpr int kFull = kN / kPer * kPer;
#pragma unroll
        for (int q = 0; q < kFull; q += kPer) {
            VT x;
#pragma unroll
            for (int e = 0; e < kPer; ++e) x[e] = v[q + e];
            *reinterpret_cast<VT*>(p + q) = x;
        }
#pragma unroll
        for (int q = kFull; q < kN; ++q) p[q] = v[q];
    } else {
#pragma unroll
        for (int q = 0; q < kN; ++q) p[q] = v[q];
    }
}

// HittableList::pdf_value of the light list on the plan's light path
// (hittable_list.rs:408-412): the walk, / len, and the BVH-leaf form, which
// multiplies by len and divides again (bvh.rs:67-76, 191-194) -- the operations of
// light_pdf_rays_kernel and light_sample_kernel's fused pdf, through the same
// lights_pdf_* functions.  tests: the (ray, light) pairs tested.
template <typename R, int kPath, bool kRobust>
__device__ __forceinline__ R light_list_pdf(const DevScene<R>& sc, V3<R> o, V3<R> d, int32_t* stk, uint32_t& tests) {
    R acc;
    LightWork lw;
    if constexpr (kPath == kLightMixed) {
        acc = lights_pdf_mixed(sc, sc.lights, o, d);
        lw.tests = sc.n_list;
    } else if constexpr (kPath == kLightGrid) {
        acc = lights_pdf_grid<kRobust>(sc, o, d, lw);
    } else if constexpr (kPath == kLightBvh) {
        acc = lights_pdf_bvh<kRobust>(sc, o, d, stk, lw);
    } else {
        acc = lights_pdf_sum<kRobust>(sc.lights, sc.n_lights, o, d);
        lw.tests = sc.n_lights;
    }
    tests = lw.tests;
    R lpdf = P<R>::div_(acc, (R)sc.n_list);
    if (sc.light_flags & 1u) lpdf = P<R>::div_(lpdf * (R)sc.n_list, (R)sc.n_list);
    return lpdf;
}

template <typename R>
__global__ void __launch_bounds__(kQueryBlock) camera_rays_kernel(const CParams<R> p) {
    using PR = P<R>;
    extern __shared__ __attribute__((aligned(32))) unsigned char smem[];
    unsigned long long cnt[kQueryCounters] = {};
    const uint64_t n_blocks = (p.n + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t k = blk * kQueryBlock + threadIdx.x;
        if (k >= p.n) continue;
        // the pixel index j * W + i, the render's stream key; an index beyond the image is
        // the caller's error (the host form refuses it): clamped, nothing out of bounds
        uint64_t pix = p.pixels ? (uint64_t)p.pixels[k] : p.first_pixel + k;
        pix = pix < p.n_pixels ? pix : p.n_pixels - 1;
        const uint32_t j = (uint32_t)(pix / p.W), i = (uint32_t)(pix - (uint64_t)j * p.W);
        // Camera::get_ray, camera.rs:274-293 (render_kernel's start_sample)
        Rng g;
        g.seed(p.seed, pix, (uint64_t)p.sample);
        const R ox = PR::u_incl(g.next(), (R)-0.5, p.u_scale);
        const R oy = PR::u_incl(g.next(), (R)-0.5, p.u_scale);
        const V3<R> ps = (mk(p.p00[0], p.p00[1], p.p00[2]) + mk(p.du[0], p.du[1], p.du[2]) * ((R)i + ox)) +
                         mk(p.dv[0], p.dv[1], p.dv[2]) * ((R)j + oy);
        const V3<R> center = mk(p.center[0], p.center[1], p.center[2]);
        V3<R> origin = center;
        if (p.defocus) {
            const V3<R> qd = unit_disk<R>(g);
            origin = (center + mk(p.disk_u[0], p.disk_u[1], p.disk_u[2]) * qd.x) +
                     mk(p.disk_v[0], p.disk_v[1], p.disk_v[2]) * qd.z;
        }
        const V3<R> d = ps - origin;
        const R ray[6] = {origin.x, origin.y, origin.z, d.x, d.y, d.z};
        store_rec<record_align(6 * sizeof(R))>(p.rays + 6 * k, ray);
        const uint64_t st[4] = {g.s0, g.s1, g.s2, g.s3};
        store_rec<16>(p.rng + 4 * k, st);
        cnt[kQcRays] += 1;
    }
    query_counters_flush(smem, p.counters, cnt);
}

template <typename R, int kPath, bool kRobust>
__global__ void __launch_bounds__(kQueryBlock) shade_rays_kernel(const SParams<R> p) {
    using PR = P<R>;
    extern __shared__ __attribute__((aligned(32))) unsigned char smem[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int32_t* const stk = reinterpret_cast<int32_t*>(smem) + wave * p.stack * 64 + lane;
    (void)stk;
    unsigned long long cnt[kQueryCounters] = {};
    const uint64_t n_blocks = (p.n + kQueryBlock - 1) / kQueryBlock;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t k = blk * kQueryBlock + threadIdx.x;
        const bool live = k < p.n;
        int32_t id[4] = {-1, 0, 0, 0};
        R ray[6] = {}, h[9] = {};
        if (live) {
            load_rec<16>(p.ids + 4 * k, id);
            load_rec<record_align(6 * sizeof(R))>(p.rays + 6 * k, ray);
            load_rec<record_align(9 * sizeof(R))>(p.hits + 9 * k, h);
        }
        // a miss: object id < 0 (a material id that is not the scene's is answered the
        // same way: no table is read out of bounds)
        const bool hit = live && id[0] >= 0 && (uint32_t)id[1] < p.sc.n_mat;
        const uint32_t m = hit ? (uint32_t)id[1] : 0u;
        const bool front = id[2] != 0;
        const V3<R> d = mk(ray[3], ray[4], ray[5]);
        const V3<R> pnt = mk(h[1], h[2], h[3]), nrm = mk(h[4], h[5], h[6]);
        const V3<R> zero = mk<R>(0, 0, 0);
        Rng g = {0, 0, 0, 0};
        uint32_t mtype = kMatInvisible;
        R4<R> mp = R4<R>{0, 0, 0, 0};
        if (hit) {
            uint64_t st[4];
            load_rec<16>(p.rng + 4 * k, st);
            g.s0 = st[0], g.s1 = st[1], g.s2 = st[2], g.s3 = st[3];
            // four zero words are no xoshiro256++ state (no seeding gives them): every draw
            // would be 0 and the rejection loops would never end -- the stream of (0, 0, 0) instead
            if ((st[0] | st[1] | st[2] | st[3]) == 0) g.seed(0, 0, 0);
            mtype = p.sc.mat_type[m];
            mp = p.sc.mat_p[m];
        }
        // Material::emitted: DiffuseLight's texture at the record's (u, v, p)
        // (material.rs:508-514), black for every other material (material.rs:42-44);
        // Lambertian's attenuation is its texture's colour there (material.rs:357-376)
        V3<R> colour = mk(mp.x, mp.y, mp.z);
        if (p.sc.mat_tex && (mtype == kMatDiffuseLight || mtype == kMatLambertian))
            colour = tex_colour(p.sc, p.sc.mat_tex[m], h[7], h[8], pnt);
        const V3<R> emitted = mtype == kMatDiffuseLight ? colour : zero;
        int32_t event = hit ? kEventAbsorbed : kEventMiss;   // DiffuseLight, Invisible: scatter() is None
        V3<R> dir = zero, weight = zero;
        R pdf3[3] = {(R)0, (R)0, (R)0};
        if (mtype == kMatMetal || mtype == kMatDielectric) {
            const bool metal = mtype == kMatMetal;
            bool keep = true;
            if constexpr (sizeof(R) == 8) {
                // Metal::scatter and Dialectric::scatter (material.rs:407-421, 458-487) in
                // one pass, with the reference's UnitSphere loop: render_kernel's f64 bounce
                dir = specular_dir64<true>(metal, to64(d), to64(nrm), front, p.sc.mat64[m], g, keep);
            } else if (metal) {
                const V3<R> refl = reflect(PR::normalize(d), nrm);
                dir = refl + unit_sphere<R>(g) * mp.w;
                keep = dot(dir, nrm) > (R)0;
            } else {
                const R ratio = front ? PR::div_((R)1, mp.w) : mp.w;
                const V3<R> unit = PR::normalize(d);
                const R cos_t = PR::min_(dot(unit, -nrm), (R)1);
                const R sin_t = PR::sqrt_((R)1 - cos_t * cos_t);
                const bool cannot = ratio * sin_t > (R)1;
                if (cannot || reflectance(cos_t, ratio) > PR::u_open01(g.next())) dir = reflect(unit, nrm);
                else dir = refract(unit, nrm, ratio);
            }
            if (keep) {   // Reflect, camera.rs:488-500: mult * attenuation, no emission
                event = kEventReflect;
                weight = metal ? mk(mp.x, mp.y, mp.z) : mk<R>(1, 1, 1);
            } else {
                dir = zero;
            }
        }
        const bool lamb = mtype == kMatLambertian;
        if (lamb) {
            // MixturePdf(HittablePdf(lights), CosinePdf)::generate: pdf.rs:91-96,
            // hittable_list.rs:414-419 -- one Standard for the lobe, then gen_range(0..len)
            // and the entry's random(), or the cosine hemisphere (render_kernel's draws)
            const bool to_light = PR::u_std(g.next()) < (R)0.5;
            bool sampled = false;
            R4<R> L = R4<R>{0, 0, 0, 0};
            if (to_light) {   // (the host refuses an empty list)
                const uint32_t idx = g.index(p.sc.n_list);
                const uint32_t ref = p.sc.lref ? p.sc.lref[idx] : idx;
                if (ref & kLrefQuad) {
                    dir = quad_random(p.sc.lquads + kQuadR * (ref & 0x3fffffffu), pnt, g);
                    sampled = true;
                } else if (ref & kLrefDefault) {
                    dir = mk<R>(1, 0, 0);                  // Hittable::random default
                    sampled = true;
                } else {
                    L = p.sc.lights[ref];
                }
            }
            // a sphere light or the cosine lobe, in one pass
            if (!sampled) dir = mixture_direction(to_light, nrm, mk(L.x, L.y, L.z), L.w, pnt, g);
        }
        // ---- the Lambertian lanes' light pdf, together
        if (lamb) {
            uint32_t tests;
            const R lpdf = light_list_pdf<R, kPath, kRobust>(p.sc, pnt, dir, stk, tests);
            cnt[kQcLightTests] += tests;
            // pdf.rs:33-101, camera.rs:504-521, in render_kernel's order
            const V3<R> ndir = PR::normalize(dir);
            const V3<R> wn = PR::normalize(nrm);
            const R cos_w = PR::over_pi(dot(ndir, wn));
            const R pdf = lpdf * (R)0.5 + PR::max_(cos_w, (R)0) * (R)0.5;
            const R spdf = PR::max_(PR::over_pi(dot(nrm, ndir)), (R)0);
            weight = PR::divs(colour * spdf, pdf);
            pdf3[0] = pdf, pdf3[1] = lpdf, pdf3[2] = spdf;
            event = kEventScatter;
        }
        if (!live) continue;
        cnt[kQcRays] += 1;
        const bool goes_on = event >= kEventReflect;
        cnt[kQcHits] += goes_on ? 1 : 0;
        const V3<R> np = goes_on ? pnt : zero;
        const R nx[6] = {np.x, np.y, np.z, dir.x, dir.y, dir.z};
        const R w3[3] = {weight.x, weight.y, weight.z}, e3[3] = {emitted.x, emitted.y, emitted.z};
        store_rec<record_align(6 * sizeof(R))>(p.next + 6 * k, nx);
        store_rec<record_align(3 * sizeof(R))>(p.weight + 3 * k, w3);
        store_rec<record_align(3 * sizeof(R))>(p.emitted + 3 * k, e3);
        p.event[k] = event;
        if (p.pdfs) store_rec<record_align(3 * sizeof(R))>(p.pdfs + 3 * k, pdf3);
        if (hit) {   // (a miss leaves its state untouched)
            const uint64_t st[4] = {g.s0, g.s1, g.s2, g.s3};
            store_rec<16>(p.rng + 4 * k, st);
        }
    }
    query_counters_flush(smem, p.counters, cnt);
}

}  // namespace dev

}  // namespace rtw
