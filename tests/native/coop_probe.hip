// coop_probe.hip -- the wave-cooperative light-grid walks of light_pdf.hpp
// (lights_pdf_grid_coop, lights_pdf_grid_coop64, lights_pdf_grid_coop_list) run
// wave by wave on a small light set, next to the lane walk, the linear sums and
// a sweep of the piece walk over every cut (tests/test_gpu_coop_probe.py).
//
//   coop_probe IN OUT
//
// The lights are staged by host/stage_scene.cpp (f32 and f64) at the given
// grid density, so the grid, the cell records, lg_sph32 and the padding are the
// renderer's.  Link host/stage_scene.cpp and host/bvh.cpp.
//
// IN:  u64 n_lights, n_rays, n_waves; f64 density; n_lights x 4 f64 {c, r};
//      n_rays x 6 f64 {o, d}; n_rays x i32 sampled light (-1: none);
//      n_waves x WaveIn {u32 P, cap_words, ray[64], pend[64]}.
// OUT: Header; u32 big ids [n_big]; u32 cell lengths [n_cells];
//      u8 counts [n_rays][3 predicates][6 cuts][n_lights] (predicate 0: the f64
//      scene's rounded grid with light_may_hit, 1 / 2: the f32 scene's grid with
//      light_hit_f32<false / true>; cuts 1, 2, 3, 7, cells, and in place of a
//      sixth the predicate alone over the light list in list order, no grid);
//      n_waves x 64 Lane64; 2 x n_waves x 64 Lane32 (kRobust = false, true).
// Every kernel runs 64 threads per block: the walks are wave-wide and converged.
// Exits non-zero on any HIP error or malformed input.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "host/stage_scene.hpp"
#include "light_pdf.hpp"   // (bvh_traverse.hpp's rtw_probes.hpp leaves every RTW_PROBE_* hook empty here)

using namespace rtw;
using namespace rtw::dev;

#define CHECK(x)                                                                              \
    do {                                                                                      \
        const hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(2);                                                                          \
        }                                                                                     \
    } while (0)

constexpr uint32_t kMaxLights = 512, kMaxRays = 4096, kMaxWaves = 64;
constexpr uint32_t kMaxCapWords = 1536;   // the slots' LDS of a wave (words)
constexpr uint32_t kCuts = 6, kPreds = 3;    // the last "cut": the plain predicate over the whole light list, no walk

struct Header {
    double lo[3], cell[3];                 // the grid as build_light_grid made it
    uint32_t n[3], n_big, n_cells, n_items, pad[2];
};
struct WaveIn {
    uint32_t P, cap_words, ray[64], pend[64];
};
struct Lane64 {
    double coop, walk, lin;
    uint32_t nbig, cells;                  // big lights light_may_hit accepts; the own ray's cells (0: misses the grid)
    uint32_t m13, m14, m16, pad;           // lane 0: the wave's marks
    uint32_t lw_tests, lw_cells;           // the lane's LightWork of the cooperative walk
};
struct Lane32 {
    float coop, walk, lin, pk, pks;        // the product's five paths
    float plain, forced, minterm, sterm;   // the probe's own loop: the sum, with `sampled` forced in, the smallest term, sampled's
    uint32_t m, s_hit, cells;              // hit lights; sampled was among them; the own ray's cells
    uint32_t m13, m14, lw_tests, lw_cells;
};

// the f64 scene's grid as the f32 walk reads it (render_kernel.hpp fills Grid64 so)
static Grid64 grid64_of(const DevScene<double>& sc) {
    Grid64 gr;
    gr.lg_start = sc.lg_start;
    gr.lg_rec = sc.lg_rec;
    gr.lg_sph32 = sc.lg_sph32;
    gr.lg_id = sc.lg_id;
    gr.lights = sc.lights;
    for (int a = 0; a < 3; ++a) {
        gr.lo[a] = (float)sc.lg_lo[a];
        gr.hi[a] = (float)sc.lg_hi[a];
        gr.cell[a] = (float)sc.lg_cell[a];
        gr.inv[a] = (float)sc.lg_inv[a];
        gr.n[a] = sc.lg_n[a];
    }
    gr.big = sc.lg_big;
    return gr;
}
// ... and as lights_pdf_grid_coop64 hands it to the walk
__device__ __forceinline__ DevScene<float> walk_scene(const Grid64& sc) {
    DevScene<float> g;
    g.lg_start = sc.lg_start;
    g.lg_sph = sc.lg_sph32;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g.lg_lo[a] = sc.lo[a];
        g.lg_hi[a] = sc.hi[a];
        g.lg_cell[a] = sc.cell[a];
        g.lg_inv[a] = sc.inv[a];
        g.lg_n[a] = sc.n[a];
    }
    return g;
}

__device__ __forceinline__ uint32_t cut_of(uint32_t c, uint32_t cells) {
    return c == 0 ? 1u : (c == 1 ? 2u : (c == 2 ? 3u : (c == 3 ? 7u : cells)));
}

// Kernel 1: for every cut k, light_grid_walk_piece_rec over all k pieces with
// t_at as the cooperative walks compute it, and the kernels' own predicates.
// One ray per thread; cnt[ray][pred][cut][light] starts at 0.
__global__ void __launch_bounds__(64) probe_counts(Grid64 gr, DevScene<float> sc, const double* __restrict__ rays,
                                                   uint32_t n_rays, uint32_t n_lights, uint8_t* __restrict__ cnt) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n_rays) return;
    const double* p = rays + 6 * k;
    uint8_t* c0 = cnt + (size_t)k * kPreds * kCuts * n_lights;
    auto at = [&](uint32_t pred, uint32_t cut, uint32_t id) -> uint8_t& {
        return c0[((size_t)pred * kCuts + cut) * n_lights + id];
    };
    {   // a. the f64 scene's rounded grid, light_may_hit (lights_pdf_grid_coop_list's `test` of the f64 instance)
        const DevScene<float> g = walk_scene(gr);
        const LightPre pre(mk(p[0], p[1], p[2]), mk(p[3], p[4], p[5]));
        const V3<float> ro = mk(pre.ox, pre.oy, pre.oz), rd = mk(pre.dx, pre.dy, pre.dz);
        const float ria = __builtin_amdgcn_rcpf(__builtin_fmaf(rd.x, rd.x, __builtin_fmaf(rd.y, rd.y, rd.z * rd.z)));
        const float ron = light_on(ro.x, ro.y, ro.z), rdn = fabsf(rd.x) + fabsf(rd.y) + fabsf(rd.z);
        for (uint32_t q = 0; q < gr.big; ++q) {
            const R4<float> L = g.lg_sph[q];
            if (light_may_hit(L.x, L.y, L.z, L.w, ro.x, ro.y, ro.z, rd.x, rd.y, rd.z, ria, ron, rdn))
                for (uint32_t c = 0; c + 1 < kCuts; ++c) ++at(0, c, gr.lg_id[q]);
        }
        for (uint32_t q = 0; q < n_lights; ++q)
            if (pre.may_hit(gr.lights[q])) ++at(0, kCuts - 1, q);
        float rtn = 0.f, rtf = 0.f;
        uint32_t cells = 0;
        if (light_grid_span(g, ro, rd, grid_inv(rd.x), grid_inv(rd.y), grid_inv(rd.z), rtn, rtf, cells)) {
            for (uint32_t c = 0; c + 1 < kCuts; ++c) {
                const uint32_t rk = cut_of(c, cells);
                const float step = (rtf - rtn) / (float)rk;
                auto t_at = [&](uint32_t q) { return q == 0 ? rtn : __builtin_fmaf((float)q, step, rtn); };
                for (uint32_t j = 0; j < rk; ++j)
                    light_grid_walk_piece_rec(g, gr.lg_rec, g.lg_sph, ro, rd, grid_inv(rd.x), grid_inv(rd.y),
                                              grid_inv(rd.z), t_at(j), t_at(j + 1), j == 0, j + 1 == rk,
                                              [&](const R4<float>& L, auto&& idx, float te, float tx) {
                        if (light_may_hit(L.x, L.y, L.z, L.w, ro.x, ro.y, ro.z, rd.x, rd.y, rd.z, ria, ron, rdn)) {
                            const float tc = -__builtin_fmaf(rd.z, ro.z - L.z, __builtin_fmaf(rd.y, ro.y - L.y,
                                                                                               rd.x * (ro.x - L.x))) * ria;
                            if (!(tc >= te && tc < tx)) return;
                            ++at(0, c, gr.lg_id[idx()]);
                        }
                    });
            }
        }
    }
    // b. the f32 scene's grid, light_hit_f32 (lights_pdf_grid_coop's `test`)
    auto sweep32 = [&](auto robust, uint32_t pred) {
        constexpr bool kRobust = decltype(robust)::value;
        const V3<float> ro = mk((float)p[0], (float)p[1], (float)p[2]), rd = mk((float)p[3], (float)p[4], (float)p[5]);
        const float ra = len2_f32(rd);
        const float ria = __builtin_amdgcn_rcpf(ra);
        for (uint32_t q = 0; q < sc.lg_big; ++q)
            if (light_hit_f32<kRobust>(sc.lg_sph[q], ro, rd, ra, ria))
                for (uint32_t c = 0; c + 1 < kCuts; ++c) ++at(pred, c, sc.lg_id[q]);
        for (uint32_t q = 0; q < n_lights; ++q)
            if (light_hit_f32<kRobust>(sc.lights[q], ro, rd, ra, ria)) ++at(pred, kCuts - 1, q);
        float rtn = 0.f, rtf = 0.f;
        uint32_t cells = 0;
        if (!light_grid_span(sc, ro, rd, grid_inv(rd.x), grid_inv(rd.y), grid_inv(rd.z), rtn, rtf, cells)) return;
        for (uint32_t c = 0; c + 1 < kCuts; ++c) {
            const uint32_t rk = cut_of(c, cells);
            const float step = (rtf - rtn) / (float)rk;
            auto t_at = [&](uint32_t q) { return q == 0 ? rtn : __builtin_fmaf((float)q, step, rtn); };
            for (uint32_t j = 0; j < rk; ++j)
                light_grid_walk_piece_rec(sc, sc.lg_rec, sc.lg_sph, ro, rd, grid_inv(rd.x), grid_inv(rd.y),
                                          grid_inv(rd.z), t_at(j), t_at(j + 1), j == 0, j + 1 == rk,
                                          [&](const R4<float>& L, auto&& idx, float te, float tx) {
                    const float fx = ro.x - L.x, fy = ro.y - L.y, fz = ro.z - L.z;
                    const float tc = -__builtin_fmaf(rd.z, fz, __builtin_fmaf(rd.y, fy, rd.x * fx)) * ria;
                    if (light_hit_f32<kRobust>(L, ro, rd, ra, ria) & (tc >= te) & (tc < tx)) ++at(pred, c, sc.lg_id[idx()]);
                });
        }
    };
    sweep32(std::false_type{}, 1);
    sweep32(std::true_type{}, 2);
}

// Kernel 2: one f64 wave per block.  The ray in LDS in the kernel's [word][lane]
// layout, the slots after it.
__global__ void __launch_bounds__(64) probe_f64(Grid64 gr, DevScene<double> sc, const double* __restrict__ rays,
                                                const WaveIn* __restrict__ waves, Lane64* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[12 * 64 + kMaxCapWords];
    const uint32_t lane = threadIdx.x;
    const WaveIn& w = waves[blockIdx.x];
    const double* p = rays + 6 * (size_t)w.ray[lane];
    const bool pend = w.pend[lane] != 0;
    for (uint32_t q = 0; q < 6; ++q) {
        const uint64_t v = (uint64_t)__double_as_longlong(p[q]);
        lds[(2 * q) * 64 + lane] = (uint32_t)v;
        lds[(2 * q + 1) * 64 + lane] = (uint32_t)(v >> 32);
    }
    __syncthreads();
    const V3<double> o = mk(p[0], p[1], p[2]), d = mk(p[3], p[4], p[5]);
    Lane64 row{};
    LightWork lw;
    // lane 0 counts the walk's marks: 13 a walk, 14 a round, 16 an owner merge
    auto mark = [&](int id) {
        if (lane == 0) {
            row.m13 += id == 13;
            row.m14 += id == 14;
            row.m16 += id == 16;
        }
    };
    row.coop = lights_pdf_grid_coop64(gr, pend, lds, w.P, lds + 12 * 64, w.cap_words, lane, lw, mark);
    row.lw_tests = lw.tests;
    row.lw_cells = lw.cells;
    LightWork lw2;
    row.walk = lights_pdf_grid<false>(sc, o, d, lw2);
    row.lin = lights_pdf_sum<false>(sc.lights, sc.n_lights, o, d);
    {
        const LightPre pre(o, d);
        const DevScene<float> g = walk_scene(gr);
        const V3<float> of = mk(pre.ox, pre.oy, pre.oz), df = mk(pre.dx, pre.dy, pre.dz);
        for (uint32_t q = 0; q < gr.big; ++q) {
            const R4<float> L = gr.lg_sph32[q];
            row.nbig += light_may_hit(L.x, L.y, L.z, L.w, pre.ox, pre.oy, pre.oz, pre.dx, pre.dy, pre.dz, pre.ia, pre.on,
                                      pre.dn) ? 1u : 0u;
        }
        float tn, tf;
        uint32_t cells = 0;
        row.cells = light_grid_span(g, of, df, grid_inv(df.x), grid_inv(df.y), grid_inv(df.z), tn, tf, cells) ? cells : 0u;
    }
    out[(size_t)blockIdx.x * 64 + lane] = row;
}

// Kernel 3: one f32 wave per block; `cap` floats of slots.
template <bool kRobust>
__global__ void __launch_bounds__(64) probe_f32(DevScene<float> sc, const R4<float>* __restrict__ lp,
                                                const double* __restrict__ rays, const int32_t* __restrict__ sampled,
                                                const WaveIn* __restrict__ waves, Lane32* __restrict__ out) {
    __shared__ float slots[kMaxCapWords];
    const uint32_t lane = threadIdx.x;
    const WaveIn& w = waves[blockIdx.x];
    const double* p = rays + 6 * (size_t)w.ray[lane];
    const int32_t s = sampled[w.ray[lane]];
    const bool pend = w.pend[lane] != 0;
    const V3<float> o = mk((float)p[0], (float)p[1], (float)p[2]), d = mk((float)p[3], (float)p[4], (float)p[5]);
    // the slots of the f32 walk: one float per piece, a multiple of 64, at least one round
    const uint32_t cap = max(64u, w.cap_words / 8u / 64u * 64u);
    Lane32 row{};
    LightWork lw;
    auto mark = [&](int id) {
        if (lane == 0) {
            row.m13 += id == 13;
            row.m14 += id == 14;
        }
    };
    row.coop = lights_pdf_grid_coop<kRobust>(sc, pend, o, d, w.P, slots, cap, lane, lw, mark);
    row.lw_tests = lw.tests;
    row.lw_cells = lw.cells;
    LightWork lw2;
    row.walk = lights_pdf_grid<kRobust>(sc, o, d, lw2);
    row.lin = lights_pdf_sum<kRobust>(sc.lights, sc.n_lights, o, d);
    row.pk = lights_pdf_sum_pk<kRobust>(sc.lights, lp, sc.n_lights, o, d, -1);
    row.pks = lights_pdf_sum_pk<kRobust>(sc.lights, lp, sc.n_lights, o, d, s);
    {   // the plain sweep
        const float a = len2_f32(d);
        const float ia = __builtin_amdgcn_rcpf(a);
        float plain = 0.f, forced = 0.f, mn = INFINITY;
        bool mn_nan = false;
        for (uint32_t k = 0; k < sc.n_lights; ++k) {
            const R4<float> L = sc.lights[k];
            const bool hit = light_hit_f32<kRobust>(L, o, d, a, ia);
            const float term = light_pdf_f32(L, o);
            if (hit) {
                ++row.m;
                plain += term;
                mn_nan |= term != term;
                mn = term < mn ? term : mn;
            }
            if (hit || (int32_t)k == s) forced += term;
            if ((int32_t)k == s) {
                row.s_hit = hit ? 1u : 0u;
                row.sterm = term;
            }
        }
        row.plain = plain;
        row.forced = forced;
        row.minterm = mn_nan ? NAN : mn;
        float tn, tf;
        uint32_t cells = 0;
        row.cells = light_grid_span(sc, o, d, grid_inv(d.x), grid_inv(d.y), grid_inv(d.z), tn, tf, cells) ? cells : 0u;
    }
    out[(size_t)blockIdx.x * 64 + lane] = row;
}

template <typename T>
static std::vector<T> read_n(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "coop_probe: short input\n");
        exit(3);
    }
    return v;
}
template <typename T>
static T* upload(const T* v, size_t n) {
    T* p = nullptr;
    CHECK(hipMalloc(&p, sizeof(T) * (n + 1)));
    if (n) CHECK(hipMemcpy(p, v, sizeof(T) * n, hipMemcpyHostToDevice));
    return p;
}
static void bad(const char* what) {
    fprintf(stderr, "coop_probe: %s\n", what);
    exit(3);
}

// the lights staged as the renderer stages them, the blob on the device
template <typename R>
struct Staged {
    DevScene<R> ds;
    std::vector<unsigned char> blob;   // as uploaded (pointers relative to `dev`)
    unsigned char* dev = nullptr;
    template <typename T>
    const T* host(const T* dev_ptr) const {
        return reinterpret_cast<const T*>(blob.data() + ((uintptr_t)dev_ptr - (uintptr_t)dev));
    }
};
template <typename R>
static Staged<R> stage(const rtw_scene& s, double density) {
    Staged<R> st;
    DevScene<R> tmp{};
    const size_t bytes = stage_scene<R>(&s, &tmp, 0, 4, 4, density).size();
    CHECK(hipMalloc(&st.dev, bytes));
    st.ds = DevScene<R>{};
    st.blob = stage_scene<R>(&s, &st.ds, (uintptr_t)st.dev, 4, 4, density);
    if (st.blob.size() != bytes) bad("staging is not deterministic");
    CHECK(hipMemcpy(st.dev, st.blob.data(), bytes, hipMemcpyHostToDevice));
    return st;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: coop_probe IN OUT\n");
        return 3;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 3;
    }
    const std::vector<uint64_t> head = read_n<uint64_t>(f, 3);
    const uint64_t n_lights = head[0], n_rays = head[1], n_waves = head[2];
    const double density = read_n<double>(f, 1)[0];
    if (n_lights < 1 || n_lights > kMaxLights || n_rays < 1 || n_rays > kMaxRays || n_waves > kMaxWaves)
        bad("at most 512 lights, 4096 rays and 64 waves (and at least one light and one ray)");
    if (!(density > 0 && density <= 64)) bad("grid density out of range");
    const std::vector<double> lights = read_n<double>(f, 4 * n_lights);
    const std::vector<double> rays = read_n<double>(f, 6 * n_rays);
    const std::vector<int32_t> sampled = read_n<int32_t>(f, n_rays);
    const std::vector<WaveIn> waves = read_n<WaveIn>(f, n_waves);
    fclose(f);
    for (const int32_t s : sampled)
        if (s < -1 || s >= (int32_t)n_lights) bad("sampled light out of range");
    for (const WaveIn& w : waves) {
        if (w.P == 0 || w.cap_words > kMaxCapWords || w.cap_words % 64) bad("wave: P == 0 or cap_words not a multiple of 64 <= 1536");
        for (int l = 0; l < 64; ++l)
            if (w.ray[l] >= n_rays) bad("wave: ray index out of range");
    }

    // one Lambertian sphere far below: the world is not the probe's subject
    const double sphere[4] = {0.0, -1e6, 0.0, 1.0}, mat[5] = {0.5, 0.5, 0.5, 0.0, 0.0};
    const uint32_t zero = 0;
    rtw_scene s{};
    s.n_spheres = 1;
    s.spheres = sphere;
    s.sphere_mat = &zero;
    s.n_materials = 1;
    s.mat_type = &zero;
    s.mat_params = mat;
    s.n_lights = (uint32_t)n_lights;
    s.lights = lights.data();
    const Staged<float> s32 = stage<float>(s, density);
    const Staged<double> s64 = stage<double>(s, density);
    if (!s32.ds.lg_on || !s64.ds.lg_on) bad("no light grid: no finite light");
    const Grid64 gr = grid64_of(s64.ds);

    Header h{};
    for (int a = 0; a < 3; ++a) {
        h.lo[a] = s64.ds.lg_lo[a];
        h.cell[a] = s64.ds.lg_cell[a];
        h.n[a] = s64.ds.lg_n[a];
        if (s32.ds.lg_n[a] != s64.ds.lg_n[a]) bad("the f32 and f64 grids differ");
    }
    h.n_big = s64.ds.lg_big;
    h.n_cells = h.n[0] * h.n[1] * h.n[2];
    const uint32_t* start = s64.host(s64.ds.lg_start);
    const uint32_t* lg_id = s64.host(s64.ds.lg_id);
    h.n_items = start[h.n_cells];
    if (memcmp(start, s32.host(s32.ds.lg_start), sizeof(uint32_t) * (h.n_cells + 1)) != 0 ||
        memcmp(lg_id, s32.host(s32.ds.lg_id), sizeof(uint32_t) * h.n_items) != 0 || s32.ds.lg_big != h.n_big)
        bad("the f32 and f64 grids differ");
    std::vector<uint32_t> cell_len(h.n_cells);
    for (uint32_t c = 0; c < h.n_cells; ++c) cell_len[c] = start[c + 1] - start[c];

    // the light pairs of the packed test, as the render kernel stages them in LDS
    std::vector<R4<float>> lp(2 * ((n_lights + 1) / 2));
    {
        const R4<float>* li = s32.host(s32.ds.lights);
        const uint32_t n = (uint32_t)n_lights;
        for (uint32_t q = 0; 2 * q < n; ++q) {
            const R4<float> A = li[2 * q];
            const bool odd = 2 * q + 1 < n;
            const R4<float> B = odd ? li[2 * q + 1] : R4<float>{0, 0, 0, 0};
            lp[2 * q] = R4<float>{A.x, B.x, A.y, B.y};
            lp[2 * q + 1] = R4<float>{A.z, B.z, A.w * A.w, odd ? B.w * B.w : -INFINITY};
        }
    }

    double* d_rays = upload(rays.data(), rays.size());
    int32_t* d_sampled = upload(sampled.data(), sampled.size());
    WaveIn* d_waves = upload(waves.data(), waves.size());
    R4<float>* d_lp = upload(lp.data(), lp.size());
    const size_t n_cnt = (size_t)n_rays * kPreds * kCuts * n_lights;
    std::vector<uint8_t> cnt(n_cnt);
    {
        uint8_t* d_cnt = nullptr;
        CHECK(hipMalloc(&d_cnt, n_cnt));
        CHECK(hipMemset(d_cnt, 0, n_cnt));
        probe_counts<<<dim3((unsigned)((n_rays + 63) / 64)), dim3(64)>>>(gr, s32.ds, d_rays, (uint32_t)n_rays,
                                                                          (uint32_t)n_lights, d_cnt);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(cnt.data(), d_cnt, n_cnt, hipMemcpyDeviceToHost));
        CHECK(hipFree(d_cnt));
    }
    std::vector<Lane64> l64(n_waves * 64);
    std::vector<Lane32> l32[2] = {std::vector<Lane32>(n_waves * 64), std::vector<Lane32>(n_waves * 64)};
    if (n_waves) {
        Lane64* d_64 = nullptr;
        Lane32* d_32 = nullptr;
        CHECK(hipMalloc(&d_64, sizeof(Lane64) * l64.size()));
        CHECK(hipMalloc(&d_32, sizeof(Lane32) * l64.size()));
        CHECK(hipMemset(d_64, 0, sizeof(Lane64) * l64.size()));
        probe_f64<<<dim3((unsigned)n_waves), dim3(64)>>>(gr, s64.ds, d_rays, d_waves, d_64);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(l64.data(), d_64, sizeof(Lane64) * l64.size(), hipMemcpyDeviceToHost));
        for (int r = 0; r < 2; ++r) {
            CHECK(hipMemset(d_32, 0, sizeof(Lane32) * l64.size()));
            if (r == 0) probe_f32<false><<<dim3((unsigned)n_waves), dim3(64)>>>(s32.ds, d_lp, d_rays, d_sampled, d_waves, d_32);
            else probe_f32<true><<<dim3((unsigned)n_waves), dim3(64)>>>(s32.ds, d_lp, d_rays, d_sampled, d_waves, d_32);
            CHECK(hipGetLastError());
            CHECK(hipDeviceSynchronize());
            CHECK(hipMemcpy(l32[r].data(), d_32, sizeof(Lane32) * l64.size(), hipMemcpyDeviceToHost));
        }
        CHECK(hipFree(d_64));
        CHECK(hipFree(d_32));
    }
    CHECK(hipFree(d_rays));
    CHECK(hipFree(d_sampled));
    CHECK(hipFree(d_waves));
    CHECK(hipFree(d_lp));
    CHECK(hipFree(s32.dev));
    CHECK(hipFree(s64.dev));

    FILE* g = fopen(argv[2], "wb");
    if (!g) {
        perror(argv[2]);
        return 3;
    }
    auto put = [&](const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, g) == bytes; };
    if (!put(&h, sizeof h) || !put(lg_id, sizeof(uint32_t) * h.n_big) || !put(cell_len.data(), sizeof(uint32_t) * h.n_cells) ||
        !put(cnt.data(), n_cnt) || !put(l64.data(), sizeof(Lane64) * l64.size()) ||
        !put(l32[0].data(), sizeof(Lane32) * l64.size()) || !put(l32[1].data(), sizeof(Lane32) * l64.size()) ||
        fclose(g) != 0) {
        fprintf(stderr, "coop_probe: cannot write %s\n", argv[2]);
        return 3;
    }
    printf("coop_probe: %llu lights, %llu rays, %llu waves, grid %u x %u x %u, %u big\n", (unsigned long long)n_lights,
           (unsigned long long)n_rays, (unsigned long long)n_waves, h.n[0], h.n[1], h.n[2], h.n_big);
    return 0;
}
