// cull_probe.hip -- the f64 kernels' f32 culling filters and their f64
// counterparts, one record per thread (tests/test_gpu_cull_probe.py).
//
//   cull_probe IN OUT
//
// IN:  u64 n, u64 m; n x 10 f64 {o, d, c, r}; n x 4 f32 {c, r^2} (the sphere as
//      stage_scene.cpp fills bsph32); m x 13 f64 {o, d, box lo, box hi, tb} (the
//      tree's padded f64 box); m x 6 f32 (that box rounded outward, the f32 tree's).
// OUT: n x {f64 t (world query, t_min = eps), t (light query, t_min = 0), pdf;
//      u32 hit (world), hit (light), sphere_may_hit, light_may_hit};
//      m x {u32 ntest of bvh_traverse_ww, ntest of bvh4_traverse} on a one-node
//      tree whose two children are both the record's box, with leaves of 1 and 2
//      spheres: ntest = 1 * (child 0 entered) + 2 * (child 1 entered).
// Exits non-zero on any HIP error.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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

struct SphereRow {
    double t_world, t_light, pdf;
    uint32_t hit_world, hit_light, may_sphere, may_light;
};
struct BoxRow {
    uint32_t ntest_ww, ntest_4;
};

__global__ void probe_spheres(const double* __restrict__ rec, const R4<float>* __restrict__ s32, uint64_t n,
                              SphereRow* __restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double* p = rec + 10 * k;
    const V3<double> o = mk(p[0], p[1], p[2]), d = mk(p[3], p[4], p[5]), c = mk(p[6], p[7], p[8]);
    const double r = p[9];
    SphereRow row;
    row.t_world = row.t_light = 0.0;
    // the world query (SphereTester<double>::test_hit) and the light query
    row.hit_world = sphere_t(c, r * r, o, d, P<double>::kEps, row.t_world) ? 1u : 0u;
    row.hit_light = sphere_t(c, r * r, o, d, 0.0, row.t_light) ? 1u : 0u;
    row.pdf = sphere_pdf_value(c, r, o, d);
    {   // the ray quantities exactly as test_leaf computes them
        const float ox = (float)o.x, oy = (float)o.y, oz = (float)o.z;
        const float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z;
        const float ia = __builtin_amdgcn_rcpf(__builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz)));
        const float on = fabsf(ox) + fabsf(oy) + fabsf(oz), dn = fabsf(dx) + fabsf(dy) + fabsf(dz);
        row.may_sphere = sphere_may_hit(s32[k], ox, oy, oz, dx, dy, dz, ia, on, dn) ? 1u : 0u;
    }
    row.may_light = LightPre(o, d).may_hit(R4<double>{c.x, c.y, c.z, r}) ? 1u : 0u;
    out[k] = row;
}

// a tester that accepts nothing: the traversals' ntest counts the leaves entered
struct CountTester {
    V3<double> o, d;
    double tb;
    __device__ __forceinline__ double bound() const { return tb; }
    __device__ __forceinline__ void test(const R4<double>&, int32_t) {}
};

// 64 threads per block: the traversals are wave-wide (every lane calls them)
__global__ void probe_boxes(const double* __restrict__ rec, const float* __restrict__ b32, uint64_t m,
                            BvhNode<float>* __restrict__ nodes32, Bvh4Node<double>* __restrict__ nodes4,
                            const R4<double>* __restrict__ bsph, const R4<float>* __restrict__ bsph32,
                            const uint32_t* __restrict__ bid, BoxRow* __restrict__ out) {
    __shared__ int32_t stack[8 * 64];
    const uint32_t lane = threadIdx.x;
    const uint64_t k = (uint64_t)blockIdx.x * 64 + lane;
    const bool live = k < m;
    const uint64_t kk = live ? k : m - 1;
    const double* p = rec + 13 * kk;
    const float* q = b32 + 6 * kk;
    const V3<double> o = mk(p[0], p[1], p[2]), d = mk(p[3], p[4], p[5]);
    const int32_t leaf1 = ~(int32_t)((0u << 4) | 1u), leaf2 = ~(int32_t)((1u << 4) | 2u);
    if (live) {
        BvhNode<float> nd;
        for (int c = 0; c < 2; ++c) {
            nd.lo_x[c] = q[0];
            nd.lo_y[c] = q[1];
            nd.lo_z[c] = q[2];
            nd.hi_x[c] = q[3];
            nd.hi_y[c] = q[4];
            nd.hi_z[c] = q[5];
        }
        nd.child[0] = leaf1;
        nd.child[1] = leaf2;
        nd.pad[0] = nd.pad[1] = 0;
        nodes32[k] = nd;
        // the octant copies as stage_scene.cpp packs them: near / far planes by the
        // octant's signs, the link's bits in the low half of a double, empty slots
        // near = +inf, far = -inf with an empty leaf
        for (int oct = 0; oct < 8; ++oct) {
            Bvh4Node<double> n4;
            for (int s = 0; s < 4; ++s) {
                const bool valid = s < 2;
                double nr[3], fr[3];
                for (int a = 0; a < 3; ++a) {
                    const bool neg = (oct >> a) & 1;
                    const double lo = valid ? p[6 + a] : (double)INFINITY, hi = valid ? p[9 + a] : -(double)INFINITY;
                    nr[a] = neg ? hi : lo;
                    fr[a] = neg ? lo : hi;
                }
                const int32_t link = valid ? (s == 0 ? leaf1 : leaf2) : ~(int32_t)0;
                const double lr = __longlong_as_double((long long)(uint64_t)(uint32_t)link);
                n4.a[s] = R4<double>{nr[0], nr[1], nr[2], fr[0]};
                n4.b[s] = R4<double>{fr[1], fr[2], lr, 0.0};
            }
            nodes4[8 * k + oct] = n4;
        }
    }
    __syncthreads();
    DevScene<double> sc{};
    sc.bvh32 = nodes32 + kk;
    sc.bsph32 = bsph32;
    sc.bsph = bsph;
    sc.bid = bid;
    sc.bvh4 = nodes4 + 8 * kk;
    sc.n_nodes4 = 1;
    sc.bvh4_stack = 4;
    BoxRow row{0u, 0u};
    uint32_t nvis = 0;
    CountTester T{o, d, p[12]};
    bvh_traverse_ww(sc, 0, o, d, T, stack + lane, nvis, row.ntest_ww, !live);
    __syncthreads();
    bvh4_traverse(sc, 0, o, d, T, stack + lane, nvis, row.ntest_4, !live);
    if (live) out[k] = row;
}

template <typename T>
static std::vector<T> read_n(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "cull_probe: short input\n");
        exit(3);
    }
    return v;
}
template <typename T>
static T* upload(const std::vector<T>& v) {
    T* p = nullptr;
    CHECK(hipMalloc(&p, sizeof(T) * (v.size() + 1)));
    if (!v.empty()) CHECK(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: cull_probe IN OUT\n");
        return 3;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 3;
    }
    const std::vector<uint64_t> head = read_n<uint64_t>(f, 2);
    const uint64_t n = head[0], m = head[1];
    if (n > (1u << 20) || m > (1u << 20)) {
        fprintf(stderr, "cull_probe: at most 2^20 records per launch\n");
        return 3;
    }
    const std::vector<double> rec = read_n<double>(f, 10 * n);
    const std::vector<float> s32 = read_n<float>(f, 4 * n);
    const std::vector<double> box = read_n<double>(f, 13 * m);
    const std::vector<float> b32 = read_n<float>(f, 6 * m);
    fclose(f);

    std::vector<SphereRow> rows(n);
    std::vector<BoxRow> brows(m);
    if (n) {
        double* d_rec = upload(rec);
        float* d_s32 = upload(s32);
        SphereRow* d_out = nullptr;
        CHECK(hipMalloc(&d_out, sizeof(SphereRow) * n));
        CHECK(hipMemset(d_out, 0, sizeof(SphereRow) * n));
        probe_spheres<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(d_rec, reinterpret_cast<const R4<float>*>(d_s32),
                                                                         n, d_out);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(rows.data(), d_out, sizeof(SphereRow) * n, hipMemcpyDeviceToHost));
        CHECK(hipFree(d_rec));
        CHECK(hipFree(d_s32));
        CHECK(hipFree(d_out));
    }
    if (m) {
        double* d_box = upload(box);
        float* d_b32 = upload(b32);
        // three leaf spheres nothing hits (the tester ignores them anyway)
        const std::vector<double> bs(12, 0.0);
        const std::vector<float> bs32(12, 0.0f);
        const std::vector<uint32_t> ids = {0u, 1u, 2u};
        double* d_bs = upload(bs);
        float* d_bs32 = upload(bs32);
        uint32_t* d_ids = upload(ids);
        BvhNode<float>* d_n32 = nullptr;
        Bvh4Node<double>* d_n4 = nullptr;
        BoxRow* d_out = nullptr;
        CHECK(hipMalloc(&d_n32, sizeof(BvhNode<float>) * m));
        CHECK(hipMalloc(&d_n4, sizeof(Bvh4Node<double>) * 8 * m));
        CHECK(hipMalloc(&d_out, sizeof(BoxRow) * m));
        CHECK(hipMemset(d_out, 0, sizeof(BoxRow) * m));
        probe_boxes<<<dim3((unsigned)((m + 63) / 64)), dim3(64)>>>(d_box, d_b32, m, d_n32, d_n4,
                                                                    reinterpret_cast<const R4<double>*>(d_bs),
                                                                    reinterpret_cast<const R4<float>*>(d_bs32), d_ids,
                                                                    d_out);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(brows.data(), d_out, sizeof(BoxRow) * m, hipMemcpyDeviceToHost));
        CHECK(hipFree(d_box));
        CHECK(hipFree(d_b32));
        CHECK(hipFree(d_bs));
        CHECK(hipFree(d_bs32));
        CHECK(hipFree(d_ids));
        CHECK(hipFree(d_n32));
        CHECK(hipFree(d_n4));
        CHECK(hipFree(d_out));
    }
    FILE* g = fopen(argv[2], "wb");
    if (!g) {
        perror(argv[2]);
        return 3;
    }
    if ((n && fwrite(rows.data(), sizeof(SphereRow), n, g) != n) ||
        (m && fwrite(brows.data(), sizeof(BoxRow), m, g) != m) || fclose(g) != 0) {
        fprintf(stderr, "cull_probe: cannot write %s\n", argv[2]);
        return 3;
    }
    printf("cull_probe: %llu sphere records, %llu box records\n", (unsigned long long)n, (unsigned long long)m);
    return 0;
}
