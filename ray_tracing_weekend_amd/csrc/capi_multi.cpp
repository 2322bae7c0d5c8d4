// capi_multi.cpp -- multi-device contexts of the C-ABI (include/rtw.h): one
// rank per GPU (or virtual ranks on one), the whole-image render, the gather
// to rank 0 that it shares with the window and adaptive renders over the ranks
// (gather_ranks, gather_done), and the stats summed over the ranks.
#include <dlfcn.h>

#include <algorithm>
#include <mutex>
#include <type_traits>

#include "capi_ctx.hpp"

namespace {

// RCCL for the multi-device gather, resolved at the first multi-device
// context: dlopen by SONAME, so a process that already holds PyTorch's
// librccl.so.1 shares that copy (one RCCL per process); a plain C caller gets
// ROCm's.  Single-device contexts never load it.
struct RcclApi {
    bool ok = false;
    std::string err;
    ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*gather)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*group_start)() = nullptr;
    ncclResult_t (*group_end)() = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
};

const RcclApi& rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = nullptr;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) != nullptr) break;
        if (!h) {
            api.err = std::string("cannot load librccl.so.1: ") + dlerror();
            return;
        }
        auto sym = [&](auto& fn, const char* name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name));
            if (!fn && api.err.empty()) api.err = std::string("librccl.so.1 lacks ") + name;
        };
        sym(api.comm_init_all, "ncclCommInitAll");
        sym(api.comm_destroy, "ncclCommDestroy");
        sym(api.gather, "ncclGather");
        sym(api.group_start, "ncclGroupStart");
        sym(api.group_end, "ncclGroupEnd");
        sym(api.error_string, "ncclGetErrorString");
        api.ok = api.err.empty();
    });
    return api;
}

int rccl_fail(rtw_ctx* c, ncclResult_t r, const char* what) {
    const RcclApi& a = rccl_api();
    return fail(c, RTW_E_DEVICE, std::string(what) + ": " + (a.error_string ? a.error_string(r) : "RCCL error"));
}

}  // namespace

int gather_ranks(rtw_ctx* c, const std::vector<const void*>& src, size_t count, size_t elem_bytes, hipStream_t s0) {
    const uint32_t n = rtw_device_count(c);
    const size_t bytes = count * elem_bytes;
    if (c->virt) {
        // test mode (rtw_create_virtual): the gather as device copies on rank 0's
        // stream, each after its rank's work -- the same slots an RCCL gather
        // to root 0 fills
        for (uint32_t k = 1; k < n; ++k) {
            rtw_ctx* ck = rtw_device_ctx(c, k);
            HIP_TRY(c, hipEventRecord(c->peer_ev[k - 1], ck->stream));
            HIP_TRY(c, hipStreamWaitEvent(s0, c->peer_ev[k - 1], 0));
            HIP_TRY(c, hipMemcpyAsync(static_cast<unsigned char*>(c->d_gather) + (size_t)k * bytes, src[k], bytes,
                                      hipMemcpyDeviceToDevice, s0));
        }
        return RTW_OK;
    }
    // ONE gather of the packed buffers to rank 0 (RCCL over xGMI), ordered after
    // each rank's work on that rank's stream
    const RcclApi& api = rccl_api();
    const ncclDataType_t dt = elem_bytes == 4 ? ncclFloat32 : elem_bytes == 8 ? ncclFloat64 : ncclUint8;
    const size_t cnt = elem_bytes == 4 || elem_bytes == 8 ? count : bytes;
    ncclResult_t r = api.group_start();
    if (r != ncclSuccess) return rccl_fail(c, r, "ncclGroupStart");
    for (uint32_t k = 0; k < n; ++k) {
        rtw_ctx* ck = rtw_device_ctx(c, k);
        r = api.gather(k ? src[k] : c->d_gather, k ? nullptr : c->d_gather, cnt, dt, 0, c->comms[k],
                       k ? ck->stream : s0);
        if (r != ncclSuccess) {
            (void)api.group_end();
            return rccl_fail(c, r, "ncclGather");
        }
    }
    r = api.group_end();
    if (r != ncclSuccess) return rccl_fail(c, r, "ncclGroupEnd");
    return RTW_OK;
}

int gather_done(rtw_ctx* c, hipStream_t s0) {
    // every rank's next render waits for this gather + assembly (a peer's
    // packed buffer is read on s0 in the virtual mode; d_gather always)
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventRecord(c->gather_ev, s0));
    for (uint32_t k = 1; k < rtw_device_count(c); ++k) {
        rtw_ctx* ck = rtw_device_ctx(c, k);
        HIP_TRY(c, hipSetDevice(ck->device));
        HIP_TRY(c, hipStreamWaitEvent(ck->stream, c->gather_ev, 0));
    }
    HIP_TRY(c, hipSetDevice(c->device));
    c->gather_pending = true;
    return RTW_OK;
}

void destroy_ranks(rtw_ctx* c) {
    if (!c->comms.empty()) {
        // the gathers may still run on any rank's stream (rank 0's is the caller's)
        for (uint32_t k = 0; k < rtw_device_count(c); ++k) {
            (void)hipSetDevice(rtw_device_ctx(c, k)->device);
            (void)hipDeviceSynchronize();
        }
        const RcclApi& api = rccl_api();
        for (ncclComm_t m : c->comms)
            if (m && api.comm_destroy) (void)api.comm_destroy(m);
        c->comms.clear();
    }
    if (c->virt)   // the device copies of the last gather read the peers' buffers on rank 0's device
        for (uint32_t k = 0; k < rtw_device_count(c); ++k) {
            (void)hipSetDevice(rtw_device_ctx(c, k)->device);
            (void)hipDeviceSynchronize();
        }
    for (size_t k = 0; k < c->peer_ev.size(); ++k) {
        (void)hipSetDevice(c->peers[k]->device);
        if (c->peer_ev[k]) (void)hipEventDestroy(c->peer_ev[k]);
    }
    c->peer_ev.clear();
    for (rtw_ctx* pk : c->peers) rtw_destroy(pk);
    c->peers.clear();
}

extern "C" {

int rtw_visible_devices(void) {
    int visible = 0;
    return hipGetDeviceCount(&visible) == hipSuccess ? visible : RTW_E_DEVICE;
}

// the rank contexts of a multi-device context (devices[0] = rank 0 = the
// returned context) plus the events that order consecutive gathers
static int create_ranks(const int* devices, uint32_t n, int precision, rtw_ctx** out) {
    rtw_ctx* c = rtw_create(devices[0], precision);
    if (!c) return RTW_E_DEVICE;
    c->multi = true;
    for (uint32_t k = 1; k < n; ++k) {
        rtw_ctx* pk = rtw_create(devices[k], precision);
        if (!pk) {
            rtw_destroy(c);
            return RTW_E_DEVICE;
        }
        c->peers.push_back(pk);
        hipEvent_t e = nullptr;
        if (hipSetDevice(devices[k]) != hipSuccess || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            rtw_destroy(c);
            return RTW_E_DEVICE;
        }
        c->peer_ev.push_back(e);
    }
    if (hipSetDevice(devices[0]) != hipSuccess ||
        hipEventCreateWithFlags(&c->gather_ev, hipEventDisableTiming) != hipSuccess) {
        rtw_destroy(c);
        return RTW_E_DEVICE;
    }
    *out = c;
    return RTW_OK;
}

int rtw_create_devices(const int* devices, uint32_t n_devices, int precision, rtw_ctx** out) {
    if (!out) return RTW_E_INVALID;
    *out = nullptr;
    if (!devices || n_devices == 0 || (precision != RTW_F32 && precision != RTW_F64)) return RTW_E_INVALID;
    // the device list is checked before any HIP call: no negative or repeated
    // device (one rank per GPU: a repeated device would render its tiles twice
    // and RCCL rejects a clique with a duplicate device)
    for (uint32_t a = 0; a < n_devices; ++a) {
        if (devices[a] < 0) return RTW_E_INVALID;
        for (uint32_t b = 0; b < a; ++b)
            if (devices[a] == devices[b]) return RTW_E_INVALID;
    }
    const int visible = rtw_visible_devices();
    if (visible < 0) return RTW_E_DEVICE;
    for (uint32_t a = 0; a < n_devices; ++a)
        if (devices[a] >= visible) return RTW_E_INVALID;
    const RcclApi& api = rccl_api();
    if (!api.ok) return RTW_E_DEVICE;
    rtw_ctx* c = nullptr;
    const int rc = create_ranks(devices, n_devices, precision, &c);
    if (rc) return rc;
    c->comms.assign(n_devices, nullptr);
    const std::vector<int> list(devices, devices + n_devices);
    if (api.comm_init_all(c->comms.data(), (int)n_devices, list.data()) != ncclSuccess) {
        c->comms.clear();
        rtw_destroy(c);
        return RTW_E_DEVICE;
    }
    (void)hipSetDevice(devices[0]);
    *out = c;
    return RTW_OK;
}

int rtw_create_virtual(int device, uint32_t n_ranks, int precision, rtw_ctx** out) {
    if (!out) return RTW_E_INVALID;
    *out = nullptr;
    if (device < 0 || n_ranks == 0 || n_ranks > 64 || (precision != RTW_F32 && precision != RTW_F64))
        return RTW_E_INVALID;
    const int visible = rtw_visible_devices();
    if (visible < 0) return RTW_E_DEVICE;
    if (device >= visible) return RTW_E_INVALID;
    const std::vector<int> list(n_ranks, device);
    rtw_ctx* c = nullptr;
    const int rc = create_ranks(list.data(), n_ranks, precision, &c);
    if (rc) return rc;
    c->virt = true;
    *out = c;
    return RTW_OK;
}

int rtw_create_mask_ex(uint64_t device_mask, int precision, rtw_ctx** out) {
    if (!out) return RTW_E_INVALID;
    *out = nullptr;
    std::vector<int> list;
    for (int k = 0; k < 64; ++k)
        if ((device_mask >> k) & 1u) list.push_back(k);
    if (list.empty()) return RTW_E_INVALID;
    return rtw_create_devices(list.data(), (uint32_t)list.size(), precision, out);
}

rtw_ctx* rtw_create_mask(uint64_t device_mask, int precision) {
    rtw_ctx* c = nullptr;
    return rtw_create_mask_ex(device_mask, precision, &c) == RTW_OK ? c : nullptr;
}

uint32_t rtw_device_count(const rtw_ctx* c) { return c ? 1u + (uint32_t)c->peers.size() : 0u; }

rtw_ctx* rtw_device_ctx(rtw_ctx* c, uint32_t k) {
    if (!c) return nullptr;
    if (k == 0) return c;
    return k <= c->peers.size() ? c->peers[k - 1] : nullptr;
}

int rtw_device_of(const rtw_ctx* c) { return c ? c->device : RTW_E_INVALID; }

int rtw_render_image_device(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, void* d_image, size_t image_bytes,
                            void* stream) {
    if (!c || !cam) return fail(c, RTW_E_INVALID, "bad argument");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    const uint32_t W = cam->image_width, H = cam->image_height, n = rtw_device_count(c);
    const size_t esz = c->precision == RTW_F32 ? sizeof(float) : sizeof(double);
    const size_t img = (size_t)W * H * 3 * esz;
    if (image_bytes < img || (img && !d_image)) return fail(c, RTW_E_INVALID, "d_image is smaller than W*H*3");
    hipStream_t s0 = resolve_stream(c, stream);
    // rank k renders the tiles T = k (mod n) into a packed buffer of rank 0's
    // size (the most tiles: RCCL gathers equal counts)
    const size_t per = std::max<size_t>((size_t)rtw_tiles_for_rank(W, H, 0, n) * 64 * 3, 1);
    if (!c->multi) {
        // one device, no collective: the packed tiles -> the image
        HIP_TRY(c, hipSetDevice(c->device));
        int rc = ensure(c, &c->d_out, &c->out_cap, per * esz);
        if (rc) return rc;
        rc = rtw_render_device(c, cam, seed, 0, 1, c->d_out, c->out_cap, stream);
        if (rc) return rc;
        return img ? rtw_assemble_tiles(c, c->d_out, c->out_cap, 1, W, H, d_image, stream) : RTW_OK;
    }
    // Balance (tuning "balance"): once every rank has counted its tiles' costs
    // for this camera and scene (the first render of a key counts them), deal
    // the tiles to the ranks by those costs (rtw_split_deal) -- the reference
    // balances its pixels dynamically over the host cores, camera.rs:340-353.
    // The image does not depend on the split (every pixel's samples are its own).
    const bool have = c->split.active(W, H, n);
    if (c->knobs.balance && n > 1 && img &&
        (!have || (c->split.automatic && (c->split.scene != c->scene_serial ||
                                          memcmp(&c->split.cam, cam, sizeof *cam) != 0)))) {
        bool all = true;
        for (uint32_t k = 0; k < n && all; ++k) {
            const rtw_ctx* ck = rtw_device_ctx(c, k);
            all = ck->lpt.st.has(lpt_key(ck, cam, k, n));
        }
        if (all) {
            std::vector<uint32_t> cost(rtw::n_tiles_of(W, H), 0), owner(cost.size(), 0);
            for (uint32_t k = 0; k < n; ++k) {
                rtw_ctx* ck = rtw_device_ctx(c, k);
                const int rc = tile_costs_of(ck, cam, k, n, cost.data());
                if (rc) return k ? fail(c, rc, ck->err) : rc;
            }
            int rc = rtw_split_deal(cost.data(), W, H, n, owner.data());
            if (rc) return fail(c, rc, "rtw_split_deal failed");
            for (uint32_t k = 0; k < n; ++k)
                apply_split(rtw_device_ctx(c, k), W, H, n, owner.data(), cost.data(), true, cam);
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // (the previous call's gather + assembly, possibly on another stream: rank
    // 0's render below waits for gather_ev (rtw_render_device), the peers'
    // streams were made to wait for it when it was recorded; a reallocation of
    // d_gather in `ensure` synchronises the device)
    int rc = ensure(c, &c->d_gather, &c->gather_cap, (size_t)n * per * esz);
    if (rc) return rc;
    // launch every rank's share (asynchronous, each device on its own stream);
    // rank 0 renders in place into its slot of the gather target
    for (uint32_t k = 0; k < n; ++k) {
        rtw_ctx* ck = rtw_device_ctx(c, k);
        HIP_TRY(c, hipSetDevice(ck->device));
        void* dst = c->d_gather;
        if (k) {
            rc = ensure(ck, &ck->d_out, &ck->out_cap, per * esz);
            if (rc) return fail(c, rc, ck->err);
            dst = ck->d_out;
        }
        rc = rtw_render_device(ck, cam, seed, k, n, dst, per * esz, k ? (void*)ck->stream : stream);
        if (rc) return k ? fail(c, rc, ck->err) : rc;
    }
    std::vector<const void*> src(n, c->d_gather);
    for (uint32_t k = 1; k < n; ++k) src[k] = rtw_device_ctx(c, k)->d_out;
    rc = gather_ranks(c, src, per, esz, s0);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // rank 0 un-interleaves the n buffers into the image
    rc = img ? rtw_assemble_tiles(c, c->d_gather, per * esz, n, W, H, d_image, stream) : RTW_OK;
    if (rc) return rc;
    rc = gather_done(c, s0);
    if (rc) return rc;
    c->stats_ranks = n;
    return RTW_OK;
}

int rtw_get_stats(rtw_ctx* c, rtw_stats* out) {
    if (!c || !out) return RTW_E_INVALID;
    if (!c->peers.empty() && c->stats_ranks > 1) {
        // multi-device: the counters summed over the ranks of the last render,
        // kernel_ms the slowest rank's; the rest as rank 0 reports it (after a
        // rank-0-only rtw_render_device: rank 0's alone)
        rtw_stats sum{};
        int worst = RTW_OK;
        for (uint32_t k = 0; k < std::min(c->stats_ranks, rtw_device_count(c)); ++k) {
            rtw_ctx* ck = rtw_device_ctx(c, k);
            rtw_stats st{};
            const int rc = get_stats_one(ck, &st);
            if (rc == RTW_E_DEVICE || rc == RTW_E_INVALID) return k ? fail(c, rc, ck->err) : rc;
            if (rc && !worst) {
                worst = rc;
                if (k) c->err = ck->err;
            }
            if (k == 0) sum = st;
            else {
                sum.samples += st.samples;
                sum.segments += st.segments;
                sum.lambertian += st.lambertian;
                sum.node_visits += st.node_visits;
                sum.sphere_tests += st.sphere_tests;
                sum.panic_plane_uv += st.panic_plane_uv;
                sum.panic_no_lights += st.panic_no_lights;
                sum.light_tests += st.light_tests;
                sum.grid_cells += st.grid_cells;
                sum.kernel_ms = std::max(sum.kernel_ms, st.kernel_ms);
            }
        }
        (void)hipSetDevice(c->device);
        *out = sum;
        return worst;
    }
    return get_stats_one(c, out);
}

}  // extern "C"
