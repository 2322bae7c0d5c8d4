// features_kernels.h -- host-visible description of the feature pass
// (rtw_render_features): its parameter block and the launch entry points of
// features_f32.hip / features_f64.hip.  The pass traces the render's own
// primary rays -- the (seed, pixel, sample) stream of render_kernel's
// start_sample -- to their first hit and folds 8 channels per pixel in f64:
// albedo [0..2], shading normal [3..5], distance [6], hits [7].  It reads the
// staged scene (rtw_kernels.h DevScene) with the worlds, the LDS layout and
// the counters of the ray queries (query_kernels.h) and nothing of the render's.
#pragma once

#include "query_kernels.h"

namespace rtw {

constexpr uint32_t kFeatureChannels = 8;
// the tile counter follows the query counters in the context's counter block
constexpr int kFeatureNextTile = kQueryCounters;

template <typename R>
struct FParams {
    DevScene<R> sc;
    R center[3], p00[3], du[3], dv[3], disk_u[3], disk_v[3], bg[3];   // KParams's camera (pass_params)
    R u_scale;                        // Uniform::new_inclusive(-0.5, 0.5) scale
    uint64_t seed;
    uint32_t defocus;                 // defocus_angle > f64::EPSILON
    uint32_t W, H;
    uint32_t first, end;              // the samples [first, end) of every pixel, clipped by counts
    uint32_t tiles_x, n_tiles;        // 8 x 8 tiles across, in all
    uint32_t stack;                   // per-lane traversal stack entries (BVH worlds)
    const uint32_t* counts;           // null, or [H][W]: pixel p stops at counts[p]
    double* features;                 // [H][W][8] sums, read when first > 0 (16-byte aligned)
    int32_t* ids;                     // null, or [H][W][2] {object or -1, material} of sample 0
    unsigned long long* counters;     // kQueryCounters, then the next tile (kFeatureNextTile)
};

// Launches (features_f32.hip / features_f64.hip) on `stream`: p.n_tiles > 0, the
// world / test form / LDS of the query plan (hit_kernel_exists names the kernels).
// Each returns the world launched, or -1 (no such kernel, or the launch failed).
int launch_primary_features(const FParams<float>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                            hipStream_t stream);
int launch_primary_features(const FParams<double>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                            hipStream_t stream);

}  // namespace rtw
