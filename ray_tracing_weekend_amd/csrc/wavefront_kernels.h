// wavefront_kernels.h -- host-visible description of the wavefront path rounds
// (rtw_path_begin / rtw_path_advance / rtw_render_wavefront): the parameter
// blocks of the three kernels and the launch entry points of wavefront.hip.
// The kernels read no scene: a path state, the arrays one round of
// rtw_shade_rays wrote, a colour array and counters (query_kernels.h).
#pragma once

#include "path_kernels.h"

namespace rtw {

// rtw_query_stats.is_light_pdf of one advance and of the driver
enum : uint32_t { kQueryPathAdvance = 6, kQueryWavefront = 7 };

// path_begin_kernel: paths k < n start with mult = 1, res = 0, slot = first_slot + k
template <typename R>
struct PathBegin {
    R* mult;                          // n x 3
    R* res;                           // n x 3
    uint32_t* slot;                   // n
    uint64_t n;
    uint32_t first_slot;
};

// path_advance_kernel: one round's fold (camera.rs:470-521) and the compaction
// of the paths that go on
template <typename R>
struct PathAdvance {
    // the round, as shade_rays_kernel wrote it (rng: advanced in place by it)
    const int32_t* event;             // n
    const R* weight;                  // n x 3
    const R* emitted;                 // n x 3
    const R* next;                    // n x 6 {p, direction}
    const uint64_t* rng;              // n x 4
    // the state the round started from
    const R* mult;                    // n x 3
    const R* res;                     // n x 3
    const uint32_t* slot;             // n
    // the survivors' state, appended at *count: none of it overlaps the above
    R* out_rays;                      // x 6: the survivors' `next`
    uint64_t* out_rng;                // x 4
    R* out_mult;                      // x 3
    R* out_res;                       // x 3
    uint32_t* out_slot;
    R* colour;                        // colour_slots x 3: a path that ends writes colour[slot]
    uint64_t colour_slots;            // (a slot beyond it is skipped)
    unsigned long long* count;        // the survivors so far (zero before the launch)
    unsigned long long* counters;     // kQueryCounters: rays += n, hits += survivors or SCATTER events
    uint64_t n;
    R bg[3];                          // the camera's background
    uint32_t last;                    // the round at max_depth - 1: a survivor ends with 0 + res'
    uint32_t count_scatter;           // hits counts the SCATTER events (the driver's `lambertian`)
};

// path_fold_kernel: sums[i] += (double)colour[b * n + i] for b = 0 .. batch - 1, in that order
struct PathFold {
    const void* colour;               // batch x n values of the kernel's precision
    double* sums;                     // n = W * H * 3
    uint64_t n;
    uint32_t batch;
};

// Launches (wavefront.hip) on `stream`: n > 0.  0, or -1: the launch failed.
// grid_cap: tuning "query_grid" (query_kernels.h).
int launch_path_begin(const PathBegin<float>& p, uint32_t grid_cap, hipStream_t stream);
int launch_path_begin(const PathBegin<double>& p, uint32_t grid_cap, hipStream_t stream);
int launch_path_advance(const PathAdvance<float>& p, uint32_t grid_cap, hipStream_t stream);
int launch_path_advance(const PathAdvance<double>& p, uint32_t grid_cap, hipStream_t stream);
int launch_path_fold(bool f64, const PathFold& p, uint32_t grid_cap, hipStream_t stream);

}  // namespace rtw
