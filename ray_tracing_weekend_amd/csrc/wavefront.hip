// wavefront.hip -- the kernels of the wavefront path rounds (wavefront_kernel.hpp)
// in both precisions, and their launches.  Built with -ffp-contract=off: the
// fold rounds every product before its add, as the host loop it restates does.
#include "query_launch.hpp"
#include "wavefront_kernel.hpp"

namespace rtw {

namespace {

inline uint64_t blocks_of(uint64_t n) { return (n + kQueryBlock - 1) / kQueryBlock; }

template <typename R>
int begin_t(const PathBegin<R>& p, uint32_t grid_cap, hipStream_t stream) {
    return launch_resident(&dev::path_begin_kernel<R>, blocks_of(p.n), p, 0, grid_cap, stream);
}
template <typename R>
int advance_t(const PathAdvance<R>& p, uint32_t grid_cap, hipStream_t stream) {
    return launch_resident(&dev::path_advance_kernel<R>, blocks_of(p.n), p, 0, grid_cap, stream);
}

}  // namespace

int launch_path_begin(const PathBegin<float>& p, uint32_t grid_cap, hipStream_t stream) {
    return begin_t(p, grid_cap, stream);
}
int launch_path_begin(const PathBegin<double>& p, uint32_t grid_cap, hipStream_t stream) {
    return begin_t(p, grid_cap, stream);
}
int launch_path_advance(const PathAdvance<float>& p, uint32_t grid_cap, hipStream_t stream) {
    return advance_t(p, grid_cap, stream);
}
int launch_path_advance(const PathAdvance<double>& p, uint32_t grid_cap, hipStream_t stream) {
    return advance_t(p, grid_cap, stream);
}

int launch_path_fold(bool f64, const PathFold& p, uint32_t grid_cap, hipStream_t stream) {
    if (f64) return launch_resident(&dev::path_fold_kernel<double>, blocks_of(p.n), p, 0, grid_cap, stream);
    return launch_resident(&dev::path_fold_kernel<float>, blocks_of(p.n), p, 0, grid_cap, stream);
}

}  // namespace rtw
