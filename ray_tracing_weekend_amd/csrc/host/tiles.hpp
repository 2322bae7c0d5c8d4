// tiles.hpp -- the 8x8 tile arithmetic of the rank split: tile counts, the
// tiles of a rank (a dealt split or the round robin), the image <-> a rank's
// packed tiles, the assembly's slot map and the deal itself.  Host only, no HIP
// call.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../../include/rtw.h"
#include "../rtw_kernels.h"

namespace rtw {

inline uint32_t tiles_across(uint32_t pixels) { return (pixels + kTile - 1) / kTile; }

inline uint64_t n_tiles_of(uint32_t W, uint32_t H) { return (uint64_t)tiles_across(W) * tiles_across(H); }

// the round robin's tile count of `rank`; a dealt split keeps it
inline uint32_t tiles_for_rank(uint32_t W, uint32_t H, uint32_t rank, uint32_t nranks) {
    if (nranks == 0 || rank >= nranks) return 0;
    const uint64_t n = n_tiles_of(W, H);
    return rank < n ? (uint32_t)((n - rank + nranks - 1) / nranks) : 0u;
}

// the bytes of n_tiles packed tiles [tile][64][3] of elements of elem_bytes
inline size_t packed_bytes(uint32_t n_tiles, size_t elem_bytes) { return (size_t)n_tiles * 64 * 3 * elem_bytes; }

// the global tiles of `rank`, in the order they are packed (increasing T);
// split_rank null: the round robin
inline void local_tiles(const std::vector<uint32_t>* split_rank, uint32_t W, uint32_t H, uint32_t rank,
                        uint32_t nranks, std::vector<uint32_t>& out) {
    out.clear();
    const uint64_t n = n_tiles_of(W, H);
    if (split_rank) {
        for (uint64_t T = 0; T < n; ++T)
            if ((*split_rank)[T] == rank) out.push_back((uint32_t)T);
    } else {
        for (uint64_t T = rank; T < n; T += nranks) out.push_back((uint32_t)T);
    }
}

// pixels inside the image of these tiles
inline uint64_t tile_pixels(uint32_t W, uint32_t H, const std::vector<uint32_t>& tiles) {
    const uint32_t tiles_x = tiles_across(W);
    uint64_t px = 0;
    for (uint32_t T : tiles) {
        const uint32_t tx = T % tiles_x, ty = T / tiles_x;
        px += (uint64_t)std::min(kTile, W - tx * kTile) * std::min(kTile, H - ty * kTile);
    }
    return px;
}

// f(the pixel's offset in the image [H][W][3], its offset in the packed tiles
// [lt][ly * 8 + lx][3]) for every pixel of `tiles` (a rank's, in packed order)
// that lies inside the image
template <typename F>
inline void each_packed_pixel(uint32_t W, uint32_t H, const std::vector<uint32_t>& tiles, F&& f) {
    const uint32_t tiles_x = tiles_across(W);
    for (size_t lt = 0; lt < tiles.size(); ++lt) {
        const uint32_t tx = tiles[lt] % tiles_x, ty = tiles[lt] / tiles_x;
        for (uint32_t px = 0; px < 64; ++px) {
            const uint32_t i = tx * kTile + (px & 7u), j = ty * kTile + (px >> 3);
            if (i < W && j < H) f(((size_t)j * W + i) * 3, (lt * 64 + px) * 3);
        }
    }
}

// the image [H][W][3] -> a rank's packed tiles (tiles.size() * 64 * 3 values;
// pixels outside the image: 0)
inline void image_to_packed(const double* img, uint32_t W, uint32_t H, const std::vector<uint32_t>& tiles,
                            double* packed) {
    std::fill(packed, packed + tiles.size() * 64 * 3, 0.0);
    each_packed_pixel(W, H, tiles, [&](size_t at, size_t pk) {
        for (int k = 0; k < 3; ++k) packed[pk + k] = img[at + k];
    });
}

// a rank's packed tiles -> its pixels of the image [H][W][3] (the others untouched)
inline void packed_to_image(const double* packed, uint32_t W, uint32_t H, const std::vector<uint32_t>& tiles,
                            double* img) {
    each_packed_pixel(W, H, tiles, [&](size_t at, size_t pk) {
        for (int k = 0; k < 3; ++k) img[at + k] = packed[pk + k];
    });
}

// the assembly's map of a split: global tile T -> lt * n + rank (the round
// robin's own index form, so the assembly kernel decodes both alike)
inline std::vector<uint32_t> tile_slots(const std::vector<uint32_t>& split_rank, uint32_t nranks) {
    std::vector<uint32_t> slot(split_rank.size());
    std::vector<uint32_t> next(nranks, 0);
    for (size_t T = 0; T < slot.size(); ++T) {
        const uint32_t k = split_rank[T];
        slot[T] = next[k]++ * nranks + k;
    }
    return slot;
}

// rtw_split_deal
inline int split_deal(const uint32_t* tile_cost, uint32_t W, uint32_t H, uint32_t nranks, uint32_t* tile_rank) {
    if (nranks == 0 || nranks > RTW_MAX_RANKS) return RTW_E_INVALID;
    const uint64_t n = n_tiles_of(W, H);
    if (n > 0xFFFFFFFFull / nranks) return RTW_E_UNSUPPORTED;
    if (n && (!tile_cost || !tile_rank)) return RTW_E_INVALID;
    // costliest tiles first (ties: lower index), each to the rank of least dealt
    // cost (ties: lower rank) among those below their round-robin tile count
    std::vector<uint32_t> order(n);
    for (uint64_t T = 0; T < n; ++T) order[T] = (uint32_t)T;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return tile_cost[a] > tile_cost[b]; });
    std::vector<uint64_t> load(nranks, 0);
    std::vector<uint32_t> room(nranks);
    for (uint32_t r = 0; r < nranks; ++r) room[r] = tiles_for_rank(W, H, r, nranks);
    for (uint32_t T : order) {
        uint32_t best = nranks;
        for (uint32_t r = 0; r < nranks; ++r)
            if (room[r] && (best == nranks || load[r] < load[best])) best = r;
        tile_rank[T] = best;
        load[best] += tile_cost[T];
        --room[best];
    }
    return RTW_OK;
}

// a split is valid: every tile has a rank < nranks, and rank r exactly its
// round-robin tile count (tile_rank null: the round robin itself)
inline int check_split(uint32_t W, uint32_t H, uint32_t nranks, const uint32_t* tile_rank) {
    if (nranks == 0 || nranks > RTW_MAX_RANKS) return RTW_E_INVALID;
    const uint64_t n = n_tiles_of(W, H);
    if (n > 0xFFFFFFFFull / nranks) return RTW_E_UNSUPPORTED;
    if (!tile_rank) return RTW_OK;
    std::vector<uint32_t> cnt(nranks, 0);
    for (uint64_t T = 0; T < n; ++T) {
        if (tile_rank[T] >= nranks) return RTW_E_INVALID;
        ++cnt[tile_rank[T]];
    }
    for (uint32_t r = 0; r < nranks; ++r)
        if (cnt[r] != tiles_for_rank(W, H, r, nranks)) return RTW_E_INVALID;
    return RTW_OK;
}

}  // namespace rtw
