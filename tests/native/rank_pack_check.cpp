// rank_pack_check.cpp -- CPU check of host/tiles.hpp's image <-> packed-rank
// helpers (image_to_packed, packed_to_image): for 37 x 23 and 16 x 8 images over
// 1, 2, 3 and 8 ranks, under the round robin and under a split dealt from
// synthetic costs, every rank's packed tiles hold its pixels where the
// assembly's decoding (tile_slots, or T itself) looks for them and zeros outside
// the image, and the ranks' parts put back give the image.  Every case is also
// printed for the restatement in tests/test_rank_pack_host.py, which builds and
// runs this:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -I<csrc> -I<include> rank_pack_check.cpp -o rank_pack_check
// Lines: "CASE W H n split", "SPLIT ranks..." (a dealt split), per rank
// "TILES k tiles..." and "PACKED k values..." (the image holds the value
// (j * W + i) * 3 + c + 1 at pixel (i, j), channel c: integers, exact).
#include <stdio.h>

#include <vector>

#include "host/tiles.hpp"

static int g_wrong = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++g_wrong;                   \
            printf("WRONG: " __VA_ARGS__); \
            printf("\n");                \
        }                                \
    } while (0)

// the synthetic, uneven tile costs of the dealt cases (restated in the test)
static uint32_t cost_of(uint32_t T) { return (T * 7919u) % 13u + (T % 3u == 0 ? 40u : 1u); }

static void check_case(uint32_t W, uint32_t H, uint32_t n, bool dealt) {
    const uint32_t nt = (uint32_t)rtw::n_tiles_of(W, H), tiles_x = rtw::tiles_across(W);
    printf("CASE %u %u %u %d\n", W, H, n, dealt ? 1 : 0);
    std::vector<uint32_t> split, slot(nt);
    if (dealt) {
        std::vector<uint32_t> cost(nt);
        for (uint32_t T = 0; T < nt; ++T) cost[T] = cost_of(T);
        split.resize(nt);
        CHECK(rtw::split_deal(cost.data(), W, H, n, split.data()) == RTW_OK, "split_deal failed");
        CHECK(rtw::check_split(W, H, n, split.data()) == RTW_OK, "the dealt split is not valid");
        slot = rtw::tile_slots(split, n);
        printf("SPLIT");
        for (uint32_t r : split) printf(" %u", r);
        printf("\n");
    } else {
        for (uint32_t T = 0; T < nt; ++T) slot[T] = T;
    }
    std::vector<double> img((size_t)W * H * 3), back((size_t)W * H * 3, -1.0);
    for (size_t k = 0; k < img.size(); ++k) img[k] = (double)(k + 1);
    std::vector<uint32_t> tiles, seen(nt, 0);
    for (uint32_t r = 0; r < n; ++r) {
        rtw::local_tiles(dealt ? &split : nullptr, W, H, r, n, tiles);
        CHECK(tiles.size() == rtw::tiles_for_rank(W, H, r, n), "rank %u of %u has %zu tiles", r, n, tiles.size());
        printf("TILES %u", r);
        for (uint32_t T : tiles) printf(" %u", T);
        printf("\n");
        // one element more on either side: the helpers stay inside tiles.size() * 64 * 3
        std::vector<double> buf(tiles.size() * 64 * 3 + 2, -7.0);
        double* packed = buf.data() + 1;
        rtw::image_to_packed(img.data(), W, H, tiles, packed);
        CHECK(buf.front() == -7.0 && buf.back() == -7.0, "rank %u: image_to_packed wrote outside its buffer", r);
        printf("PACKED %u", r);
        for (size_t k = 0; k < tiles.size() * 64 * 3; ++k) printf(" %.0f", packed[k]);
        printf("\n");
        for (size_t lt = 0; lt < tiles.size(); ++lt) {
            const uint32_t T = tiles[lt];
            CHECK(T < nt && !seen[T], "rank %u: tile %u twice or out of range", r, T);
            if (T >= nt) continue;
            ++seen[T];
            CHECK(lt == 0 || tiles[lt - 1] < T, "rank %u: tiles not ascending at %zu", r, lt);
            // the assembly finds tile T at rank slot % n, local tile slot / n
            CHECK(slot[T] % n == r && slot[T] / n == lt, "tile %u: slot %u, packed at rank %u local %zu", T, slot[T], r, lt);
            const uint32_t tx = T % tiles_x, ty = T / tiles_x;
            for (uint32_t px = 0; px < 64; ++px) {
                const uint32_t i = tx * 8 + (px & 7u), j = ty * 8 + (px >> 3);
                for (uint32_t c = 0; c < 3; ++c) {
                    const double v = packed[(lt * 64 + px) * 3 + c];
                    const double want = i < W && j < H ? img[((size_t)j * W + i) * 3 + c] : 0.0;
                    CHECK(v == want, "rank %u tile %u pixel %u channel %u: %.0f, expected %.0f", r, T, px, c, v, want);
                }
            }
        }
        rtw::packed_to_image(packed, W, H, tiles, back.data());
    }
    for (uint32_t T = 0; T < nt; ++T) CHECK(seen[T] == 1, "tile %u belongs to %u ranks", T, seen[T]);
    CHECK(back == img, "%u x %u over %u ranks: the ranks' parts do not give the image back", W, H, n);
}

int main() {
    const uint32_t sizes[][2] = {{37, 23}, {16, 8}};
    const uint32_t ranks[] = {1, 2, 3, 8};
    for (const auto& s : sizes)
        for (uint32_t n : ranks)
            for (int dealt = 0; dealt < 2; ++dealt) check_case(s[0], s[1], n, dealt != 0);
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
