// query_grid_check.cpp -- CPU check of the grid of a query, feature or
// wavefront launch (host/query_plan.hpp query_grid): min(blocks, resident,
// tuning "query_grid" or no cap), never 0 for blocks > 0.  Header only (the
// header's includes name HIP types, so it is compiled by hipcc's host pass):
// built and run by tests/test_query_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -I<csrc> -I<include> query_grid_check.cpp
// (the test also builds it with -fsanitize=address,undefined: a host program, run alone)
#include <stdio.h>

#include "host/query_plan.hpp"

static int g_wrong = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            ++g_wrong;                     \
            printf("WRONG: " __VA_ARGS__); \
            printf("\n");                  \
        }                                  \
    } while (0)

using rtw::query_grid;

// the rule, restated with plain comparisons
static uint64_t restated(uint64_t blocks, uint64_t resident, uint32_t cap) {
    uint64_t g = blocks;
    if (resident < g) g = resident;
    if (cap != 0 && cap < g) g = cap;
    if (g == 0 && blocks > 0) g = 1;
    return g;
}

int main() {
    const uint64_t resident = 2048;   // 8 workgroups x 256 CUs
    // cap 0 (off): today's grid, above, at and below the resident count
    CHECK(query_grid(16384, resident, 0) == 2048, "cap 0, blocks above resident: %u", query_grid(16384, resident, 0));
    CHECK(query_grid(2049, resident, 0) == 2048, "cap 0, blocks one above resident");
    CHECK(query_grid(2048, resident, 0) == 2048, "cap 0, blocks equal to resident");
    CHECK(query_grid(2047, resident, 0) == 2047, "cap 0, blocks one below resident");
    CHECK(query_grid(9, resident, 0) == 9 && query_grid(1, resident, 0) == 1, "cap 0, few blocks");
    // cap 1: one workgroup walks every block
    CHECK(query_grid(16384, resident, 1) == 1 && query_grid(9, resident, 1) == 1 && query_grid(1, resident, 1) == 1,
          "cap 1");
    // a cap between: 3 does not divide 4 or 9 blocks
    CHECK(query_grid(4, resident, 3) == 3 && query_grid(9, resident, 3) == 3 && query_grid(2, resident, 3) == 2, "cap 3");
    // cap > blocks, cap > resident: the cap changes nothing
    CHECK(query_grid(9, resident, 100) == 9, "cap above blocks");
    CHECK(query_grid(16384, resident, 4096) == 2048, "cap above resident");
    CHECK(query_grid(16384, resident, 2048) == 2048 && query_grid(16384, resident, 2047) == 2047, "cap at resident");
    // a huge cap (rtw_set_tuning clamps to 2^20; the function takes any uint32)
    CHECK(query_grid(16384, resident, 1u << 20) == 2048 && query_grid(16384, resident, 0xFFFFFFFFu) == 2048, "huge cap");
    CHECK(query_grid(5, resident, 0xFFFFFFFFu) == 5, "huge cap, few blocks");
    // never 0 for blocks > 0, even if the occupancy query answered 0; nothing to launch for 0 blocks
    CHECK(query_grid(7, 0, 0) == 1 && query_grid(7, 0, 5) == 1 && query_grid(1, 0, 1) == 1, "resident 0");
    CHECK(query_grid(0, resident, 0) == 0 && query_grid(0, resident, 3) == 0, "no blocks");
    // 2^40 rays are 2^32 blocks; a resident count beyond a uint32 saturates, it does not wrap
    CHECK(query_grid((uint64_t)1 << 32, resident, 0) == 2048, "2^32 blocks");
    CHECK(query_grid((uint64_t)1 << 33, (uint64_t)1 << 33, 0) == 0xFFFFFFFFu, "beyond a uint32: %u",
          query_grid((uint64_t)1 << 33, (uint64_t)1 << 33, 0));
    CHECK(query_grid((uint64_t)1 << 33, (uint64_t)1 << 33, 7) == 7, "beyond a uint32, capped");
    // sweep against the restatement
    const uint64_t bs[] = {0, 1, 2, 3, 4, 9, 12, 255, 256, 2047, 2048, 2049, 4096, 1u << 20, (uint64_t)1 << 32};
    const uint64_t rs[] = {0, 1, 2, 8, 256, 2047, 2048, 2049, 1u << 20};
    const uint32_t cs[] = {0, 1, 2, 3, 8, 2047, 2048, 2049, 1u << 20, 0xFFFFFFFFu};
    int n = 0;
    for (uint64_t b : bs)
        for (uint64_t r : rs)
            for (uint32_t c : cs) {
                const uint32_t g = query_grid(b, r, c);
                CHECK(g == restated(b, r, c), "sweep %llu %llu %u: %u", (unsigned long long)b, (unsigned long long)r, c, g);
                CHECK((b == 0) == (g == 0) && g <= b && (c == 0 || g <= c), "sweep bounds %llu %llu %u",
                      (unsigned long long)b, (unsigned long long)r, c);
                ++n;
            }
    printf("%d combinations\n%d wrong\n", n, g_wrong);
    return g_wrong ? 1 : 0;
}
