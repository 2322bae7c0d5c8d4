// lpt_state_check.cpp -- CPU check of the task-order state (host/lpt_state.hpp)
// and of a pass's kernel parameters (host/render_pass.hpp pass_params).  Built
// and run by tests/test_lpt_state_host.py:
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> \
//       lpt_state_check.cpp -o lpt_state_check
// The state check is a table of event sequences: each event is a render of a
// key, with the source of its tile costs as the if / else chain of lpt_prepare
// gave it before that chain became lpt_source.  `drive` does to the state what
// capi_lpt.cpp does for each source, without the device work.
#include <stdio.h>

#include <vector>

#include "host/lpt_state.hpp"
#include "host/render_pass.hpp"

static int g_wrong = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++g_wrong;                   \
            printf("WRONG: " __VA_ARGS__); \
            printf("\n");                \
        }                                \
    } while (0)

using rtw::LptKey;
using rtw::LptSource;
using rtw::LptState;

static const char* kNames[] = {"split costs", "count inline", "pilot", "read back", "cached"};

struct Render {
    LptKey key;
    LptSource want;
    bool split_has_costs = false;
    bool lpt_inline = true;
    bool launch_ok = true;      // a counting render: lpt_counted is reached
    bool readback_ok = true;
};

static LptKey key_of(uint32_t spp = 32) {
    LptKey k{};
    k.cam.image_width = 40;
    k.cam.image_height = 24;
    k.cam.samples_per_pixel = spp;
    k.cam.max_depth = 50;
    k.scene_serial = 3;
    k.rank = 1;
    k.nranks = 4;
    k.prec = 8;
    k.split = 0;
    return k;
}

static void drive(LptState& s, const Render& e) {
    switch (rtw::lpt_source(s, e.key, e.split_has_costs, e.lpt_inline)) {
    case rtw::kSplitCosts: s.adopt(e.key); break;
    case rtw::kCountInline:
        s.invalidate();
        if (e.launch_ok) s.counted(e.key);
        break;
    case rtw::kPilot:
        s.invalidate();
        s.adopt(e.key);
        break;
    case rtw::kReadBack: s.read_back(e.readback_ok); break;
    case rtw::kCached: break;
    }
}

static void run(const char* name, const std::vector<Render>& seq) {
    LptState s;
    for (size_t k = 0; k < seq.size(); ++k) {
        const LptSource got = rtw::lpt_source(s, seq[k].key, seq[k].split_has_costs, seq[k].lpt_inline);
        CHECK(got == seq[k].want, "%s: render %zu takes its costs from '%s', expected '%s'", name, k, kNames[got],
              kNames[seq[k].want]);
        drive(s, seq[k]);
        // with costs on the host the task list can be built; a counting render has none yet
        CHECK(s.valid == (got != rtw::kCountInline && !(got == rtw::kReadBack && !seq[k].readback_ok)),
              "%s: render %zu leaves valid = %d", name, k, (int)s.valid);
    }
}

static void check_state() {
    const LptKey K = key_of();
    // a cold context with inline counting
    run("cold", {{K, rtw::kCountInline}, {K, rtw::kReadBack}, {K, rtw::kCached}, {K, rtw::kCached}});
    // each key field on its own: a recount, whether the old costs were pending or on the host
    LptKey changed[6] = {K, K, K, K, K, K};
    changed[0].cam.center[1] += 1.0;   // (any byte of the camera)
    changed[1].scene_serial = 4;
    changed[2].rank = 2;
    changed[3].nranks = 5;
    changed[4].prec = 4;
    changed[5].split = 1;
    const char* field[6] = {"camera", "scene serial", "rank", "nranks", "precision", "split id"};
    for (int f = 0; f < 6; ++f) {
        CHECK(!(changed[f] == K), "%s: the keys compare equal", field[f]);
        run(field[f], {{K, rtw::kCountInline}, {K, rtw::kReadBack}, {changed[f], rtw::kCountInline},
                       {changed[f], rtw::kReadBack}, {changed[f], rtw::kCached}, {K, rtw::kCountInline}});
        run(field[f], {{K, rtw::kCountInline}, {changed[f], rtw::kCountInline}, {changed[f], rtw::kReadBack}});
    }
    // lpt_inline 0: a pilot render, then its costs
    run("pilot", {{K, rtw::kPilot, false, false}, {K, rtw::kCached, false, false}, {changed[0], rtw::kPilot, false, false}});
    // a split dealt by costs and a new key: the split's costs, no counting -- also when only
    // the camera is new (current behaviour, see ADVICE.md: stale costs after a camera change)
    run("split costs", {{K, rtw::kCountInline}, {K, rtw::kReadBack}, {changed[5], rtw::kSplitCosts, true},
                        {changed[5], rtw::kCached, true}, {changed[0], rtw::kSplitCosts, true}});
    run("split costs, no pilot", {{K, rtw::kSplitCosts, true, false}, {K, rtw::kCached, true, false}});
    // a counting render whose launch failed leaves nothing pending: the next one counts again
    run("failed launch", {{K, rtw::kCountInline, false, true, false}, {K, rtw::kCountInline}, {K, rtw::kReadBack}});
    {
        LptState s;
        drive(s, {K, rtw::kCountInline, false, true, false});
        CHECK(!s.pending && !s.valid && !s.has(K), "failed launch: pending %d valid %d", (int)s.pending, (int)s.valid);
    }
    // a failed read-back: the next render recounts
    run("failed read-back", {{K, rtw::kCountInline}, {K, rtw::kReadBack, false, true, true, false},
                             {K, rtw::kCountInline}, {K, rtw::kReadBack}, {K, rtw::kCached}});
    // has(): pending or valid costs of that very key
    {
        LptState s;
        CHECK(!s.has(K), "a new state has costs");
        s.counted(K);
        CHECK(s.has(K) && !s.has(changed[2]), "pending costs: has()");
        s.read_back(true);
        CHECK(s.has(K) && s.valid && !s.pending, "read back: has()");
        s.invalidate();
        CHECK(!s.has(K), "invalidated: has()");
    }
    // the task list: stale until built, then for another n_chunks, group or target, and after new costs
    {
        LptState s;
        s.adopt(K);
        CHECK(s.table_stale(8, 0, 1u << 17), "no table yet");
        s.table_built(8, 0, 1u << 17);
        CHECK(!s.table_stale(8, 0, 1u << 17), "the table just built is stale");
        CHECK(s.table_stale(4, 0, 1u << 17), "n_chunks 4 against a table of 8");
        CHECK(s.table_stale(8, 2, 1u << 17), "group 2 against a table of group 0");
        CHECK(s.table_stale(8, 0, 1000), "target 1000 against a table of 2^17");
        CHECK(!s.table_stale(8, 0, 1u << 17), "the checks changed the table");
        CHECK(rtw::lpt_source(s, K, false, true) == rtw::kCached && !s.table_stale(8, 0, 1u << 17), "a cached render");
        s.adopt(changed[0]);
        CHECK(s.table_stale(8, 0, 1u << 17), "new costs keep the old table");
        s.table_built(8, 0, 1u << 17);
        s.invalidate();
        CHECK(s.table_stale(8, 0, 1u << 17), "invalidate keeps the table");
    }
}

// The windows of one render share the render's key (its camera keeps its sample
// count); the windows of rtw_render_window_device share the key without one.
static void check_keys() {
    rtw_camera cam = key_of(12).cam;
    const rtw::Pass whole = rtw::one_shot_pass(cam);
    LptKey k_whole = key_of(12), k[3], d[2];
    k_whole.cam = rtw::key_camera(cam, whole);
    for (uint32_t w = 0; w < 3; ++w) {
        k[w] = key_of(12);
        k[w].cam = rtw::key_camera(cam, rtw::window_pass(4 * w, 4, 1, nullptr, w == 0, cam.samples_per_pixel));
        CHECK(k[w] == k_whole && k[w].cam.samples_per_pixel == 12, "window %u of a render: another key", w);
    }
    run("windows of a render", {{k[0], rtw::kCountInline}, {k[1], rtw::kReadBack}, {k[2], rtw::kCached},
                                {k_whole, rtw::kCached}});
    const uint32_t first[2] = {0, 4}, n[2] = {4, 6};
    for (int w = 0; w < 2; ++w) {
        d[w] = key_of(12);
        d[w].cam = rtw::key_camera(cam, rtw::window_pass(first[w], n[w], 1, nullptr, true, 0));
        CHECK(d[w].cam.samples_per_pixel == 0, "window render: the key's camera has %u samples",
              d[w].cam.samples_per_pixel);
    }
    CHECK(d[0] == d[1] && !(d[0] == k_whole), "window renders of 4 and 6 samples: keys");
    run("window renders", {{d[0], rtw::kCountInline}, {d[1], rtw::kReadBack}, {k_whole, rtw::kCountInline}});
}

template <typename R>
static void check_params(const char* pr) {
    rtw::DevScene<R> sc{};
    sc.n_sph = 7;
    rtw_camera cam = key_of(12).cam;
    cam.center[0] = 1.5;
    cam.pixel_delta_u[2] = -0.25;
    cam.background[1] = 0.5;
    cam.defocus_angle = 0.6;
    rtw::RenderKnobs knobs;
    rtw::RenderPlan pl;
    pl.chunk = 1;
    pl.n_chunks = 12;
    pl.group = 4;
    pl.n_groups = 3;
    pl.stack = 24;
    pl.robust = 1;
    pl.hit64 = 1;
    const uint32_t nt = rtw::tiles_for_rank(40, 24, 1, 4);   // 15 tiles: ranks 0-2 have 4, rank 3 has 3
    pl.n_tasks = nt * pl.n_groups;
    // one-shot: every sample of the camera, from sample 0
    {
        const rtw::KParams<R> p = rtw::pass_params<R>(sc, cam, 99, 1, 4, knobs, pl, rtw::one_shot_pass(cam));
        CHECK(p.s_base == 0 && p.c_base == 0 && p.spp == 12, "%s one-shot: s_base %u c_base %u spp %u", pr, p.s_base,
              p.c_base, p.spp);
        CHECK(nt == 4 && p.n_local_tiles == nt && p.tiles_x == 5 && p.rank == 1 && p.nranks == 4 && !p.tile_map,
              "%s one-shot: tiles %u (%u across) rank %u / %u", pr, p.n_local_tiles, p.tiles_x, p.rank, p.nranks);
        CHECK(p.seed == 99 && p.W == 40 && p.H == 24 && p.max_depth == 50 && p.defocus == 1, "%s one-shot: camera", pr);
        CHECK(p.center[0] == (R)1.5 && p.du[2] == (R)-0.25 && p.bg[1] == (R)0.5, "%s one-shot: camera vectors", pr);
        CHECK(p.u_scale >= (R)1 && p.u_scale * (R)(1.0 - 2.220446049250313080847e-16) - (R)0.5 <= (R)0.5,
              "%s one-shot: u_scale %.17g", pr, (double)p.u_scale);
        CHECK(p.chunk == 1 && p.n_chunks == 12 && p.group == 4 && p.n_groups == 3 && p.n_tasks == 12 &&
                  p.stack == 24 && p.sc.robust == 1 && p.hit64 == 1 && p.sc.n_sph == 7,
              "%s one-shot: the plan's values", pr);
        CHECK(p.item_order == knobs.item_order && p.persist == knobs.persist, "%s one-shot: knobs", pr);
        CHECK(!p.partial && !p.counters && !p.task_table && !p.tile_cost && !p.cost_spp && !p.cost_time,
              "%s one-shot: buffers and task order are the caller's", pr);
        const rtw::KParams<R> v = rtw::render_kernel_view(p);
        CHECK(v.spp == 12 && v.partial == p.partial, "%s one-shot: the kernel's view", pr);
    }
    // a window: first 8, n 4, chunk 2
    {
        rtw::RenderPlan pw = pl;
        pw.chunk = 2;
        pw.n_chunks = 2;
        std::vector<R> buf(64);
        rtw::KParams<R> p = rtw::pass_params<R>(sc, cam, 99, 1, 4, knobs, pw, rtw::window_pass(8, 4, 2, nullptr, false, 12));
        CHECK(p.s_base == 8 && p.c_base == 4 && p.spp == 4 && p.chunk == 2 && p.n_chunks == 2,
              "%s window: s_base %u c_base %u spp %u", pr, p.s_base, p.c_base, p.spp);
        p.partial = buf.data() + 32;
        p.cost_spp = 2;
        const rtw::KParams<R> v = rtw::render_kernel_view(p);
        CHECK(v.spp == 12 && v.cost_spp == 10 && v.partial == buf.data() + 32 - 4 * 3,
              "%s window: the kernel's view has spp %u, partial moved by %td", pr, v.spp, v.partial - p.partial);
        CHECK(rtw::kPassKinds[rtw::kPassWindow].fold == rtw::kFoldWindow && rtw::kPassKinds[rtw::kPassWindow].fixed_chunk,
              "%s window: its row", pr);
    }
    // an adaptive sub-pass: the listed tiles, one sample per item
    {
        rtw::RenderPlan pa = pl;
        pa.n_chunks = 3;
        const uint32_t list[3] = {2, 5, 11};
        const rtw::Pass ps = rtw::adaptive_pass(4, 3, list, 3);
        const rtw::KParams<R> p = rtw::pass_params<R>(sc, cam, 99, 0, 1, knobs, pa, ps);
        CHECK(p.tile_map == list && p.n_local_tiles == 3 && ps.chunk == 1 && p.chunk == 1,
              "%s adaptive: %u tiles, chunk %u", pr, p.n_local_tiles, p.chunk);
        CHECK(p.s_base == 4 && p.c_base == 4 && p.spp == 3 && !ps.begin, "%s adaptive: s_base %u c_base %u spp %u", pr,
              p.s_base, p.c_base, p.spp);
        const rtw::PassKindRow& row = rtw::kPassKinds[rtw::kPassAdaptive];
        CHECK(row.fold == rtw::kFoldNone && !row.lpt && !row.split && row.fixed_chunk, "%s adaptive: its row", pr);
        CHECK(rtw::adaptive_pass(0, 4, nullptr, 15).begin, "%s adaptive: the first sub-pass begins the render", pr);
    }
}

int main() {
    check_state();
    check_keys();
    check_params<float>("f32");
    check_params<double>("f64");
    printf("%d wrong\n", g_wrong);
    return g_wrong ? 1 : 0;
}
