"""Adaptive and windowed renders over multi-device contexts:
rtw_render_adaptive_image, rtw_render_adaptive_image_device and
rtw_render_window_image, on the n-rank path of one GPU (rtw_create_virtual).

Every (pixel, sample) has its own RNG stream and a tile's state never leaves
the rank that owns it, so the n-rank result is the one-device result bit for
bit -- sums, counts and NaN mask, in both precisions, for any rank count and
any valid split.  "Identical" is tests/test_gpu_windows.py's: equal NaN masks,
equal values elsewhere."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

import adaptive_rule as A
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = _capi.RTW_E_INVALID, _capi.RTW_E_UNSUPPORTED
MIN, WIN, MAX, TOL = 4, 4, 32, 0.125
PRECS = [rtw.RTW_F64, rtw.RTW_F32]


def _identical(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _renderer(soa, prec, tuning=None, chunk=0, **kw):
    r = rtw.Renderer(device=0, precision=prec, **kw)
    if chunk:
        r.set_chunk(chunk)
    for k, v in (tuning or {}).items():
        r.set_tuning(k, v)
    r.set_scene(soa)
    return r


def _cam(w, h, depth, spp=1):
    soa, b = rtw.scenes.simple_soa(A.SEED_SCENE, A.GRID)
    return soa, b.copy().with_image_width(w).with_image_height(h).with_samples_per_pixel(spp) \
        .with_max_depth(depth).build()


def _stats(st):
    return st.samples, st.segments, st.lambertian


@functools.lru_cache(maxsize=None)
def _one_device(w, h, depth, prec, partial_max=0):
    """(sums, counts, (samples, segments, lambertian)) of Renderer.render_adaptive
    on a one-device context.  Computed once per case, read-only."""
    soa, cam = _cam(w, h, depth)
    with _renderer(soa, prec, {"partial_max": partial_max} if partial_max else None) as r:
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
        st = _stats(r.stats)
    sums.setflags(write=False)
    counts.setflags(write=False)
    return sums, counts, st


def _shared(prec):
    return _one_device(A.W, A.H, A.DEPTH, prec)


def _active_per_rank(counts, n):
    """For each pass end, the tiles of each rank (round robin) that render that pass."""
    tc = np.array(A.tile_counts(counts))
    ends = A.pass_ends(MIN, MAX, WIN)
    return [[int((tc[k::n] >= e).sum()) for k in range(n)] for e in ends]


def test_preconditions_of_the_shared_case():
    """Asserted on the one-device result, so that the n-rank tests cannot pass
    trivially: the tile counts take at least 3 values, min and max among them,
    and under the round robin over 8 ranks some rank has no active tile in a
    pass in which another still has one."""
    _, counts, _ = _shared(rtw.RTW_F64)
    hist = sorted(collections.Counter(A.tile_counts(counts)).items())
    print("one-device f64 tile counts:", hist)
    values = {c for c, _ in hist}
    assert len(values) >= 3 and MIN in values and MAX in values
    per_pass = _active_per_rank(counts, 8)
    print("active tiles per rank (n = 8), per pass:", per_pass)
    assert any(min(p) == 0 and max(p) > 0 for p in per_pass)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [2, 3, 8])
def test_adaptive_n_ranks_identical_to_one_device(n, prec):
    soa, cam = A.simple_scene()
    ref_sums, ref_counts, ref_st = _shared(prec)
    with _renderer(soa, prec, virtual_ranks=n) as r:
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
        got = _stats(r.stats)
        assert r.stats.chunk == 1 and r.stats.kernel_ms > 0
        per_rank = [_stats(r.rank_view(k).get_stats()) for k in range(n)]
        again = _stats(r.get_stats())
    assert np.array_equal(counts, ref_counts)
    assert _identical(sums, ref_sums)
    assert got[0] == int(counts.astype(np.uint64).sum())
    assert got == ref_st and again == ref_st
    assert tuple(sum(p[i] for p in per_rank) for i in range(3)) == ref_st
    # each rank's samples are its own tiles' (the round robin)
    tc, px = np.array(A.tile_counts(counts), np.uint64), _tile_pixels(A.W, A.H)
    assert [p[0] for p in per_rank] == [int((tc[k::n] * px[k::n]).sum()) for k in range(n)]


def _tile_pixels(w, h):
    return np.array([min(8, w - tx) * min(8, h - ty) for ty in range(0, h, 8) for tx in range(0, w, 8)], np.uint64)


def test_f64_three_ranks_against_the_oracle():
    soa, cam = A.simple_scene()
    want_sums, want_counts = A.adaptive(A.oracle_samples(), MIN, MAX, WIN, TOL)
    with _renderer(soa, rtw.RTW_F64, virtual_ranks=3) as r:
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
    assert np.array_equal(counts, want_counts)
    assert _identical(sums, want_sums)


def test_ragged_tiles_eight_ranks():
    """120 x 72 at depth 50: 15 x 9 tiles, 135 = 16 * 8 + 7, so the ranks own 17
    or 16 tiles and the last slots of the gather target stay unused."""
    soa, cam = _cam(120, 72, 50)
    ref_sums, ref_counts, ref_st = _one_device(120, 72, 50, rtw.RTW_F64)
    hist = sorted(collections.Counter(A.tile_counts(ref_counts)).items())
    print("120 x 72 one-device tile counts:", hist)
    assert len(hist) >= 3
    with _renderer(soa, rtw.RTW_F64, virtual_ranks=8) as r:
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
        assert _stats(r.stats) == ref_st
    assert np.array_equal(counts, ref_counts) and _identical(sums, ref_sums)


def test_dealt_split_is_followed_and_left_alone():
    soa, cam = A.simple_scene()
    ref_sums, ref_counts, ref_st = _shared(rtw.RTW_F64)
    nt = rtw.n_tiles(A.W, A.H)
    costs = np.array([1 + 50 * (t % 4 == 0) + 7 * (t % 5) for t in range(nt)], np.uint32)
    split = rtw.split_deal(costs, A.W, A.H, 3)
    assert not np.array_equal(split, np.arange(nt) % 3)           # not the round robin
    with _renderer(soa, rtw.RTW_F64, virtual_ranks=3) as r:
        r.set_split(A.W, A.H, 3, split)
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
        assert _stats(r.stats) == ref_st
        kind, got = r.get_split(A.W, A.H, 3)
        assert kind == 1 and np.array_equal(got, split)           # neither dealt anew nor cleared
        # each rank rendered the tiles the split gives it
        tc, px = np.array(A.tile_counts(counts), np.uint64), _tile_pixels(A.W, A.H)
        assert [r.rank_view(k).get_stats().samples for k in range(3)] == \
            [int((tc * px)[split == k].sum()) for k in range(3)]
        assert np.array_equal(counts, ref_counts) and _identical(sums, ref_sums)
        r.set_split(A.W, A.H, 3, None)
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
        assert r.get_split(A.W, A.H, 3)[0] == 0
    assert np.array_equal(counts, ref_counts) and _identical(sums, ref_sums)


def test_stale_state_after_a_larger_image():
    """The state buffer is carved anew for the smaller image: the words that
    become the flags of the tiles a rank does not own held the larger image's
    sums."""
    soa, big = _cam(120, 72, 50)
    _, small = A.simple_scene()
    big_sums, big_counts, _ = _one_device(120, 72, 50, rtw.RTW_F64)
    ref_sums, ref_counts, ref_st = _shared(rtw.RTW_F64)
    with _renderer(soa, rtw.RTW_F64, virtual_ranks=3) as r:
        sums, counts = r.render_adaptive(big, A.SEED, MIN, MAX, WIN, TOL)
        assert np.array_equal(counts, big_counts) and _identical(sums, big_sums)
        sums, counts = r.render_adaptive(small, A.SEED, MIN, MAX, WIN, TOL)
        assert _stats(r.stats) == ref_st
    assert np.array_equal(counts, ref_counts) and _identical(sums, ref_sums)


def test_a_rank_without_tiles():
    """16 x 8: 2 tiles over 3 ranks.  Rank 2 takes no part and its stats are
    those of no work -- not an error 'before the first render'."""
    soa, cam = _cam(16, 8, A.DEPTH)
    ref_sums, ref_counts, ref_st = _one_device(16, 8, A.DEPTH, rtw.RTW_F64)
    with _renderer(soa, rtw.RTW_F64, virtual_ranks=3) as r:
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
        assert _stats(r.stats) == ref_st
        per_rank = [_stats(r.rank_view(k).get_stats()) for k in range(3)]
        assert per_rank[2] == (0, 0, 0) and per_rank[0][0] > 0 and per_rank[1][0] > 0
        assert tuple(sum(p[i] for p in per_rank) for i in range(3)) == ref_st
        img = r.render(cam, A.SEED)                               # and the context renders on
        assert np.isfinite(img).any() and r.stats.samples == 16 * 8
    assert np.array_equal(counts, ref_counts) and _identical(sums, ref_sums)


def test_sub_passes():
    """partial_max at its 1 MiB floor: a rank's 45 tiles of 120 x 72 take 69120
    bytes a sample in f64, so 15 samples fit and a window of 16 is cut in two."""
    soa, cam = _cam(120, 72, 4)
    with _renderer(soa, rtw.RTW_F64) as r:
        ref_sums, ref_counts = r.render_adaptive(cam, 3, 17, 49, 16, TOL)
        ref_st = _stats(r.stats)
    assert len(np.unique(ref_counts)) >= 2
    assert (1 << 20) // (45 * 64 * 3 * 8) < 16
    with _renderer(soa, rtw.RTW_F64, {"partial_max": 1 << 20}, virtual_ranks=3) as r:
        sums, counts = r.render_adaptive(cam, 3, 17, 49, 16, TOL)
        assert _stats(r.stats) == ref_st
    assert np.array_equal(counts, ref_counts) and _identical(sums, ref_sums)


def test_device_form_on_the_callers_stream():
    import torch
    soa, cam = A.simple_scene()
    ref_sums, ref_counts, ref_st = _shared(rtw.RTW_F64)
    n = A.W * A.H
    lib = rtw._lib
    with _renderer(soa, rtw.RTW_F64, virtual_ranks=3) as r:
        host_sums, host_counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
        stream = torch.cuda.Stream(device=0)
        with torch.cuda.stream(stream):
            d_sums = torch.full((A.H, A.W, 3), -5.0, dtype=torch.float64, device="cuda:0")
            d_counts = torch.full((A.H, A.W), 77, dtype=torch.int32, device="cuda:0")
            r.render_adaptive_device(cam, A.SEED, MIN, MAX, WIN, TOL, d_sums.data_ptr(), n * 24,
                                     d_counts.data_ptr(), n * 4)
            got_sums, got_counts = d_sums.cpu().numpy(), d_counts.cpu().numpy().astype(np.uint32)   # stream order
        assert _stats(r.get_stats()) == ref_st

        def dev(s=d_sums.data_ptr(), sb=n * 24, c=d_counts.data_ptr(), cb=n * 4):
            return lib.rtw_render_adaptive_image_device(r.ctx, C.byref(cam.raw), C.c_uint64(A.SEED), MIN, MAX, WIN, TOL,
                                                        C.c_void_p(s) if s else None, sb,
                                                        C.c_void_p(c) if c else None, cb, None)
        d_sums.fill_(2.5)
        d_counts.fill_(9)
        torch.cuda.synchronize()
        assert dev(sb=n * 24 - 8) == E_INVALID and dev(cb=n * 4 - 4) == E_INVALID
        assert dev(s=None) == E_INVALID and dev(c=None) == E_INVALID
        torch.cuda.synchronize()
        assert bool((d_sums == 2.5).all()) and bool((d_counts == 9).all())
    assert np.array_equal(host_counts, ref_counts) and _identical(host_sums, ref_sums)
    assert np.array_equal(got_counts, host_counts) and _identical(got_sums, host_sums)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [2, 3])
def test_windows_n_ranks(n, prec):
    """40 x 24 at depth 50: [0, 4) then [4, 10), the host array carried between
    the calls, against the one-device one-shot render of 10 spp at chunk 1; an
    f32 context returns the f64 running sums (the one-shot image is those
    rounded to f32 once, tests/test_gpu_windows.py _as_rendered)."""
    soa, cam = _cam(40, 24, 50, spp=10)
    with _renderer(soa, prec, chunk=1) as r:
        ref = r.render(cam, 21)
        assert r.stats.chunk == 1
        one = r.render_window(cam, 21, 0, 4)
        one = r.render_window(cam, 21, 4, 6, one)
        ref_st = _stats(r.stats)                                   # of the window [4, 10)
    with _renderer(soa, prec, chunk=1, virtual_ranks=n) as r:
        sums = r.render_window(cam, 21, 0, 4)
        assert r.stats.samples == 40 * 24 * 4
        sums = r.render_window(cam, 21, 4, 6, sums)
        assert _stats(r.stats) == ref_st and ref_st[0] == 40 * 24 * 6
        assert sum(r.rank_view(k).get_stats().samples for k in range(n)) == 40 * 24 * 6
    assert sums.dtype == np.float64 and _identical(sums, one)
    assert _identical(sums if prec == rtw.RTW_F64 else sums.astype(np.float32).astype(np.float64), ref)
    if prec == rtw.RTW_F32:
        assert not _identical(sums, ref)                           # the running sums were not rounded to f32


def test_window_argument_checks():
    soa, cam = _cam(40, 24, 50)
    with _renderer(soa, rtw.RTW_F64, chunk=2, virtual_ranks=2) as r:
        sums = r.render_window(cam, 21, 0, 4)
        before = sums.copy()
        with pytest.raises(rtw.RenderError) as e:
            r.render_window(cam, 21, 3, 2, sums)                   # not a multiple of the explicit chunk
        assert e.value.code == E_INVALID and _identical(sums, before)
        st = _stats(r.get_stats())
        assert r.render_window(cam, 21, 4, 0, sums) is sums       # no samples: nothing happens
        assert _identical(sums, before) and _stats(r.get_stats()) == st
        lib, p = rtw._lib, sums.ctypes.data_as(_capi._f64p)
        assert lib.rtw_render_window_image(r.ctx, C.byref(cam.raw), C.c_uint64(1), 0xFFFFFFFF, 1, p, None) == E_INVALID
        assert lib.rtw_render_window_image(r.ctx, C.byref(cam.raw), C.c_uint64(1), 0, 2, None, None) == E_INVALID
        assert lib.rtw_render_window_image(r.ctx, None, C.c_uint64(1), 0, 2, p, None) == E_INVALID
        assert _identical(sums, before)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        assert lib.rtw_render_window_image(r.ctx, C.byref(cam.raw), C.c_uint64(1), 0, 2, p, None) \
            == _capi.RTW_E_NO_SCENE


@pytest.mark.parametrize("prec", PRECS)
def test_a_list_of_one_gpu(prec):
    """Renderer(devices=[0]) is a multi-device context of one rank: the RCCL
    branch of the gather (a clique of one, rank 0 in place) with the byte-typed
    records and the f64 accumulators."""
    soa, cam = A.simple_scene()
    ref_sums, ref_counts, ref_st = _shared(prec)
    with _renderer(soa, prec) as r:
        ref_win = r.render_window(cam, A.SEED, 0, 3)
        ref_win = r.render_window(cam, A.SEED, 3, 2, ref_win)
    with _renderer(soa, prec, devices=[0]) as r:
        assert r.n_devices == 1
        sums, counts = r.render_adaptive(cam, A.SEED, MIN, MAX, WIN, TOL)
        assert _stats(r.stats) == ref_st
        win = r.render_window(cam, A.SEED, 0, 3)
        win = r.render_window(cam, A.SEED, 3, 2, win)
        assert r.stats.samples == A.W * A.H * 2
    assert np.array_equal(counts, ref_counts) and _identical(sums, ref_sums)
    assert _identical(win, ref_win)


def test_one_device_delegates_and_the_old_forms_still_refuse():
    import torch
    soa, cam = A.simple_scene()
    ref_sums, ref_counts, ref_st = _shared(rtw.RTW_F64)
    lib, n = rtw._lib, A.W * A.H
    sums, counts, st = np.zeros((A.H, A.W, 3)), np.zeros((A.H, A.W), np.uint32), _capi.rtw_stats()
    sp, cp = sums.ctypes.data_as(_capi._f64p), counts.ctypes.data_as(_capi._u32p)
    d_sums = torch.full((A.H, A.W, 3), -5.0, dtype=torch.float64, device="cuda:0")
    d_counts = torch.full((A.H, A.W), 77, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with _renderer(soa, rtw.RTW_F64) as r:
        assert r.n_devices == 1
        assert lib.rtw_render_adaptive_image(r.ctx, C.byref(cam.raw), C.c_uint64(A.SEED), MIN, MAX, WIN, TOL, sp, cp,
                                             C.byref(st)) == 0
        assert _stats(st) == ref_st
        assert np.array_equal(counts, ref_counts) and _identical(sums, ref_sums)
        assert lib.rtw_render_adaptive_image_device(r.ctx, C.byref(cam.raw), C.c_uint64(A.SEED), MIN, MAX, WIN, TOL,
                                                    C.c_void_p(d_sums.data_ptr()), n * 24,
                                                    C.c_void_p(d_counts.data_ptr()), n * 4, None) == 0
        assert _stats(r.get_stats()) == ref_st
        torch.cuda.synchronize()
        assert np.array_equal(d_counts.cpu().numpy().astype(np.uint32), ref_counts)
        assert _identical(d_sums.cpu().numpy(), ref_sums)
        assert lib.rtw_render_adaptive_image(r.ctx, C.byref(cam.raw), C.c_uint64(A.SEED), 1, MAX, WIN, TOL, sp, cp,
                                             None) == E_INVALID
        old = r.render_window(cam, A.SEED, 0, 3)
        new = np.zeros((A.H, A.W, 3))
        assert lib.rtw_render_window_image(r.ctx, C.byref(cam.raw), C.c_uint64(A.SEED), 0, 3,
                                           new.ctypes.data_as(_capi._f64p), C.byref(st)) == 0
        assert _identical(new, old) and st.samples == n * 3
    # the one-device entry points keep refusing a multi-device context
    with _renderer(soa, rtw.RTW_F64, virtual_ranks=2) as r:
        before = sums.copy()
        assert lib.rtw_render_adaptive(r.ctx, C.byref(cam.raw), C.c_uint64(A.SEED), MIN, MAX, WIN, TOL, sp, cp,
                                       None) == E_UNSUPPORTED
        assert lib.rtw_render_adaptive_device(r.ctx, C.byref(cam.raw), C.c_uint64(A.SEED), MIN, MAX, WIN, TOL,
                                              C.c_void_p(d_sums.data_ptr()), n * 24,
                                              C.c_void_p(d_counts.data_ptr()), n * 4, None) == E_UNSUPPORTED
        assert lib.rtw_render_window(r.ctx, C.byref(cam.raw), C.c_uint64(A.SEED), 0, 2, sp, None) == E_UNSUPPORTED
        assert lib.rtw_render_window_device(r.ctx, C.byref(cam.raw), C.c_uint64(A.SEED), 0, 1, 0, 2,
                                            C.c_void_p(d_sums.data_ptr()), n * 24, None) == E_UNSUPPORTED
        assert _identical(sums, before)
