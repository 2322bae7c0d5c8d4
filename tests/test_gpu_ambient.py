"""Ambient occlusion as one query (rtw_ambient_occlusion) on the GPU.

f64: the directions, the occluded bytes and the open counts bit for bit against
the case file (tests/ambient_cases.py: the independent restatement's Rng,
cosine_hemisphere and Onb, and nee_cases.any_hit with every gate on), and
against the context's own occluded() on the recorded directions; every world
gives the same bits; calls compose over first_stream and over sample windows;
blocks past a workgroup's first and segments of 1, 3 and 70 lanes; the
zero-normal rule, a NaN normal, empty ranges; a closed form; the refusals; the
torch device entry; render_ao.

f32: the identities bit for bit (the occluded record is the f32 context's own
occluded() on the recorded d, open is the integer sum of the record); the
directions against f32_forms.cone_or_cosine under the rule test_gpu_f32_records.py
applies to its "cosine lobe" rows -- over the pooled rows the kernel's p50, p99
and max row error (inf-norm, relative to the law's) are each at most 4 x the
calibration's (the same form in float32), the law being the form in float64 on
the f32 inputs; only rows within rounding of Onb's |w.x| > 0.9 decision may be
left out, at most 1 %; and against the f64 case file the occluded bytes differ
on at most 1 % of a case's pairs (the case file's t_min note)."""
import ctypes as C

import numpy as np
import pytest

import ambient_cases as A
import f32_forms as FF
import query_cases as Q
import ray_tracing_weekend_amd as rtw
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

AMBIENT = 9                                   # rtw_query_stats.is_light_pdf
WORLD_OF_KIND = {0: 2, 1: 3, 2: 4, 3: 5}      # rtw_query_stats.kernel of tuning bvh_kind
WORLDS = [("brute, lds 1", rtw.RTW_ACCEL_BRUTE, {"lds": 1}, 1), ("brute, lds 0", rtw.RTW_ACCEL_BRUTE, {"lds": 0}, 0)] + \
         [(f"bvh_kind {k}", rtw.RTW_ACCEL_BVH, {"bvh_kind": k}, WORLD_OF_KIND[k]) for k in range(4)]
ALLOW, CAP = 4.0, 0.01                        # test_gpu_f32_records.py's allowance and cap
T = A.T_MIN


def same(a, b):
    """bit for bit up to the sign of zero, NaN masks equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def rows_off(a, b):
    a, b = np.asarray(a), np.asarray(b)
    ok = (a == b) | (np.isnan(a) & np.isnan(b))
    return np.flatnonzero(~ok.reshape(len(a), -1).all(1))[:8]


def context(soa, precision=rtw.RTW_F64, accel=None, **tuning):
    r = rtw.Renderer(device=0, precision=precision)
    if accel is not None:
        r.set_accel(accel)
    for k, v in tuning.items():
        r.set_tuning(k, v)
    r.set_scene(soa)
    return r


def equal(got, exp):
    open_, dirs, occ = got
    assert same(dirs, exp.directions), ("d", rows_off(dirs, exp.directions))
    assert np.array_equal(occ, exp.occluded), ("occluded", np.flatnonzero(occ != exp.occluded)[:8])
    assert open_.dtype == np.uint32 and np.array_equal(open_, exp.open), ("open", np.flatnonzero(open_ != exp.open)[:8])


def identities(r, pts, S, t_min, t_max, got, open0=None):
    """the record against the context's own any hit: occluded == r.occluded({p, d}, t_max) on the
    recorded directions of the live rows, open == open0 + the integer count of the record's zeros"""
    open_, dirs, occ = got
    pts = np.asarray(pts, dirs.dtype)
    n = len(pts)
    live = np.repeat((pts[:, 3:6] != 0).any(1), S)
    rays = np.ascontiguousarray(np.concatenate([np.repeat(pts[:, :3], S, 0), dirs], 1))[live]
    own = r.occluded(rays, np.full(len(rays), t_max, dirs.dtype), t_min)
    assert np.array_equal(occ[live], own), np.flatnonzero(occ[live] != own)[:8]
    assert not occ[~live].any() and not dirs[~live].any()
    base = np.zeros(n, np.uint32) if open0 is None else open0
    assert np.array_equal(open_, base + (live & (occ == 0)).reshape(n, S).sum(1, dtype=np.uint32))


# ------------------------------------------------------------------- f64
@pytest.mark.parametrize("name", list(A.CASES) + [n + "/eps" for n in A.EPS_CASES])
def test_f64_directions_bytes_and_counts_are_the_case_files(name):
    eps = name.endswith("/eps")                                     # the reference's own t_min: the default
    soa, pts, S, t_max, exp = A.eps_case(name[:-4]) if eps else A.case(name)
    t_min = None if eps else T
    with context(soa) as r:
        got = r.ambient_occlusion(pts, A.SEED, S, t_max, t_min, records=True)
        st = r.get_query_stats()
        assert st.is_light_pdf == AMBIENT and st.rays == len(pts) * S and st.hits == len(pts) * S - int(got[0].sum())
        assert got[1].dtype == np.float64 and got[2].dtype == np.uint8
        equal(got, exp)
        assert np.array_equal(r.ambient_occlusion(pts, A.SEED, S, t_max, t_min), got[0])   # without records
        identities(r, pts, S, exp.t_min, t_max, got)


@pytest.mark.parametrize("what,accel,tuning,world", WORLDS, ids=[w[0] for w in WORLDS])
def test_f64_every_world_gives_identical_bits(what, accel, tuning, world):
    # (scenes::simple runs the world asked for; lights64 and cornell_box -- one sphere -- may plan
    # another: there only the bits are compared)
    for name in ("simple", "lights64", "cornell_box"):
        soa, pts, S, t_max, exp = A.case(name)
        with context(soa, accel=accel, **tuning) as r:
            got = r.ambient_occlusion(pts, A.SEED, S, t_max, T, records=True)
            assert name != "simple" or r.get_query_stats().kernel == world
            equal(got, exp)


def test_f64_calls_compose_over_streams_and_sample_windows():
    soa, pts, S, t_max, exp = A.case("cornell_box")
    assert S == 4
    with context(soa) as r:
        a, h = 1000, 77
        whole = r.ambient_occlusion(pts, A.SEED, S, t_max, T, first_stream=a, records=True)
        d0 = r.ambient_occlusion(pts[:h], A.SEED, S, t_max, T, first_stream=a, records=True)
        d1 = r.ambient_occlusion(pts[h:], A.SEED, S, t_max, T, first_stream=a + h, records=True)
        for x, y0, y1 in zip(whole, d0, d1):
            assert same(np.concatenate([y0, y1]), x)
        assert not same(whole[1], exp.directions)                    # (another stream, another answer)
        # sample windows: (0, 2) then (2, 2) continued == S = 4
        w0 = r.ambient_occlusion(pts, A.SEED, 2, t_max, T)
        w1 = r.ambient_occlusion(pts, A.SEED, 2, t_max, T, first_sample=2, open=w0.copy())
        assert np.array_equal(w1, exp.open) and not np.array_equal(w0, exp.open)
        # a 64-bit first_stream
        big = (1 << 40) + 3
        want = A.Expected(soa, pts[:40], A.SEED, 2, t_max, T, first_stream=big, first_sample=1)
        equal(r.ambient_occlusion(pts[:40], A.SEED, 2, t_max, T, first_stream=big, first_sample=1, records=True), want)


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("S", [1, 3])
def test_f64_blocks_past_a_workgroups_first_and_segments(grid, S):
    """S = 1: 64 segments a wave; S = 3: segments straddle waves and blocks (256 = 85 * 3 + 1)"""
    soa, pts, _, t_max, _ = A.case("cornell_box")
    tiled = np.ascontiguousarray(np.tile(pts, (4, 1)))
    assert len(tiled) == 652 and (len(tiled) * S) % 64 and len(tiled) * S > 2 * 256
    want = tiled_expectation(S)
    assert not np.array_equal(want.occluded[:163 * S], want.occluded[163 * S:326 * S])   # distinct streams per tile
    for what, accel, tuning, world in (WORLDS[0], WORLDS[5]):
        with context(soa, accel=accel, query_grid=grid, **tuning) as r:
            equal(r.ambient_occlusion(tiled, A.SEED, S, t_max, T, first_stream=5, records=True), want)
            assert np.array_equal(r.ambient_occlusion(tiled, A.SEED, S, t_max, T, first_stream=5), want.open)


_TILED = {}


def tiled_expectation(S):
    if S not in _TILED:
        soa, pts, _, t_max, _ = A.case("cornell_box")
        _TILED[S] = A.Expected(soa, np.tile(pts, (4, 1)), A.SEED, S, t_max, T, first_stream=5)
    return _TILED[S]


@pytest.mark.parametrize("grid", [1, 2])
def test_f64_a_segment_longer_than_a_wave_with_a_ragged_tail(grid):
    soa, pts, _, t_max, _ = A.case("cornell_box")
    S, p = 70, pts[:10]
    assert (len(p) * S) % 256 and (len(p) * S) % 64 and len(p) * S > 2 * 256
    if "long" not in _TILED:
        _TILED["long"] = A.Expected(soa, p, A.SEED, S, t_max, T)
    want = _TILED["long"]
    assert 0 < want.open.min() and want.open.max() < S
    for what, accel, tuning, world in (WORLDS[0], WORLDS[5]):
        with context(soa, accel=accel, query_grid=grid, **tuning) as r:
            equal(r.ambient_occlusion(p, A.SEED, S, t_max, T, records=True), want)
            assert np.array_equal(r.ambient_occlusion(p, A.SEED, S, t_max, T), want.open)


def test_f64_zero_normals_nan_normals_and_empty_ranges():
    soa, pts, S, t_max, exp = A.case("cornell_box")
    p = pts[:64].copy()
    dead = [3, 17, 40]
    p[dead, 3:6] = 0.0
    p[17, 3] = -0.0                                                  # (-0 is 0)
    start = np.arange(64, dtype=np.uint32) + 7
    want = A.Expected(soa, p, A.SEED, S, t_max, T, open=start)
    live = np.setdiff1d(np.arange(64), dead)
    with context(soa) as r:
        got = r.ambient_occlusion(p, A.SEED, S, t_max, T, open=start.copy(), records=True)
        equal(got, want)
        assert np.array_equal(got[0][dead], start[dead]) and not np.array_equal(got[0], start)   # untouched
        for k in dead:
            assert not got[1][k * S:(k + 1) * S].any() and not got[2][k * S:(k + 1) * S].any()
        assert r.get_query_stats().rays == (64 - len(dead)) * S
        identities(r, p, S, T, t_max, got, start)
        # overwriting: a skipped row is 0, its neighbours' streams are unchanged
        fresh = r.ambient_occlusion(p, A.SEED, S, t_max, T, records=True)
        assert not fresh[0][dead].any() and np.array_equal(fresh[0][live], exp.open[live])
        rows = (live[:, None] * S + np.arange(S)).ravel()
        assert same(fresh[1][rows], exp.directions[rows]) and np.array_equal(fresh[2][rows], exp.occluded[rows])
        # a NaN normal is no zero normal: its directions are NaN, a NaN ray meets nothing, all open
        q = pts[:8].copy()
        q[2, 4] = np.nan
        o, d, occ = r.ambient_occlusion(q, A.SEED, S, t_max, T, records=True)
        assert o[2] == S and np.isnan(d[2 * S:3 * S]).all() and not occ[2 * S:3 * S].any()
        assert np.array_equal(np.delete(o, 2), np.delete(exp.open[:8], 2))
        assert r.get_query_stats().rays == 8 * S
        # an empty or NaN range: every pair open, nothing traced into
        for empty in (float("nan"), T / 2):
            o, d, occ = r.ambient_occlusion(pts[:64], A.SEED, S, empty, T, records=True)
            assert (o == S).all() and not occ.any() and same(d, exp.directions[:64 * S])
            assert r.get_query_stats().hits == 0


def test_f64_closed_form_and_its_near_twin():
    soa, t_max, exp = A.closed_form(False)
    with context(soa) as r:
        got = r.ambient_occlusion(A.CLOSED_POINT, A.SEED, A.CLOSED_S, t_max, T, records=True)
        equal(got, exp)
        share = int(got[0][0]) / A.CLOSED_S
        print("closed form: open share", share, "expected", 15 / 16, "bound", A.CLOSED_BOUND)
        assert abs(share - 15 / 16) <= A.CLOSED_BOUND
        _, near, exp = A.closed_form(True)
        assert near == 2.5
        got = r.ambient_occlusion(A.CLOSED_POINT, A.SEED, A.CLOSED_S, near, T, records=True)
        equal(got, exp)
        assert int(got[0][0]) == A.CLOSED_S and not got[2].any()


def test_refusals():
    soa, pts, S, t_max, _ = A.case("cornell_box")
    lib, inv = rtw._lib, _capi.RTW_E_INVALID
    inf = float("inf")
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    p8 = np.ascontiguousarray(pts[:8])
    open_, dirs, occ = np.zeros(8, np.uint32), np.zeros((16, 3)), np.zeros(16, np.uint8)
    with context(soa) as r:
        with pytest.raises(rtw.RenderError) as e:
            r.ambient_occlusion(p8, 1, 0)
        assert e.value.code == inv                                   # n_samples = 0
        with pytest.raises(rtw.RenderError) as e:
            r.ambient_occlusion(p8, 1, 1, t_min=-1.0)
        assert e.value.code == inv
        assert lib.rtw_ambient_occlusion(r.ctx, None, 8, 1, 0, 0, 2, 0.0, inf, 0, vp(open_), None, None) == inv
        assert lib.rtw_ambient_occlusion(r.ctx, vp(p8), 8, 1, 0, 0, 2, 0.0, inf, 0, None, None, None) == inv
        assert lib.rtw_ambient_occlusion(r.ctx, None, 0, 1, 0, 0, 2, 0.0, inf, 0, None, None, None) == _capi.RTW_OK
        # n over 2^40, n * S over 2^62, and n * S over 2^32 with a record: refused before anything is read
        assert lib.rtw_ambient_occlusion(r.ctx, vp(p8), (1 << 40) + 1, 1, 0, 0, 1, 0.0, inf, 0, vp(open_), None,
                                         None) == inv
        assert lib.rtw_ambient_occlusion(r.ctx, vp(p8), 1 << 40, 1, 0, 0, (1 << 22) + 1, 0.0, inf, 0, vp(open_), None,
                                         None) == inv
        assert lib.rtw_ambient_occlusion(r.ctx, vp(p8), 1 << 31, 1, 0, 0, 4, 0.0, inf, 0, vp(open_), vp(dirs),
                                         None) == inv
        assert lib.rtw_ambient_occlusion(r.ctx, vp(p8), 1 << 31, 1, 0, 0, 4, 0.0, inf, 0, vp(open_), None,
                                         vp(occ)) == inv
        # the device form: short and misaligned buffers (host pointers: refused before any is read)
        dev = lambda *a: lib.rtw_ambient_occlusion_device(r.ctx, *a, None)   # noqa: E731
        ok_args = [vp(p8), p8.nbytes, 8, 1, 0, 0, 2, 0.0, inf, 0, vp(open_), open_.nbytes, vp(dirs), dirs.nbytes,
                   vp(occ), occ.nbytes]
        for at, short in ((1, p8.nbytes - 1), (11, open_.nbytes - 1), (13, dirs.nbytes - 1), (15, occ.nbytes - 1)):
            a = list(ok_args)
            a[at] = short
            assert dev(*a) == inv, at
        big = np.zeros(16 * 6 + 2)
        mis = big.ctypes.data + (8 if big.ctypes.data % 16 == 0 else 0)   # 8 B off a 16 B boundary
        a = list(ok_args)
        a[0] = C.c_void_p(mis)
        assert mis % 16 == 8 and dev(*a) == inv                       # f64 points: 16 B
        a = list(ok_args)
        a[12] = C.c_void_p(mis + 4)
        assert dev(*a) == inv                                         # f64 directions: 8 B
        a = list(ok_args)
        a[10] = C.c_void_p(mis + 2)
        assert dev(*a) == inv                                         # open: 4 B
    # an empty light list is fine here
    with context(Q.with_lights(A.case("simple")[0], np.zeros((0, 4)))) as r:
        soa_s, pts_s, S_s, t_s, exp_s = A.case("simple")
        assert np.array_equal(r.ambient_occlusion(pts_s, A.SEED, S_s, t_s, T), exp_s.open)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        with pytest.raises(rtw.RenderError) as e:
            r.ambient_occlusion(p8, 1, 1)
        assert e.value.code == _capi.RTW_E_NO_SCENE
    with rtw.Renderer(device=0, precision=rtw.RTW_F64, virtual_ranks=2) as r:
        r.set_scene(soa)
        with pytest.raises(rtw.RenderError) as e:
            r.ambient_occlusion(p8, 1, 1)
        assert e.value.code == _capi.RTW_E_UNSUPPORTED


@pytest.mark.parametrize("precision", [rtw.RTW_F64, rtw.RTW_F32], ids=["f64", "f32"])
def test_torch_device_entry_is_the_host_entry(precision):
    import torch
    soa, pts, S, t_max, _ = A.case("cornell_box")
    dt = np.float32 if precision == rtw.RTW_F32 else np.float64
    p = np.asarray(pts, dt)
    with context(soa, precision=precision) as r:
        host = r.ambient_occlusion(p, A.SEED, S, t_max, T, first_stream=3, records=True)
        t = torch.as_tensor(p, device="cuda:0")
        dev = r.ambient_occlusion(t, A.SEED, S, t_max, T, first_stream=3, records=True)
        assert all(x.is_cuda for x in dev) and dev[0].dtype == torch.int32 and dev[2].dtype == torch.uint8
        assert np.array_equal(host[0], dev[0].cpu().numpy().view(np.uint32))
        assert same(host[1], dev[1].cpu().numpy()) and np.array_equal(host[2], dev[2].cpu().numpy())
        assert np.array_equal(r.ambient_occlusion(t, A.SEED, S, t_max, T, first_stream=3).cpu().numpy().view(np.uint32),
                              host[0])
        # continued on the device: (0, 2) then (2, 2) == S = 4
        w = r.ambient_occlusion(t, A.SEED, 2, t_max, T, first_stream=3)
        w2 = r.ambient_occlusion(t, A.SEED, 2, t_max, T, first_stream=3, first_sample=2, open=w)
        assert w2 is w and np.array_equal(w.cpu().numpy().view(np.uint32), host[0])


def test_render_ao_is_its_own_composition():
    soa, b = Q.scene("simple")
    cam = b.copy().with_image_width(40).with_image_height(24).with_samples_per_pixel(2).with_max_depth(4).build()
    seed, ao = 21, 3
    with context(soa) as r:
        got_open, got_taken = r.render_ao(cam, seed, ao_samples=ao)
        open_, taken = np.zeros(40 * 24, np.uint32), np.zeros(40 * 24, np.uint32)
        for s in range(2):
            rays, _ = r.camera_rays(cam, seed, s)
            hits, ids = r.hit_rays(rays)
            pts = np.ascontiguousarray(hits[:, 1:7])
            before = open_.copy()
            open_ = r.ambient_occlusion(pts, seed ^ 0x9E3779B97F4A7C15, ao, None, None, 0, s * ao, open=open_)
            miss = ids[:, 0] < 0
            assert np.array_equal(open_[miss], before[miss])          # a miss row takes nothing
            taken += np.where(miss, 0, ao).astype(np.uint32)
        assert got_open.shape == (24, 40) and got_open.dtype == np.uint32 and got_taken.dtype == np.uint32
        assert np.array_equal(got_open.ravel(), open_) and np.array_equal(got_taken.ravel(), taken)
        assert (got_open <= got_taken).all() and set(np.unique(got_taken)) <= {0, ao, 2 * ao}
        assert (got_taken == 0).any() and (got_open > 0).sum() >= 100 and (got_open < got_taken).sum() >= 100
        # a finite reach opens more
        near_open, near_taken = r.render_ao(cam, seed, ao_samples=ao, t_max=0.05)
        assert np.array_equal(near_taken, got_taken) and (near_open >= got_open).all() and (near_open > got_open).any()


# ------------------------------------------------------------------- f32
def f32_run(name):
    soa, pts, S, t_max, exp = A.case(name)
    p32 = np.asarray(pts, np.float32)
    with context(soa, precision=rtw.RTW_F32) as r:
        got = r.ambient_occlusion(p32, A.SEED, S, t_max, T, records=True)
        assert got[1].dtype == np.float32 and got[0].dtype == np.uint32
        st = r.get_query_stats()
        assert st.is_light_pdf == AMBIENT and st.rays == len(pts) * S and st.hits == int(got[2].sum())
        identities(r, p32, S, T, t_max, got)                         # bit for bit, the count exact
        assert np.array_equal(r.ambient_occlusion(p32, A.SEED, S, t_max, T), got[0])
    return p32, S, exp, got


@pytest.mark.parametrize("name", list(A.CASES))
def test_f32_identities_and_the_share_of_pairs_that_differ_from_f64(name):
    p32, S, exp, (open_, dirs, occ) = f32_run(name)
    differ = occ != exp.occluded
    share = float(differ.mean())
    print(f"{name} f32: {int(differ.sum())} of {len(occ)} pairs answer otherwise than the f64 case file "
          f"({100 * share:.3f} %, cap {100 * CAP:.0f} %)")
    assert share <= CAP
    # the counts differ only where a pair does
    changed = differ.reshape(-1, S).any(1)
    assert np.array_equal(open_[~changed], exp.open[~changed])


def cosine_form(dtype, p32, S):
    """f32_forms.cone_or_cosine's cosine lobe about the f32 normals: (directions [n * S, 3], Onb's w.x)"""
    F = FF.Forms(dtype, True)
    U = FF.Uniforms(F, True)
    n = len(p32)
    out, wx = np.zeros((n * S, 3), np.float64), np.zeros(n * S, np.float64)
    nrm = FF.v3(F.arr(p32[:, 3:6]))
    zero = (np.zeros(n, F.dt),) * 3
    for j in range(S):
        s = FF.rng_seed(A.SEED, np.arange(n, dtype=np.uint64), j)
        d = FF.cone_or_cosine(F, U, s, np.zeros(n, bool), nrm, zero, np.zeros(n, F.dt), zero)
        out[j::S] = FF.stack3(d)
        wx[j::S] = F.normalize(nrm)[0]
    return out, wx


def test_f32_directions_against_the_f32_forms():
    kernel, law, cal, wx_law, wx_cal = [], [], [], [], []
    for name in A.CASES:
        p32, S, exp, got = f32_run(name)
        kernel.append(got[1].astype(np.float64))
        for dtype, ds, ws in ((np.float64, law, wx_law), (np.float32, cal, wx_cal)):
            d, wx = cosine_form(dtype, p32, S)
            ds.append(d)
            ws.append(wx)
    kernel, law, cal = np.concatenate(kernel), np.concatenate(law), np.concatenate(cal)
    wx_law, wx_cal = np.concatenate(wx_law), np.concatenate(wx_cal)
    assert len(law) >= 1000 and np.isfinite(law).all() and np.isfinite(kernel).all()
    tiny = np.finfo(np.float32).tiny
    err = lambda x: np.abs(x - law).max(1) / np.maximum(np.abs(law).max(1), tiny)   # noqa: E731
    ek, ec = err(kernel), err(cal)
    # near a decision: Onb's |w.x| > 0.9 within 4 x the calibration's p99 error in w.x
    near = np.abs(np.abs(wx_law) - 0.9) <= ALLOW * np.percentile(np.abs(wx_law - wx_cal), 99)
    no_cal = (np.abs(wx_law) > 0.9) != (np.abs(wx_cal) > 0.9)
    assert not (no_cal & ~near).any()
    out = near & (no_cal | (ek > 64.0 * ec[~no_cal].max()))
    assert out.mean() <= CAP
    keep = ~out
    for q in (50, 99, 100):
        k, c = float(np.percentile(ek[keep], q)), float(np.percentile(ec[keep], q))
        print(f"f32 directions p{q}: kernel {k:.3e}, calibration {c:.3e}, ratio {k / c if c else 0.0:.3f} "
              f"({int(keep.sum())} rows, {int(out.sum())} left out)")
        assert k <= ALLOW * c, (q, k, c)
