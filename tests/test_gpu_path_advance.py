"""rtw_path_advance on the GPU against its numpy restatement
(tests/wavefront_cases.py, held against Renderer.render_wavefront's lines by
tests/test_wavefront_host.py), on synthetic records: after sorting the
out-state by slot every field is the restatement's bit for bit (NaNs as NaN,
the sign of zero included), colour is equal and untouched slots keep their
sentinel, the count and the query stats are right, the survivors of each block
of 256 stay together and in order, the host and the device form agree,
overlapping buffers are refused, and a slot beyond the colour array is refused
(host) or skipped (device).  n = 1000 is no multiple of 64 or 256."""
import functools

import numpy as np
import pytest
import torch

import ray_tracing_weekend_amd as rtw
import wavefront_cases as WC
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

BG = (0.7, 0.8, 1.0)
PRECISIONS = [pytest.param(rtw.RTW_F32, id="f32"), pytest.param(rtw.RTW_F64, id="f64")]
FIELDS = ("rays", "rng", "mult", "res", "slot")
ORDER = ("mult", "res", "slot", "event", "weight", "emitted", "nxt", "rng")


def dtype_of(precision):
    return np.float32 if precision == rtw.RTW_F32 else np.float64


@functools.lru_cache(maxsize=None)
def case(precision, n, kind, last=False, slots=None):
    """(records, expected survivors in input order, expected colour): computed once, never written to"""
    dt = dtype_of(precision)
    rec = WC.records(n, dt, kind, seed=n + 1, slots=slots)
    colour = np.full((slots or n, 3), WC.SENTINEL, dt)
    out, want_colour = WC.advance(rec, colour, BG, last)
    for a in (*rec.values(), *out.values(), want_colour):
        a.flags.writeable = False
    return rec, out, want_colour


def sentinel_out(n, dt):
    return (np.full((n, 6), WC.SENTINEL, dt), np.full((n, 4), 77, np.uint64), np.full((n, 3), WC.SENTINEL, dt),
            np.full((n, 3), WC.SENTINEL, dt), np.full(n, 0xABCD, np.uint32))


def run_host(r, rec, n_slots, last=False):
    """(survivors, colour, the whole out buffers) of the host form"""
    dt = rec["mult"].dtype
    n = len(rec["slot"])
    colour = np.full((n_slots, 3), WC.SENTINEL, dt)
    bufs = sentinel_out(n, dt)
    out = r.path_advance(*[rec[k] for k in ORDER], colour, BG, last, out=bufs)
    return dict(zip(FIELDS, out)), colour, dict(zip(FIELDS, bufs))


def to_dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.as_tensor(a.copy()).cuda()


def to_host(t, like):
    a = t.cpu().numpy()
    return a.view(like) if a.dtype != like and a.dtype.itemsize == np.dtype(like).itemsize and a.dtype.kind == "i" else a


def run_device(r, rec, n_slots, last=False):
    dt = rec["mult"].dtype
    n = len(rec["slot"])
    colour = to_dev(np.full((n_slots, 3), WC.SENTINEL, dt))
    bufs = tuple(to_dev(b) for b in sentinel_out(n, dt))
    out = r.path_advance(*[to_dev(rec[k]) for k in ORDER], colour, BG, last, out=bufs)
    kinds = (dt, np.uint64, dt, dt, np.uint32)
    return ({f: to_host(t, k) for f, t, k in zip(FIELDS, out, kinds)}, colour.cpu().numpy(),
            {f: to_host(t, k) for f, t, k in zip(FIELDS, bufs, kinds)})


def check(r, rec, want, want_colour, got, colour, bufs, n_slots):
    n, m = len(rec["slot"]), len(want["slot"])
    assert len(got["slot"]) == m                                  # the count
    if n:
        st = r.get_query_stats()
        assert (st.is_light_pdf, st.rays, st.hits) == (6, n, m)
    by_got, by_want = np.argsort(got["slot"], kind="stable"), np.argsort(want["slot"], kind="stable")
    for f in FIELDS:
        assert WC.same(got[f][by_got], want[f][by_want]), f       # NaN as NaN, -0 as -0
    assert WC.same(colour, want_colour[:n_slots])
    ended = np.setdiff1d(rec["slot"], want["slot"])
    untouched = np.setdiff1d(np.arange(n_slots), ended)
    assert (colour[untouched] == WC.SENTINEL).all()               # only a path that ends writes its slot
    keep = np.isin(rec["slot"], want["slot"])
    assert WC.blocks_keep_their_order(rec["slot"], keep, got["slot"])
    fresh = sentinel_out(n, rec["mult"].dtype)
    for f, s in zip(FIELDS, fresh):                               # rows beyond the count are left as they were
        assert WC.same(bufs[f][m:], s[m:]), f


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,kind,last", [(1000, "mixed", False), (1000, "end", False), (1000, "go", False),
                                         (0, "mixed", False), (1, "go", False), (1, "end", False),
                                         (257, "mixed", False), (1000, "mixed", True), (257, "go", True)])
def test_advance_is_the_restatement(precision, n, kind, last):
    rec, want, want_colour = case(precision, n, kind, last)
    if kind == "mixed" and n >= 257:
        ev = rec["event"]
        assert {0, 1, 2, 3} <= set(ev.tolist()) and ((ev < 0) | (ev > 3)).sum() == 2
        assert np.isnan(rec["mult"]).any() and np.isinf(rec["emitted"]).any() and np.signbit(rec["res"][rec["res"] == 0]).any()
        assert (rec["slot"] != np.arange(n)).any()
    if kind == "end" or last:
        assert len(want["slot"]) == 0
    if kind == "go" and not last:
        assert len(want["slot"]) == n
    with rtw.Renderer(device=0, precision=precision) as r:        # (no scene: an advance reads none)
        got_h, colour_h, bufs_h = run_host(r, rec, n, last)
        check(r, rec, want, want_colour, got_h, colour_h, bufs_h, n)
        got_d, colour_d, bufs_d = run_device(r, rec, n, last)
        check(r, rec, want, want_colour, got_d, colour_d, bufs_d, n)
        # the two forms agree (block order aside)
        a, b = np.argsort(got_h["slot"], kind="stable"), np.argsort(got_d["slot"], kind="stable")
        for f in FIELDS:
            assert WC.same(got_h[f][a], got_d[f][b]), f
        assert WC.same(colour_h, colour_d)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_overlapping_buffers_are_refused(precision):
    rec, _, _ = case(precision, 257, "mixed")
    dt = dtype_of(precision)
    with rtw.Renderer(device=0, precision=precision) as r:
        colour = np.full((257, 3), WC.SENTINEL, dt)
        ins = [rec[k].copy() for k in ORDER]
        bufs = list(sentinel_out(257, dt))
        bufs[2] = ins[0]                                           # out mult = in mult: in place
        with pytest.raises(rtw.RenderError) as e:
            r.path_advance(*ins, colour, BG, out=tuple(bufs))
        assert e.value.code == _capi.RTW_E_INVALID and "overlaps" in str(e.value)
        assert (colour == WC.SENTINEL).all() and WC.same(ins[0], rec["mult"])
        d_ins = [to_dev(rec[k]) for k in ORDER]
        d_colour = to_dev(colour)
        for victim, at in ((6, 0), (4, 2), (7, 1)):                # out rays = next, out mult = weight, out rng = rng
            d_bufs = [to_dev(b) for b in sentinel_out(257, dt)]
            d_bufs[at] = d_ins[victim]
            with pytest.raises(rtw.RenderError) as e:
                r.path_advance(*d_ins, d_colour, BG, out=tuple(d_bufs))
            assert e.value.code == _capi.RTW_E_INVALID and "overlaps" in str(e.value)
        d_bufs = [to_dev(b) for b in sentinel_out(257, dt)]
        with pytest.raises(rtw.RenderError) as e:                  # out res = colour
            r.path_advance(*d_ins, d_colour, BG, out=(d_bufs[0], d_bufs[1], d_bufs[2], d_colour, d_bufs[4]))
        assert e.value.code == _capi.RTW_E_INVALID
        assert (d_colour.cpu().numpy() == WC.SENTINEL).all()       # nothing ran


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_slot_beyond_the_colour_array(precision):
    """The host form refuses it; in a device buffer it is the caller's error and
    that path's colour is skipped: nothing is written out of bounds, every other
    path is as ever."""
    n, cap = 1000, 900
    rec, want, want_colour = case(precision, n, "mixed")
    assert ((rec["slot"] >= cap) & (rec["event"] < 2)).sum() > 10
    with rtw.Renderer(device=0, precision=precision) as r:
        with pytest.raises(rtw.RenderError) as e:
            run_host(r, rec, cap)
        assert e.value.code == _capi.RTW_E_INVALID and "slot" in str(e.value)
        # the colour tensor is the head of a larger one: what lies behind it keeps its sentinel
        dt = rec["mult"].dtype
        whole = to_dev(np.full((n, 3), WC.SENTINEL, dt))
        bufs = tuple(to_dev(b) for b in sentinel_out(n, dt))
        out = r.path_advance(*[to_dev(rec[k]) for k in ORDER], whole[:cap], BG, out=bufs)
        assert len(out[4]) == len(want["slot"])
        got = whole.cpu().numpy()
        assert WC.same(got[:cap], want_colour[:cap]) and (got[cap:] == WC.SENTINEL).all()
        by_got = np.argsort(to_host(out[4], np.uint32), kind="stable")
        by_want = np.argsort(want["slot"], kind="stable")
        assert WC.same(out[2].cpu().numpy()[by_got], want["mult"][by_want])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_begin_and_short_or_misaligned_buffers(precision):
    dt = dtype_of(precision)
    with rtw.Renderer(device=0, precision=precision) as r:
        mult, res, slot = r.path_begin(1000, first_slot=37)
        assert WC.same(mult.cpu().numpy(), np.ones((1000, 3), dt)) and WC.same(res.cpu().numpy(), np.zeros((1000, 3), dt))
        assert slot.cpu().numpy().view(np.uint32).tolist() == list(range(37, 1037))
        top = r.path_begin(3, first_slot=(1 << 32) - 3)[2]
        assert top.cpu().numpy().view(np.uint32).tolist() == [(1 << 32) - 3, (1 << 32) - 2, (1 << 32) - 1]
        with pytest.raises(rtw.RenderError):
            r.path_begin(4, first_slot=(1 << 32) - 3)
        rec, _, _ = case(precision, 257, "mixed")
        d_ins = [to_dev(rec[k]) for k in ORDER]
        colour = to_dev(np.zeros((257, 3), dt))
        short = [to_dev(b) for b in sentinel_out(257, dt)]
        short[3] = short[3][:200]                                  # out res: fewer than n rows
        with pytest.raises(rtw.RenderError) as e:
            r.path_advance(*d_ins, colour, BG, out=tuple(short))
        assert e.value.code == _capi.RTW_E_INVALID and "smaller" in str(e.value)
        odd = [to_dev(b) for b in sentinel_out(258, dt)]
        odd[1] = odd[1].reshape(-1)[1:1 + 257 * 4].reshape(257, 4)   # out rng 8 bytes off its 16
        with pytest.raises(rtw.RenderError) as e:
            r.path_advance(*d_ins, colour, BG, out=tuple(odd))
        assert e.value.code == _capi.RTW_E_INVALID and "aligned" in str(e.value)
