"""The rules of one path advance (rtw_path_advance, include/rtw.h) restated in
numpy, and the synthetic records the GPU test runs them on.  The restatement
is held against Renderer.render_wavefront's own lines by
tests/test_wavefront_host.py; tests/test_gpu_path_advance.py compares the
kernel with it bit for bit."""
import numpy as np

MISS, ABSORBED, REFLECT, SCATTER = 0, 1, 2, 3
BLOCK = 256                                    # the kernel's workgroup: survivors of a block stay together
SENTINEL = 12345.0                             # what untouched colour slots and out-state rows hold


def bits(a):
    """the values' bit patterns, every NaN as the one pattern of all ones (payloads aside)"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    u = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).copy()
    u[np.isnan(a)] = ~u.dtype.type(0)
    return u


def same(a, b):
    """bit for bit, the sign of zero included; NaNs compared as NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


def advance(rec, colour, bg, last=False):
    """One advance of the records `rec` (a dict of mult, res, slot, event,
    weight, emitted, nxt, rng): (the survivors' state in input order -- a dict
    of rays, rng, mult, res, slot --, the colour array afterwards).  Every
    component in the records' dtype, each product rounded before its add."""
    dt = rec["mult"].dtype
    mult, res, e, w, ev = rec["mult"], rec["res"], rec["emitted"], rec["weight"], rec["event"]
    slot = rec["slot"].astype(np.int64)
    bg = np.asarray(bg, dt)
    colour = colour.copy()
    with np.errstate(all="ignore"):
        miss, gone = ev == MISS, ev == ABSORBED
        scat, refl = ev == SCATTER, ev == REFLECT
        other = ~(miss | gone | scat | refl)
        colour[slot[miss]] = mult[miss] * bg + res[miss]
        colour[slot[gone]] = mult[gone] * e[gone] + res[gone]
        colour[slot[other]] = mult[other] * dt.type(0) + res[other]    # a miss into black
        res2 = res.copy()
        res2[scat] = res[scat] + mult[scat] * e[scat]
        keep = scat | refl
        mult2 = mult[keep] * w[keep]
        res2 = res2[keep]
        if last:
            colour[slot[keep]] = dt.type(0) + res2
            keep = np.zeros_like(keep)
            mult2, res2 = mult2[:0], res2[:0]
    out = {"rays": rec["nxt"][keep], "rng": rec["rng"][keep], "mult": mult2, "res": res2, "slot": rec["slot"][keep]}
    return out, colour


def records(n, dtype, kind="mixed", seed=1, slots=None):
    """n synthetic paths.  kind: 'mixed' (the four events, one out-of-range
    value, NaN, inf and -0 among mult / res / emitted / weight), 'end' (every
    path ends), 'go' (every path survives).  The slots are a shuffled
    permutation of range(slots or n)."""
    g = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    f = lambda *shape: g.uniform(-2.0, 2.0, shape).astype(dt)   # noqa: E731
    rec = {"mult": f(n, 3), "res": f(n, 3), "weight": f(n, 3), "emitted": f(n, 3), "nxt": f(n, 6),
           "rng": g.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1),
           "slot": g.permutation(slots or n)[:n].astype(np.uint32)}
    if kind == "end":
        ev = g.integers(0, 2, n)
    elif kind == "go":
        ev = g.integers(2, 4, n)
    else:
        ev = g.integers(0, 4, n)
        if n > 5:
            ev[:4] = (MISS, ABSORBED, REFLECT, SCATTER)
            ev[n // 2] = 7                                     # no event: a miss into black
            ev[n - 1] = -3
        for k, (name, col, v) in enumerate((("mult", 0, np.nan), ("mult", 1, np.inf), ("emitted", 2, np.nan),
                                            ("emitted", 0, -np.inf), ("res", 1, -0.0), ("mult", 2, -0.0),
                                            ("emitted", 1, -0.0), ("weight", 0, -0.0), ("weight", 2, np.inf),
                                            ("res", 0, np.nan), ("emitted", 0, 0.0), ("mult", 0, 0.0))):
            rows = np.arange(k, n, 13)                         # every event meets every special value
            rec[name][rows, col] = v
    rec["event"] = ev.astype(np.int32)
    return rec


def blocks_keep_their_order(in_slot, keep, out_slot):
    """The survivors of each BLOCK of input paths are contiguous in the out-state
    and in input order (the slots are distinct: they name the paths)."""
    where = {int(s): k for k, s in enumerate(out_slot.tolist())}
    for at in range(0, len(in_slot), BLOCK):
        want = [int(s) for s, k in zip(in_slot[at:at + BLOCK].tolist(), keep[at:at + BLOCK].tolist()) if k]
        if want:
            first = where[want[0]]
            if out_slot[first:first + len(want)].tolist() != want:
                return False
    return True
