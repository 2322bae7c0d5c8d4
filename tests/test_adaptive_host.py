"""Adaptive sampling without a GPU: the stop rule on the oracle's per-sample
values really tells tiles apart (so the GPU tests cannot pass trivially), and
the count-aware encoders (rtw_encode_rgb8_counts / rtw_write_ppm_counts)."""
import collections

import numpy as np

import adaptive_rule as A
import ray_tracing_weekend_amd as rtw


def test_rule_on_oracle_samples_tells_tiles_apart():
    """scenes.simple, 36 x 20 (partial tiles on both axes), depth 8, render
    seed 11, samples 0..31 from oracle.trace_sample; min 4 / window 4 / max 32.
    Measured when written: tolerance 0.125 -> 5 tiles at 4, 4 at 12, 5 at 16,
    1 at 32; tolerance 0 -> 5 at 4 (the constant sky tiles), 10 at 32; seven
    pixels are NaN by sample 32.  Asserted: the condition, not the histogram."""
    samples = A.oracle_samples()
    sums, counts = A.adaptive(samples, 4, 32, 4, 0.125)
    hist = collections.Counter(A.tile_counts(counts))
    print("tolerance 0.125:", sorted(hist.items()))
    assert len(hist) >= 3 and 4 in hist and 32 in hist
    assert set(hist) <= set(A.pass_ends(4, 32, 4))
    # all pixels of a tile share its count
    for ty in range(0, A.H, 8):
        for tx in range(0, A.W, 8):
            assert len(np.unique(counts[ty:ty + 8, tx:tx + 8])) == 1
    # the invariant of the restatement itself: sums = the fold of the first `counts` samples
    j, i = 13, 30
    acc = np.zeros(3)
    for s in range(int(counts[j, i])):
        acc = acc + samples[j, i, s]
    assert np.array_equal(acc, sums[j, i], equal_nan=True)
    # tolerance 0: only tiles whose every pixel is constant stop before max
    _, c0 = A.adaptive(samples, 4, 32, 4, 0.0)
    print("tolerance 0:", sorted(collections.Counter(A.tile_counts(c0)).items()))
    assert set(np.unique(c0)) <= {4, 32}
    y = A.luma(samples)
    print("NaN pixels by sample 32:", int(np.isnan(samples).any(axis=(2, 3)).sum()))
    for ty in range(0, A.H, 8):
        for tx in range(0, A.W, 8):
            t = y[ty:ty + 8, tx:tx + 8, :4]
            constant = bool((np.isnan(t).any(-1) | (t == t[..., :1]).all(-1)).all())
            assert (c0[ty, tx] == 4) == constant, (ty, tx)


def _sums(h=9, w=13, seed=3):
    rng = np.random.default_rng(seed)
    s = rng.random((h, w, 3)) * 40.0
    s[0, 0] = [np.nan, -1.0, 1e9]
    s[1, 2] = [0.0, np.inf, 7.0]
    return s


def test_encode_counts_constant_equals_spp():
    s = _sums()
    for n in (1, 7, 32):
        counts = np.full(s.shape[:2], n, np.uint32)
        assert np.array_equal(rtw.encode_rgb8(s, counts), rtw.encode_rgb8(s, n))


def test_encode_counts_mixed_equals_restatement():
    s = _sums()
    rng = np.random.default_rng(5)
    counts = rng.integers(2, 500, s.shape[:2]).astype(np.uint32)
    got = rtw.encode_rgb8(s, counts)
    # colour.rs:14-36 per pixel: scale = 1 / count; (256 * clamp(sqrt(sum * scale), 0, 1)) as u8, NaN -> 0
    with np.errstate(all="ignore"):
        x = np.sqrt(s * (1.0 / counts.astype(np.float64))[..., None])
        v = 256.0 * np.where(np.isnan(x), x, np.clip(x, 0.0, 1.0))
    want = np.where(v > 0.0, np.where(v >= 255.0, 255.0, np.floor(np.where(np.isnan(v), 0.0, v))), 0.0)
    want = want.astype(np.uint8)[::-1]
    assert np.array_equal(got, want)
    assert len(np.unique(got)) > 50


def test_write_ppm_counts_round_trips(tmp_path):
    s = _sums()
    counts = np.random.default_rng(6).integers(2, 64, s.shape[:2]).astype(np.uint32)
    path = str(tmp_path / "a.ppm")
    n = rtw.write_ppm(path, s, counts)
    text = open(path).read()
    assert n == len(text)
    tok = text.split()
    assert tok[:4] == ["P3", str(s.shape[1]), str(s.shape[0]), "255"]
    px = np.array(tok[4:], np.uint8).reshape(s.shape)
    assert np.array_equal(px, rtw.encode_rgb8(s, counts))
    # a wrong shape is refused, a plain spp still works
    try:
        rtw.encode_rgb8(s, counts[:-1])
        raise AssertionError("counts of the wrong shape were accepted")
    except rtw.RenderError:
        pass
    assert rtw.write_ppm(path, s, 9) > 0
