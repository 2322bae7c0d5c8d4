"""The variance-guided filter (rtw_denoise_variance, include/rtw.h) restated in
numpy, and the inputs of tests/test_denoise_variance_host.py and
tests/test_gpu_denoise_variance.py -- nothing here touches the GPU.

As denoise_cases.restate, the restatement is independent of the kernels: the 25
taps of an iteration in the written order (dy outer, dx inner), each handled
for the whole image at once with numpy elementwise operations -- each an IEEE
f64 operation rounded by itself -- in the order rtw.h writes them; compare and
select is np.where on that comparison; a skipped tap leaves the accumulators as
they are."""
import functools
import os

import numpy as np

import denoise_cases as D

H5 = D.H5
EPS = 2.0 ** -40
# what the library ships (rtw_denoise_variance_params_default)
SHIPPED = dict(iterations=5, normal_power_log2=5, sigma_var=2.0, sigma_depth=0.125, demodulate=1, fill_nonfinite=1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "variance_frame_simple_64x40.npz")


def luma(c):
    return ((0.2126 * c[..., 0]) + (0.7152 * c[..., 1])) + (0.0722 * c[..., 2])


def restate_variance(sums, features, moments, n, *, iterations, normal_power_log2, sigma_var, sigma_depth, demodulate,
                     fill_nonfinite, details=False):
    """(means [H, W, 3], filled, left_nonfinite) of the filter; n: spp or counts
    [H, W].  details: also (has_var [H, W], the last iteration's ve [H, W])."""
    S = np.asarray(sums).astype(np.float64)           # f32 sums widen exactly
    Ft = np.asarray(features, np.float64)
    M = np.asarray(moments, np.float64)
    H, W = S.shape[:2]
    cnt = np.broadcast_to(np.asarray(n, np.uint32), (H, W))
    nd1 = cnt.astype(np.float64)
    nd = nd1[..., None]
    sampled = cnt > 0
    with np.errstate(all="ignore"):
        guide_ok = sampled & np.isfinite(Ft).all(-1)
        c = S / nd
        raw = np.where(sampled[..., None], c, 0.0)
        valid = guide_ok & np.isfinite(c).all(-1)
        if demodulate:
            alb = Ft[..., 0:3] / nd
            a = np.where(alb > 2.0 ** -10, alb, 2.0 ** -10)
            aY = luma(a)
        else:
            a = np.ones((H, W, 3))
            aY = np.ones((H, W))
        e = c / a
        ln = np.sqrt((Ft[..., 3] * Ft[..., 3] + Ft[..., 4] * Ft[..., 4]) + Ft[..., 5] * Ft[..., 5])
        N = np.where((ln > 0)[..., None], Ft[..., 3:6] / ln[..., None], 0.0)
        d = np.where(Ft[..., 7] > 0, Ft[..., 6] / Ft[..., 7], 0.0)
        n_zero = (N == 0).all(-1)
        # the variance of the mean of the irradiance's luminance
        m = M[..., 0] / nd1
        q = M[..., 1] / nd1
        var = q - m * m
        var = np.where(var > 0, var, 0.0)
        v = var / (nd1 - 1.0)
        ve = v / (aY * aY)
        has_var = valid & (cnt > 1) & np.isfinite(M).all(-1) & np.isfinite(ve)
        ve = np.where(has_var, ve, 0.0)
        sv2 = sigma_var * sigma_var
        valid0 = valid.copy()
        rows, cols = np.arange(H)[:, None], np.arange(W)[None, :]
        for k in range(iterations):
            step = 2 ** k
            thr = sv2 * ve + EPS
            Ye = luma(e)
            num = np.zeros((H, W, 3))
            den = np.zeros((H, W))
            vnum = np.zeros((H, W))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    jj, ii = rows + dy * step, cols + dx * step
                    inside = (jj >= 0) & (jj < H) & (ii >= 0) & (ii < W)
                    jc, ic = np.broadcast_arrays(np.clip(jj, 0, H - 1), np.clip(ii, 0, W - 1))
                    use = guide_ok & inside & valid[jc, ic]
                    if not use.any():
                        continue
                    Nq, dq, eq, veq = N[jc, ic], d[jc, ic], e[jc, ic], ve[jc, ic]
                    t = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                    t = np.where(t > 0, t, 0.0)
                    for _ in range(normal_power_log2):
                        t = t * t
                    w_n = np.where(n_zero & n_zero[jc, ic], 1.0, t)
                    mx = np.where(d > dq, d, dq)
                    r = np.abs(d - dq) / mx
                    x = r / sigma_depth
                    u = 1.0 - x * x
                    u = np.where(u > 0, u, 0.0)
                    w_d = np.where(mx > 0, u * u, 1.0)
                    g = Ye - Ye[jc, ic]
                    s = g * g
                    w_c = np.where(has_var, 1.0 / (1.0 + s / thr), 1.0)
                    w = (((H5[dy + 2] * H5[dx + 2]) * w_n) * w_d) * w_c
                    num = np.where(use[..., None], num + w[..., None] * eq, num)
                    den = np.where(use, den + w, den)
                    vnum = np.where(use, vnum + (w * w) * veq, vnum)
            fills = guide_ok & ~valid & bool(fill_nonfinite) & (den > 0)
            takes = valid | fills
            e = np.where(takes[..., None], num / den[..., None], e)
            ve = np.where(takes & has_var, vnum / (den * den), ve)
            valid = takes
        out = np.where(valid[..., None], e * a, raw)
    filled = int((guide_ok & ~valid0 & valid).sum())
    left = int((~np.isfinite(out).all(-1)).sum())
    if details:
        return out, filled, left, has_var, ve
    return out, filled, left


@functools.lru_cache(maxsize=None)
def synthetic_moments(width, height, seed=1, spp=16):
    """Moments [H, W, 2] to go with D.synthetic(width, height, seed, spp): the
    {S1, S2} of samples whose mean luminance is the frame's and whose spread is
    drawn per pixel, with, sprinkled over them, zero variance (S2 = S1^2 / n, up
    to rounding), a variance the rounding makes negative, NaN and +-inf moments
    and -- through counts_with_ones -- pixels of one sample.  Shared: do not
    write to it."""
    sums, _, counts = D.synthetic(width, height, seed, spp)
    rng = np.random.default_rng(5000 * seed + 11 * width + height)
    H, W = height, width
    nd = np.maximum(counts, 1).astype(np.float64)
    with np.errstate(all="ignore"):
        y = np.nan_to_num(luma(sums / nd[..., None]), nan=0.5, posinf=1.0, neginf=0.0)
    sd = y * rng.gamma(2.0, 0.15, (H, W))
    S1 = y * nd
    S2 = (sd * sd + y * y) * nd
    pick = lambda p: rng.random((H, W)) < p   # noqa: E731
    z = pick(0.05)
    S2[z] = (S1[z] * S1[z]) / nd[z]
    neg = pick(0.02)
    S2[neg] = S2[neg] * 0.5
    moments = np.stack([S1, S2], -1)
    moments[pick(0.02), 0] = np.nan
    moments[pick(0.02), 1] = np.inf
    moments[pick(0.01), 0] = -np.inf
    moments[pick(0.01), 1] = np.nan
    moments.setflags(write=False)
    return moments


@functools.lru_cache(maxsize=None)
def counts_with_ones(width, height, seed=1, spp=16):
    """D.synthetic's counts with some pixels of exactly one sample (n <= 1 has no
    variance).  Shared: do not write to it."""
    _, _, counts = D.synthetic(width, height, seed, spp)
    rng = np.random.default_rng(9000 * seed + 13 * width + height)
    c = counts.copy()
    if width * height > 1:
        c[(rng.random(c.shape) < 0.05) & (c > 0)] = 1
    c.setflags(write=False)
    return c


def constant_moments(width, height, spp=8, colour=(0.3, 0.5, 0.7), spread=0.1):
    """The moments of a constant image whose every sample had luminance Y +-
    spread, half each: S1 = n Y, S2 = n (Y^2 + spread^2)."""
    y = float(luma(np.array(colour)))
    return np.tile(np.array([y * spp, (y * y + spread * spread) * spp]), (height, width, 1))


@functools.lru_cache(maxsize=None)
def golden_frame():
    """tests/golden/variance_frame_simple_64x40.npz (tests/golden/make_variance_frame.py):
    sums_N, features_N, moments_N for N in 16, 64, 256 of seed 7, and ref, the
    4096-spp means of seed 8."""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
