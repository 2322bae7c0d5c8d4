"""The denoiser's filter (rtw_denoise, include/rtw.h) restated in numpy, and the
inputs of tests/test_denoise_host.py and tests/test_gpu_denoise.py -- nothing
here touches the GPU.

The restatement is independent of the kernels: it walks the 25 taps of an
iteration in the written order (dy outer, dx inner) and handles each tap for
the whole image at once with numpy elementwise operations -- each an IEEE f64
operation rounded by itself -- in the order rtw.h writes them.  Where the
contract says compare and select it is np.where on that comparison, never
np.maximum.  A skipped tap leaves the accumulators as they are."""
import functools

import numpy as np

import feature_cases as F
from oracle import oracle as O

H5 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
# the parameters the filter was specified with, and what the library ships as its
# defaults after the quality sweep of tools/denoise_bench.py (sigma_colour moved)
START = dict(iterations=5, normal_power_log2=5, sigma_colour=1.0, sigma_depth=0.125, demodulate=1, fill_nonfinite=1)
SHIPPED = dict(START, sigma_colour=0.5)


def restate(sums, features, n, *, iterations, normal_power_log2, sigma_colour, sigma_depth, demodulate,
            fill_nonfinite):
    """(means [H, W, 3], filled, left_nonfinite) of the filter; n: spp or counts [H, W]."""
    S = np.asarray(sums).astype(np.float64)           # f32 sums widen exactly
    Ft = np.asarray(features, np.float64)
    H, W = S.shape[:2]
    cnt = np.broadcast_to(np.asarray(n, np.uint32), (H, W))
    nd = cnt.astype(np.float64)[..., None]
    sampled = cnt > 0
    with np.errstate(all="ignore"):
        guide_ok = sampled & np.isfinite(Ft).all(-1)
        c = S / nd
        raw = np.where(sampled[..., None], c, 0.0)
        valid = guide_ok & np.isfinite(c).all(-1)
        if demodulate:
            alb = Ft[..., 0:3] / nd
            a = np.where(alb > 2.0 ** -10, alb, 2.0 ** -10)
        else:
            a = np.ones((H, W, 3))
        e = c / a
        ln = np.sqrt((Ft[..., 3] * Ft[..., 3] + Ft[..., 4] * Ft[..., 4]) + Ft[..., 5] * Ft[..., 5])
        N = np.where((ln > 0)[..., None], Ft[..., 3:6] / ln[..., None], 0.0)
        d = np.where(Ft[..., 7] > 0, Ft[..., 6] / Ft[..., 7], 0.0)
        n_zero = (N == 0).all(-1)
        valid0 = valid.copy()
        rows, cols = np.arange(H)[:, None], np.arange(W)[None, :]
        for k in range(iterations):
            step = 2 ** k
            s_k = sigma_colour * 2.0 ** -k
            sc2 = s_k * s_k
            num = np.zeros((H, W, 3))
            den = np.zeros((H, W))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    jj, ii = rows + dy * step, cols + dx * step
                    inside = (jj >= 0) & (jj < H) & (ii >= 0) & (ii < W)
                    jc, ic = np.broadcast_arrays(np.clip(jj, 0, H - 1), np.clip(ii, 0, W - 1))
                    use = guide_ok & inside & valid[jc, ic]
                    if not use.any():
                        continue
                    Nq, dq, eq = N[jc, ic], d[jc, ic], e[jc, ic]
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
                    if sigma_colour == 0:
                        w_c = 1.0
                    else:
                        g = e - eq
                        s = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
                        w_c = np.where(valid, 1.0 / (1.0 + s / sc2), 1.0)
                    w = (((H5[dy + 2] * H5[dx + 2]) * w_n) * w_d) * w_c
                    num = np.where(use[..., None], num + w[..., None] * eq, num)
                    den = np.where(use, den + w, den)
            fills = guide_ok & ~valid & bool(fill_nonfinite) & (den > 0)
            e = np.where((valid | fills)[..., None], num / den[..., None], e)
            valid = valid | fills
        out = np.where(valid[..., None], e * a, raw)
    filled = int((guide_ok & ~valid0 & valid).sum())
    left = int((~np.isfinite(out).all(-1)).sum())
    return out, filled, left


SURFACES = (((0.0, 1.0, 0.0), 4.0), ((0.6, 0.0, 0.8), 2.0), ((-0.8, 0.6, 0.0), 2.25), ((0.0, 0.0, 0.0), 0.0))


@functools.lru_cache(maxsize=None)
def synthetic(width, height, seed=1, spp=16):
    """(sums [H, W, 3], features [H, W, 8], counts [H, W]) of a made-up frame: a
    few surfaces in blocks of pixels (the last is the sky: normal 0, distance 0)
    with noisy colours, normals and distances, and sprinkled over them pixels
    without samples, NaN and +-inf colours, non-finite feature channels and
    albedos below 2^-10.  The arrays are shared: do not write to them."""
    rng = np.random.default_rng(1000 * seed + 7 * width + height)
    H, W = height, width
    counts = rng.integers(spp // 2, spp + 1, (H, W)).astype(np.uint32)
    jj, ii = np.mgrid[0:H, 0:W]
    surf = ((jj // 5) + (ii // 7) + rng.integers(0, 2, (H, W)) * (rng.random((H, W)) < 0.1)) % len(SURFACES)
    features = np.zeros((H, W, 8))
    sums = np.zeros((H, W, 3))
    for s, (nrm, dist) in enumerate(SURFACES):
        m = surf == s
        k = int(m.sum())
        cn = counts[m].astype(np.float64)
        sky = dist == 0.0
        hits = np.zeros(k) if sky else np.floor(cn * np.where(rng.random(k) < 0.8, 1.0, rng.random(k)))
        albedo = np.clip(np.array([0.2 + 0.2 * s, 0.5, 0.9 - 0.2 * s]) + rng.normal(0, 0.02, (k, 3)), 0, 1)
        features[m, 0:3] = albedo * cn[:, None]
        features[m, 3:6] = (np.array(nrm) + rng.normal(0, 0.03, (k, 3)) * (not sky)) * hits[:, None]
        features[m, 6] = dist * (1 + rng.normal(0, 0.01, k)) * hits
        features[m, 7] = hits
        sums[m] = albedo * (0.6 + rng.gamma(4.0, 0.1, (k, 3))) * cn[:, None]
    pick = lambda p: rng.random((H, W)) < p   # noqa: E731
    counts[pick(0.03)] = 0
    sums[pick(0.04), rng.integers(0, 3)] = np.nan
    sums[pick(0.02), 1] = np.inf
    sums[pick(0.02), 2] = -np.inf
    features[pick(0.02), rng.integers(0, 8)] = np.nan
    features[pick(0.01), 6] = np.inf
    features[pick(0.03), 0:3] = 0.0
    features[pick(0.02), 1] = 2.0 ** -14
    if H * W == 1:
        counts[:] = spp
    for a in (sums, features, counts):
        a.setflags(write=False)
    return sums, features, counts


def constant(width, height, spp=8, colour=(0.3, 0.5, 0.7), albedo=(0.5, 0.25, 1.0), normal=(0.0, 0.6, 0.8),
             distance=3.0):
    """A constant image over constant guides."""
    H, W = height, width
    sums = np.tile(np.array(colour) * spp, (H, W, 1))
    features = np.tile(np.array([*(np.array(albedo) * spp), *(np.array(normal) * spp), distance * spp, spp]), (H, W, 1))
    return sums, features


class OracleFrame:
    """scenes::simple from its own camera on the CPU oracle alone: the noisy sums
    of `spp` samples (seed 7, chunk 1), the features of exactly those samples
    (feature_cases.Samples: O.trace_path / O.world_hit) and the reference means of
    `ref_spp` samples of seed 8."""

    def __init__(self, width=64, height=36, spp=16, ref_spp=512, depth=50):
        smp = F.Samples("simple", width, height, spp, seed=7)
        _, ocam = F.cameras("simple", width, height, spp, depth)
        _, ocam_ref = F.cameras("simple", width, height, ref_spp, depth)
        sc = O.Scene(**smp.soa.__dict__)
        self.W, self.H, self.spp = width, height, spp
        self.features = smp.fold()
        self.sums, _ = O.render(ocam, sc, 7, chunk=1, accel=O.ACCEL_BVH_CACHED)
        ref, _ = O.render(ocam_ref, sc, 8, chunk=1, accel=O.ACCEL_BVH_CACHED)
        self.ref = ref / ref_spp


@functools.lru_cache(maxsize=None)
def oracle_frame():
    return OracleFrame()


def display_rms(mean, ref, mask):
    """RMS of sqrt(clip(mean, 0, 1)) against the reference's over the masked pixels."""
    with np.errstate(invalid="ignore"):
        a, b = np.sqrt(np.clip(mean[mask], 0, 1)), np.sqrt(np.clip(ref[mask], 0, 1))
    return float(np.sqrt(((a - b) ** 2).mean()))
