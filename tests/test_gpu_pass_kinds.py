"""The three kinds of render pass on one context, one after another: the
one-shot render (cold: it counts its tile costs; warm: it takes the ordered
task list), a render in sample windows (tuning "window"), rtw_render_window,
an adaptive render, and the one-shot render again.  The relations between
them are the ones tests/test_gpu_parity.py (a repeated render), test_gpu_windows.py
(windows against the one-shot render) and test_gpu_adaptive.py (each pixel's
sum against the window render of its count; the longest-first cache is left
alone) assert, with their comparisons: "identical" is equal NaN masks and
equal values elsewhere, and an f32 render is the f64 running sums rounded to
f32 once.  40 x 24 is 5 x 3 tiles (the tile rows are no multiple of a
workgroup's waves); spp 8 with lpt_min_spp 8: the one-shot renders take the
longest-first order, the passes of 4 samples do not."""
import numpy as np
import pytest

import ray_tracing_weekend_amd as rtw

pytestmark = pytest.mark.gpu

SEED_SCENE, SEED = 0x5EED0001, 77
W, H, SPP, WIN = 40, 24, 8, 4


def _identical(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _as_rendered(sums, prec):
    return sums if prec == rtw.RTW_F64 else sums.astype(np.float32).astype(np.float64)


def test_every_pass_kind_on_one_context():
    soa, b = rtw.scenes.simple_soa(SEED_SCENE)
    cam = b.with_image_width(W).with_image_height(H).with_samples_per_pixel(SPP).with_max_depth(50).build()
    for prec in (rtw.RTW_F64, rtw.RTW_F32):
        with rtw.Renderer(device=0, precision=prec) as r:
            r.set_tuning("lpt_min_spp", SPP)
            r.set_scene(soa)
            kernels = []
            cold = r.render(cam, SEED)
            kernels.append(r.last_kernel())
            warm = r.render(cam, SEED)
            kernels.append(r.last_kernel())
            assert _identical(cold, warm), prec                      # a repeated render: the first's image
            r.set_tuning("window", WIN)
            windowed = r.render(cam, SEED)
            kernels.append(r.last_kernel())
            r.set_tuning("window", 0)
            assert _identical(windowed, cold), prec                  # tuning "window": the one-shot render
            sums4 = r.render_window(cam, SEED, 0, WIN).copy()
            kernels.append(r.last_kernel())
            sums8 = r.render_window(cam, SEED, WIN, WIN, sums4.copy())
            kernels.append(r.last_kernel())
            assert _identical(_as_rendered(sums8, prec), cold), prec  # windows onto f64 sums: the one-shot render
            costs = r.tile_costs(cam)
            assert costs.shape == (15,)
            sums, counts = r.render_adaptive(cam, SEED, WIN, SPP, WIN, 0.0)
            kernels.append(r.last_kernel())
            assert set(np.unique(counts)) <= {WIN, SPP}
            for n, ref in ((WIN, sums4), (SPP, sums8)):               # each pixel: the window render of its count
                at = counts == n
                assert _identical(sums[at], ref[at]), (prec, n)
            assert np.array_equal(r.tile_costs(cam), costs), prec    # the adaptive path leaves the cache alone
            last = r.render(cam, SEED)
            kernels.append(r.last_kernel())
            assert _identical(last, warm), prec
            assert kernels[0] is not None and all(k == kernels[0] for k in kernels), (prec, kernels)
