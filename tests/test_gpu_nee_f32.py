"""The any-hit and light-sample queries in f32 (the speed mode's arithmetic).

Occlusion: the per-primitive t is the f32 closest-hit query's, so "occluded
within t_max" is an identity with "hit_rays of the same context found a hit
with t32 <= t_max" at t_max = t32 and just below it -- asserted exactly.
Against the f64 truth at t / 2 and 2 t the share of differing rays is held to
the 1 % cap of test_f32_query_against_f64_on_camera_rays.

Light sample: the list index is an integer draw and equals f64's exactly; the
fused pdf is the f32 light pdf of {origin, direction} bit for bit.  The values
-- t and the whole hit record behind the occlusion identity, the directions and
the pdf -- are held row by row to the law of the f32 forms in
tests/test_gpu_f32_records.py (test_hit_records, test_light_sample)."""
import numpy as np
import pytest

import nee_cases as N
import query_cases as Q
import ray_tracing_weekend_amd as rtw

pytestmark = pytest.mark.gpu


def test_f32_occlusion_is_the_f32_closest_hit_within_the_range():
    soa, _ = Q.scene("simple")
    rays64 = Q.camera_rays("simple", 120, 80)
    rays = rays64.astype(np.float32)
    with rtw.Renderer(device=0, precision=rtw.RTW_F32) as r:
        r.set_scene(soa)
        h32, i32 = r.hit_rays(rays)
        assert r.get_query_stats().kernel == 5
        hit = i32[:, 0] >= 0
        assert hit.sum() > 1000 and (~hit).sum() > 1000
        t32 = np.where(hit, h32[:, 0], np.float32(1.0)).astype(np.float32)
        at = r.occluded(rays, t32)
        st = r.get_query_stats()
        below = r.occluded(rays, np.nextafter(t32, np.float32(-np.inf)))
        inf = r.occluded(rays)
        assert at.dtype == np.uint8 and (st.kernel, st.is_light_pdf, st.rays, st.hits) == (5, 2, len(rays), int(hit.sum()))
        assert np.array_equal(at, hit.astype(np.uint8))        # t32 <= t_max at t_max = t32 ...
        assert not below.any()                                   # ... and nothing nearer than the closest hit
        assert np.array_equal(inf, hit.astype(np.uint8))
        # every traversal and both test forms answer alike at t_max = t32 of their own closest hit
        half, twice = r.occluded(rays, t32 / 2), r.occluded(rays, 2 * t32)
    for accel, tuning in ((rtw.RTW_ACCEL_BRUTE, {"lds": 1}), (rtw.RTW_ACCEL_BRUTE, {"lds": 0}),
                          (rtw.RTW_ACCEL_BVH, {"bvh_kind": 0}), (rtw.RTW_ACCEL_BVH, {"bvh_kind": 1}),
                          (rtw.RTW_ACCEL_BVH, {"bvh_kind": 2}), (rtw.RTW_ACCEL_BVH, {"bvh_kind": 3, "robust": 1})):
        with rtw.Renderer(device=0, precision=rtw.RTW_F32) as r:
            for k, v in tuning.items():
                r.set_tuning(k, v)
            r.set_accel(accel)
            r.set_scene(soa)
            h, i = r.hit_rays(rays)
            t = np.where(i[:, 0] >= 0, h[:, 0], np.float32(1.0)).astype(np.float32)
            assert np.array_equal(r.occluded(rays, t), (i[:, 0] >= 0).astype(np.uint8)), tuning
            assert not r.occluded(rays, np.nextafter(t, np.float32(-np.inf))).any(), tuning
    # against the f64 truth
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        h64, i64 = r.hit_rays(rays64)
        t64 = np.where(i64[:, 0] >= 0, h64[:, 0], 1.0)
        half64, twice64 = r.occluded(rays64, t64 / 2), r.occluded(rays64, 2 * t64)
    assert not half64.any() and np.array_equal(twice64, (i64[:, 0] >= 0).astype(np.uint8))
    for what, a, b in (("t / 2", half, half64), ("2 t", twice, twice64)):
        share = float((a != b).mean())
        print(f"f32 vs f64 occlusion at t_max = {what} on {len(rays)} camera rays: {int((a != b).sum())} differ "
              f"({100 * share:.4f} %)")
        assert share <= 0.01


def test_f32_light_sample_indices_and_fused_pdf():
    soa, pts = N.bounce_points("simple")
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        d64, _, l64 = r.light_sample(pts, 7, 1000, 3)
    with rtw.Renderer(device=0, precision=rtw.RTW_F32) as r:
        r.set_scene(soa)
        d, p, light = r.light_sample(pts, 7, 1000, 3)           # f64 numpy input is converted
        st = r.get_query_stats()
        assert d.dtype == np.float32 and d.shape == (len(pts), 3) and p.dtype == np.float32 and p.shape == (len(pts),)
        assert light.dtype == np.int32 and np.array_equal(light, l64)
        assert (st.kernel, st.is_light_pdf, st.rays) == (0, 3, len(pts))
        alone = r.light_pdf(np.concatenate([pts.astype(np.float32), d], 1))
        assert np.array_equal(p, alone, equal_nan=True) and (p > 0).any()
        dn, pn, ln = r.light_sample(pts, 7, 1000, 3, pdf=False)
        assert pn is None and np.array_equal(dn, d, equal_nan=True) and np.array_equal(ln, light)
    dev = np.abs(d - d64).max()
    print(f"f32 light-sample directions: largest deviation from f64 on {len(pts)} origins {dev:.3e}")
    assert np.isfinite(d).all()
