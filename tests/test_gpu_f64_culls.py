"""Render-level parity of the f64 kernels on the adversarial scenes of
tests/cull_cases.py: scaled by 2^-40 .. 2^40, translated until an f32 ulp
exceeds the small radii, light queries from 10^4 away, axis-parallel rays,
directions of length 2^-30 and 2^30, a grazing field between huge spheres.

Every pixel must be the brute-force oracle's, bit for bit (exact == 1.0, equal
NaN masks, equal segment and Lambertian counts), under brute force and under
every BVH kind crossed with the three light queries (linear sum, light BVH,
light grid): a false cull by the widened slab test, the leaf pre-pass, the
light pre-pass or the f32 grid walk shows as a wrong pixel here.
"""
import numpy as np
import pytest

import cull_cases as cc
import ray_tracing_weekend_amd as rtw
from oracle import oracle as O
from ray_tracing_weekend_amd import _capi

pytestmark = pytest.mark.gpu

K_BRUTE = (0, 1)
K_BVH_WW = 3
BVH_KIND_KERNEL = {0: 2, 1: 3, 2: 4, 3: 5}      # rtw_stats.kernel of tuning bvh_kind
LIGHT_QUERIES = {"linear": {"light_bvh_min": 1 << 30},
                 "light_bvh": {"light_bvh_min": 1, "light_grid": 0},
                 "light_grid": {"light_bvh_min": 1, "light_grid": 8}}


def _soa(sc: O.Scene) -> rtw.SceneSoA:
    soa = rtw.SceneSoA(spheres=sc.spheres, sphere_mat=sc.sphere_mat, planes=sc.planes, plane_mat=sc.plane_mat,
                       mat_type=sc.mat_type, mat_params=sc.mat_params, lights=sc.lights)
    if sc.mat_tex is not None:
        soa.mat_tex, soa.tex_type, soa.tex_params, soa.tex_refs = sc.mat_tex, sc.tex_type, sc.tex_params, sc.tex_refs
    return soa


def _camera(cam: O.Camera) -> rtw.Camera:
    raw = _capi.rtw_camera()
    for name, _ in O.Camera._fields_:
        setattr(raw, name, getattr(cam, name))
    return rtw.Camera(raw)


def _render(soa, cam, seed, accel, tuning):
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_chunk(1)
        for k, v in tuning.items():
            r.set_tuning(k, v)
        r.set_accel(accel)
        r.set_scene(soa)
        img = r.render(cam, seed)
        return img, r.stats.chunk, r.stats.kernel, (r.stats.segments, r.stats.lambertian)


class _Oracle:
    """the brute-force oracle's render of a case at a chunk, computed once per chunk"""

    def __init__(self, cam, scene, seed):
        self.args, self.at = (cam, scene, seed), {}

    def __call__(self, chunk):
        if chunk not in self.at:
            self.at[chunk] = O.render(*self.args, chunk=chunk, accel=O.ACCEL_BRUTE)
        return self.at[chunk]


def _check(what, got, oracle):
    img, chunk, _, counts = got
    ref, st = oracle(chunk)
    nan_g, nan_r = np.isnan(img).any(-1), np.isnan(ref).any(-1)
    assert np.array_equal(nan_g, nan_r), f"{what}: NaN masks differ: {nan_g.sum()} vs {nan_r.sum()}"
    ok = ~nan_r
    same = (img == ref).all(-1)[ok]
    exact = float(same.mean()) if ok.any() else 1.0
    assert exact == 1.0, f"{what}: {int((~same).sum())} of {int(ok.sum())} pixels differ from the oracle " \
                         f"(first: {np.argwhere(~((img == ref).all(-1) | nan_r))[:4].tolist()})"
    assert counts == (st.segments, st.lambertian), f"{what}: segments, lambertian {counts} vs " \
                                                   f"{(st.segments, st.lambertian)}"


def _configs(case):
    yield "brute", rtw.RTW_ACCEL_BRUTE, {}, None
    for kind in (0, 1, 2, 3):
        for name, t in LIGHT_QUERIES.items():
            yield f"bvh_kind {kind}, {name}", rtw.RTW_ACCEL_BVH, dict(t, bvh_kind=kind), kind
        for g in case.extra_grids:
            yield f"bvh_kind {kind}, light_grid {g}", rtw.RTW_ACCEL_BVH, \
                {"light_bvh_min": 1, "light_grid": g, "bvh_kind": kind}, kind


@pytest.mark.parametrize("name", cc.scene_names())
def test_f64_is_the_oracle_on_adversarial_scene(name):
    case = cc.scene(name)
    soa, cam = _soa(case.scene), _camera(case.cam)
    oracle = _Oracle(case.cam, case.scene, case.seed)
    failures = []
    for what, accel, tuning, kind in _configs(case):
        got = _render(soa, cam, case.seed, accel, tuning)
        if kind is None:
            assert got[2] in K_BRUTE, what
        else:   # bvh_kind 3 falls back to 1 when the tree does not fit in LDS
            assert got[2] == BVH_KIND_KERNEL[kind] or (kind == 3 and got[2] == K_BVH_WW), what
        try:
            _check(f"{name}, {what}", got, oracle)
        except AssertionError as e:      # every configuration is reported, not the first alone
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def test_far_origin_scene_textured_runs_the_per_lane_grid_walk():
    """Identity solid textures: the same pixels through the textured kernels,
    whose light grid walk is the per-lane one."""
    case = cc.scene("far_origin")
    assert case.textured
    sc = cc.with_identity_textures(case.scene)
    soa, cam = _soa(sc), _camera(case.cam)
    ref, st = O.render(case.cam, case.scene, case.seed, chunk=1, accel=O.ACCEL_BRUTE)
    ref_t, _ = O.render(case.cam, sc, case.seed, chunk=1, accel=O.ACCEL_BRUTE)
    oracle = _Oracle(case.cam, sc, case.seed)
    assert np.array_equal(np.nan_to_num(ref, nan=-7.0), np.nan_to_num(ref_t, nan=-7.0))
    failures = []
    for kind in (0, 2, 3):
        for g in (1, 8, 256):
            got = _render(soa, cam, case.seed, rtw.RTW_ACCEL_BVH,
                          {"bvh_kind": kind, "light_bvh_min": 1, "light_grid": g, "bvh_lds_max": 64 * 1024})
            assert got[2] in (3, 5)      # textured scenes run the while-while kernels
            try:
                _check(f"far_origin textured, bvh_kind {kind}, light_grid {g}", got, oracle)
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "\n".join(failures)
