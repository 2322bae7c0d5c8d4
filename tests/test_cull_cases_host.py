"""The adversarial cull cases (tests/cull_cases.py) against the CPU oracle alone
(no GPU): the conditions that keep the GPU tests honest.  A family in which the
oracle hits nothing cannot show a false cull, and a scene that renders only
background, or whose far-origin bounces never reach a light, exercises no
filter."""
import numpy as np
import pytest

import cull_cases as cc
from oracle import oracle as O


def test_record_families_hit_and_miss():
    R = cc.records()
    assert np.isfinite(R.rec).all() and len(R.rec) <= 1 << 20
    hit, _ = O.sphere_hit_batch(R.rec)
    for fi, fam in enumerate(cc.FAMILIES):
        m = R.family == fi
        assert m.sum() > 500
        share = hit[m].mean()
        print(f"{fam}: {m.sum()} records, {share:.3f} hit")
        if fam in cc.CONTROLS:
            continue
        assert 0.25 <= share <= 0.75, (fam, share)
    # the extreme magnitudes as a family of their own
    m = (R.tier == 2) & ~np.isin(R.family, [cc.FAMILIES.index(f) for f in cc.CONTROLS])
    assert m.sum() > 5000 and 0.25 <= hit[m].mean() <= 0.75
    # the controls control: clear misses miss, clear hits hit a light query (t_min = 0)
    hit0, _ = O.sphere_hit_batch(R.rec, 0.0)
    assert not hit[R.family == cc.FAMILIES.index("clear_miss")].any()
    assert hit0[R.family == cc.FAMILIES.index("clear_hit")].all()
    # every scale of the sweep is there, in both tiers
    assert set(np.unique(R.k)) == set(cc.K_TIER1 + cc.K_TIER2)
    assert (R.tier == 1).sum() > 10000 and (R.tier == 2).sum() > 10000


def test_axis_records_have_exact_zeros():
    R = cc.records()
    m = R.family == cc.FAMILIES.index("axis")
    d, o = R.rec[m, 3:6], R.rec[m, 0:3]
    zeros = d == 0.0
    assert (zeros.sum(1) >= 1).all() and (zeros.sum(1) == 2).any()
    assert (o[zeros] == 0.0).all()
    assert np.signbit(d[zeros]).any() and not np.signbit(d[zeros]).all()


def test_box_records_hit_and_miss():
    B, fam, _ = cc.box_records()
    hit = O.aabb_hit_batch(B)
    assert hit[fam == 0].mean() > 0.9            # o on a face
    for f in (1, 2, 3):
        assert 0.25 <= hit[fam == f].mean() <= 0.75, f


@pytest.mark.parametrize("name", cc.scene_names())
def test_scene_is_not_vacuous(name):
    c = cc.scene(name)
    img, st = O.render(c.cam, c.scene, c.seed, chunk=1, accel=O.ACCEL_BRUTE)   # raises on a reference panic
    assert st.panic_plane_uv == 0 and st.panic_no_lights == 0
    assert st.lambertian > 0
    bg = np.array(c.cam.background[:]) * c.cam.samples_per_pixel
    differs = np.isnan(img).any(-1) | (img != bg).any(-1)
    assert differs.mean() >= 0.25
    assert c.cam.image_width <= 32 and c.cam.image_height <= 24
    assert c.cam.samples_per_pixel <= 4 and c.cam.max_depth <= 12


def _paths(c):
    for j in range(c.cam.image_height):
        for i in range(c.cam.image_width):
            for s in range(c.cam.samples_per_pixel):
                yield O.trace_path(c.cam, c.scene, c.seed, i, j, s)[1]


def test_far_origin_scene_queries_lights_from_far_away():
    c = cc.scene("far_origin")
    assert len(c.scene.lights) >= 64
    ids = cc.light_sphere_ids(c.scene)
    n = 0
    for path in _paths(c):
        far = np.linalg.norm(path[:, :3], axis=1) > 1e4
        n += int((far & np.isin(path[:, 6].astype(np.int64), list(ids))).sum())
    assert n >= 500, n


@pytest.mark.parametrize("name", ["axis_parallel", "axis_one_zero", "axis_one_zero_offset"])
def test_axis_scene_hits_and_bounces(name):
    c = cc.scene(name)
    base = len(c.scene.plane_mat)
    sphere_hits = bounces = 0
    for path in _paths(c):
        d0, o0 = path[0, 3:6], path[0, 0:3]
        zero = d0 == 0.0
        assert zero.sum() == (2 if name == "axis_parallel" else 1)
        # the origin's matching components are 0 too (0 x inf = NaN in the slab
        # test), except in the offset variant (0.3 x inf = inf)
        assert (o0[zero] == (0.3 if name == "axis_one_zero_offset" else 0.0)).all()
        sphere_hits += int((path[:, 6] >= base).sum())
        bounces += len(path) - 1
    assert sphere_hits >= 1 and bounces >= 1


def test_base_scene_shape():
    c = cc.scene("base")
    assert 55 <= len(c.scene.sphere_mat) <= 65 and len(c.scene.plane_mat) == 0
    used = set(c.scene.mat_type[c.scene.sphere_mat].tolist())
    assert {O.LAMBERTIAN, O.METAL, O.DIELECTRIC} <= used
    assert len(c.scene.lights) >= 64 and len(cc.scene("base_5_lights").scene.lights) == 5
    assert c.scene.spheres[:, 3].max() >= 1000.0      # the ground is a sphere
    t = cc.scene("translated_2^22").scene
    assert np.spacing(np.float32(2.0 ** 22)) > np.sort(t.spheres[:, 3])[:10].max()   # f32 ulp above the small radii
