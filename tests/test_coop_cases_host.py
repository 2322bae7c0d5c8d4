"""The inputs of tests/test_gpu_coop_probe.py on the CPU (no GPU needed): the
conditions on tests/coop_cases.py that the oracle can check -- the sizes stay
within the probe's limits, the cluster ray hits the whole cluster and the bigs
ray the big list's lights, and the generator is deterministic."""
import numpy as np

import coop_cases as cc
from oracle import oracle as O


def _all_cases():
    cases = [c for c, _ in cc.base_cases()]
    # the boundary cases on a grid like the one the probe reports for the layer
    # (20.4 / 15 cells: the host's box pad does not matter here)
    for c in cases:
        if c.name in cc.BOUNDARY_OF:
            lo = np.array([-10.0, 0.0, -10.0]) + np.asarray(c.shift)
            cases.append(cc.boundary_case(c, {"lo": lo, "cell": np.array([1.36, 0.4, 1.36]), "n": np.array([15, 1, 15])}))
    return cases


def _hits(case, family):
    """per ray of the family: the lights the reference's Sphere::hit hits with t in [0, inf)"""
    ids = np.flatnonzero(case.family == cc.FAMILIES.index(family))
    hit, _ = O.sphere_hit_batch(cc.records(case, ids), 0.0)
    return hit.reshape(len(ids), len(case.lights))


def test_case_sizes_stay_within_the_limits():
    names = set()
    for c in _all_cases():
        names.add(c.name)
        assert 1 <= len(c.lights) <= cc.MAX_LIGHTS, c.name
        assert 1 <= len(c.rays) <= cc.MAX_RAYS and len(c.rays) % 64 == 0, c.name
        assert 1 <= len(c.waves) <= cc.MAX_WAVES, c.name
        assert len(c.family) == len(c.target) == len(c.sampled) == len(c.rays)
        assert ((c.sampled >= -1) & (c.sampled < len(c.lights))).all(), c.name
        for w in c.waves:
            assert w.ray.shape == (64,) and w.pend.shape == (64,) and (w.ray < len(c.rays)).all()
            assert w.P in cc.P_VALUES and w.cap_words % 64 == 0 and w.cap_words <= 1536
    assert {"layer", "cluster", "bigs", "row1", "row2", "row3", "row33", "row2_inf", "degenerate", "shifted", "scaled_up",
            "scaled_down", "layer_boundary", "shifted_boundary"} <= names
    # every pend pattern, every P, both slot sizes and the short one
    layer = cc.layer_case()
    assert {w.kind for w in layer.waves} >= {"main", "perm", "none", "alternating", "lane0", "lane63", "short"}
    assert {w.P for w in layer.waves} == set(cc.P_VALUES)
    assert {w.cap_words for w in layer.waves} == {512, 1536, cc.CAP_SHORT} and cc.CAP_SHORT < cc.CAP_MIN


def test_cluster_ray_hits_the_whole_cluster():
    c = cc.cluster_case()
    assert len(c.cluster) == 12
    hits = _hits(c, "cluster")
    assert hits[0][list(c.cluster)].all() and hits[0].sum() >= 12
    assert (hits.sum(axis=1) >= 9).all()          # the other two: more than an owner's list of 8


def test_bigs_ray_hits_the_big_list():
    c = cc.bigs_case()
    r = np.abs(c.lights[:, 3])
    assert sorted(c.big) == sorted(np.flatnonzero(r > 3.0 * np.median(r)).tolist()) and len(c.big) == 5
    hits = _hits(c, "bigs")
    assert (hits[:, list(c.big)].sum(axis=1) >= 3).all() and hits[0][list(c.big)].sum() >= 4


def test_rays_over_the_grid_hit_the_big_light():
    c = cc.layer_case()
    hits = _hits(c, "miss_grid_hit_big")
    assert hits[:, 400].sum() >= 8 and not hits[:, :400].any()
    ids = np.flatnonzero(c.family == cc.FAMILIES.index("miss_grid_hit_big"))
    assert (c.rays[ids, 1] > 0.4 + 0.5).all() and (c.rays[ids, 4] >= 0).all()      # above the layer, not descending


def test_generator_is_deterministic():
    for a, b in zip(_all_cases(), _all_cases()):
        assert a.name == b.name
        assert np.array_equal(a.lights, b.lights, equal_nan=True) and np.array_equal(a.rays, b.rays, equal_nan=True)
        assert np.array_equal(a.sampled, b.sampled) and np.array_equal(a.family, b.family)
        assert cc.pack(a, cc.DENSITY) == cc.pack(b, cc.DENSITY)
