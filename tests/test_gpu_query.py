"""The batched closest-hit query (rtw_hit_rays) on the GPU against the oracle
and the independent restatement (tests/query_cases.py): path segments of the
oracle's own paths, UVs, every traversal, ray counts around the wave and
workgroup sizes, adversarial rays.  All f64 comparisons are bit for bit with
equal NaN masks; the expected values never come from the GPU."""
import math

import numpy as np
import pytest

import cull_cases as cc
import query_cases as Q
import ray_tracing_weekend_amd as rtw
from indep import restate as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EPS = Q.EPS
WORLD_OF_KIND = {0: 2, 1: 3, 2: 4, 3: 5}      # rtw_query_stats.kernel of tuning bvh_kind


def query(soa, rays, t_min=EPS, precision=rtw.RTW_F64, accel=rtw.RTW_ACCEL_AUTO, **tuning):
    """(hits, ids, query stats) of one query on a fresh context."""
    with rtw.Renderer(device=0, precision=precision) as r:
        for k, v in tuning.items():
            r.set_tuning(k, v)
        r.set_accel(accel)
        r.set_scene(soa)
        hits, ids = r.hit_rays(rays, t_min)
        st = r.get_query_stats() if len(rays) else None
        return hits, ids, st


def same(a, b):
    """bit for bit up to the sign of zero, NaN masks equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def expect_records(seg):
    """(hits[:, :7], ids) the oracle's segments ask for; a miss: -1 and zeros"""
    hit = seg.ids >= 0
    ids = np.zeros((len(seg.ids), 4), np.int32)
    ids[:, 0] = seg.ids
    ids[hit, 1] = seg.mat[seg.ids[hit]]
    ids[hit, 2] = seg.front[hit]
    ids[hit, 3] = seg.kind[seg.ids[hit]]
    return seg.hits[:, :7], ids


# ------------------------------------------------------------ a. path segments
@pytest.mark.parametrize("name,worlds", [("simple", (5,)), ("simple63", (0, 1)), ("cornell_box", (0, 1)),
                                         ("simple_transform", (0, 1)), ("simple_light", (0, 1)), ("plane", (0, 1)),
                                         ("checkered_spheres", (0, 1))])
def test_oracle_path_segments(name, worlds):
    seg = Q.segments(name)
    # the oracle alone: world_hit answers every segment as trace_path met it
    assert np.array_equal(seg.wid, seg.ids)
    assert np.array_equal(seg.hits[seg.ids >= 0, 0], seg.t[seg.ids >= 0])
    if name in ("simple", "simple63"):      # the sample is not vacuous
        assert seg.rehits >= 100 and seg.misses >= 100, (seg.rehits, seg.misses)
    hits, ids, st = query(seg.soa, seg.rays)
    assert st.kernel in worlds and st.is_light_pdf == 0
    want_hits, want_ids = expect_records(seg)
    assert np.array_equal(ids[:, 0], want_ids[:, 0]), np.flatnonzero(ids[:, 0] != want_ids[:, 0])[:8]
    assert same(hits[:, 0], want_hits[:, 0])                      # t
    assert same(hits[:, 1:4], want_hits[:, 1:4])                  # p
    assert same(hits[:, 4:7], want_hits[:, 4:7])                  # normal, front-face adjusted
    assert np.array_equal(ids, want_ids)                          # material, front face, kind
    miss = seg.ids < 0
    assert not hits[miss].any() and np.array_equal(ids[miss], np.tile([-1, 0, 0, 0], (miss.sum(), 1)))
    assert (st.rays, st.hits) == (len(seg.rays), int((~miss).sum()))
    if 5 in worlds:
        assert st.node_visits > 0 and st.sphere_tests > 0
    else:
        assert st.node_visits == 0 and st.sphere_tests == len(seg.rays) * len(seg.soa.spheres)


# ------------------------------------------------------------------- b. UVs
# The sphere UV is atan2(-n.z, n.x) / 2 pi and acos(n.y) / pi of the same f64
# normal on both sides (the normal is checked bit for bit above).  The device
# math library follows the OpenCL limits for double: atan2 <= 6 ulp, acos <= 4
# ulp; the restatement's libm is within 1 ulp.  The two angles therefore differ
# by at most 7 (5) ulp of the angle, and the correctly rounded division by 2 pi
# (pi) adds half an ulp of the quotient on each side.
ATAN2_ULP, ACOS_ULP = 6 + 1, 4 + 1


def _tilted_plane_scene():
    grey = rtw.Lambertian((0.5, 0.5, 0.5))
    world = rtw.HittableList([rtw.Plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), grey),
                              rtw.Plane((1.0, -2.0, 0.5), (0.3, 1.0, -0.2), grey)])
    return rtw.flatten(world, rtw.HittableList())


def _restate_hits(soa, rays):
    w = R.World(soa)
    out = []
    for r in rays:
        rec = w.hit(tuple(r[:3]), tuple(r[3:]))
        out.append((np.nan, np.nan, np.nan) if rec is None else (rec.t, rec.u, rec.v))
    return np.array(out)


def test_plane_quad_and_cuboid_uvs_are_exact():
    # planes are one-sided: rays from below, moving along +n
    rng = np.random.default_rng(11)
    n = 200
    o = np.stack([rng.uniform(-5, 5, n), rng.uniform(-9, -4, n), rng.uniform(-5, 5, n)], 1)
    d = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(0.5, 1.5, n), rng.uniform(-0.4, 0.4, n)], 1)
    # (the tilted plane passes y in [-2.5, -1.5] above the last 50 origins' x, z: they start
    # between the planes and meet the level one)
    o[-50:] = np.stack([1.0 + rng.uniform(-1, 1, 50), np.full(50, -0.5), 0.5 + rng.uniform(-1, 1, 50)], 1)
    rays = np.ascontiguousarray(np.concatenate([o, d], 1))
    soa = _tilted_plane_scene()
    want = _restate_hits(soa, rays)
    hits, ids, _ = query(soa, rays)
    assert np.isfinite(want[:, 0]).all() and set(ids[:, 0]) == {0, 1} and (ids[:, 3] == 0).all()
    assert same(hits[:, 0], want[:, 0]) and same(hits[:, 7:9], want[:, 1:3])
    # quads and the cuboid of cornell_box, on the oracle's path segments
    seg = Q.segments("cornell_box")
    uv = seg.uv()
    hits, ids, _ = query(seg.soa, seg.rays)
    flat = np.isin(ids[:, 3], (1, 2))
    assert (ids[:, 3] == 1).sum() >= 50 and (ids[:, 3] == 2).sum() >= 10
    assert same(hits[flat, 7:9], uv[flat, :2])


@pytest.mark.parametrize("name", ["simple", "checkered_spheres"])
def test_sphere_uvs_within_the_math_library_bound(name):
    seg = Q.segments(name)
    uv = seg.uv()
    hits, ids, _ = query(seg.soa, seg.rays)
    sph = ids[:, 3] == 3
    assert sph.sum() >= 100
    u, v, a, c = uv[sph, 0], uv[sph, 1], uv[sph, 2], uv[sph, 3]
    bound_u = ATAN2_ULP * np.spacing(np.abs(a)) / (2 * math.pi) + np.spacing(np.abs(u))
    bound_v = ACOS_ULP * np.spacing(np.abs(c)) / math.pi + np.spacing(np.abs(v))
    du, dv = np.abs(hits[sph, 7] - u), np.abs(hits[sph, 8] - v)
    print(f"{name}: {int(sph.sum())} sphere hits, u differs on {int((du > 0).sum())}, v on {int((dv > 0).sum())}; "
          f"largest |du| / bound {float((du / bound_u).max()):.3f}, |dv| / bound {float((dv / bound_v).max()):.3f}")
    assert np.isfinite(hits[sph, 7:9]).all()
    assert (du <= bound_u).all(), int((du > bound_u).sum())
    assert (dv <= bound_v).all(), int((dv > bound_v).sum())


# -------------------------------------------------------- c. every traversal
def _simple_rays():
    seg = Q.segments("simple")
    return np.ascontiguousarray(np.concatenate([seg.rays, Q.camera_rays("simple", 60, 40)]))


@pytest.mark.parametrize("precision", [rtw.RTW_F64, rtw.RTW_F32], ids=["f64", "f32"])
def test_every_traversal_gives_the_brute_force_records(precision):
    soa, _ = Q.scene("simple")
    rays = _simple_rays().astype(np.float32 if precision == rtw.RTW_F32 else np.float64)
    ref_h, ref_i, st = query(soa, rays, precision=precision, accel=rtw.RTW_ACCEL_BRUTE, lds=1)
    assert st.kernel == 1
    assert (ref_i[:, 0] >= 0).sum() > 500 and (ref_i[:, 0] < 0).sum() > 500
    if precision == rtw.RTW_F64:      # the brute-force query itself is the oracle's
        seg = Q.segments("simple")
        assert np.array_equal(ref_i[:len(seg.ids), 0], seg.ids)
    configs = [("brute, lds 0", rtw.RTW_ACCEL_BRUTE, {"lds": 0}, 0)]
    for kind in (0, 1, 2, 3):
        for lds in (0, 1):
            configs.append((f"bvh_kind {kind}, lds {lds}", rtw.RTW_ACCEL_BVH, {"bvh_kind": kind, "lds": lds},
                            WORLD_OF_KIND[kind]))
    configs.append(("bvh_kind 3, bvh_lds_max 1", rtw.RTW_ACCEL_BVH, {"bvh_kind": 3, "bvh_lds_max": 1}, 3))
    failures = []
    for what, accel, tuning, world in configs:
        h, i, st = query(soa, rays, precision=precision, accel=accel, **tuning)
        if st.kernel != world:
            failures.append(f"{what}: ran world {st.kernel}, not {world}")
        if not (np.array_equal(i, ref_i) and same(h, ref_h)):
            bad = np.flatnonzero((i != ref_i).any(1) | ~((h == ref_h) | (np.isnan(h) & np.isnan(ref_h))).all(1))
            failures.append(f"{what}: {len(bad)} records differ from brute force, first rays {bad[:6].tolist()}")
        if world >= 2 and not (st.node_visits > 0 and st.sphere_tests > 0):
            failures.append(f"{what}: no traversal work counted")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ d. shapes
def test_ray_counts_around_the_wave_and_workgroup_sizes():
    soa, _ = Q.scene("simple")
    rays = _simple_rays()[:1000]
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(soa)
        full_h, full_i = r.hit_rays(rays)
        assert r.get_query_stats().kernel == 5
        seg = Q.segments("simple")
        assert np.array_equal(full_i[:len(seg.ids), 0], seg.ids[:1000])
        for n in (0, 1, 63, 64, 65, 257, 1000):
            h, i = r.hit_rays(rays[:n])
            assert h.shape == (n, 9) and i.shape == (n, 4)
            assert same(h, full_h[:n]) and np.array_equal(i, full_i[:n]), n
            if n:
                assert r.get_query_stats().rays == n


# --------------------------------------------------------- e. adversarial rays
def _oracle_records(sc, rays):
    ids, t = [], []
    for r in rays:
        k, tt, _, _, _ = O.world_hit(sc, r[:3], r[3:])
        ids.append(k)
        t.append(tt if k >= 0 else 0.0)
    return np.array(ids), np.array(t)


def _both_worlds(soa, rays, t_min=EPS):
    """the query through the brute-force sweep and through the stealing traversal"""
    out = []
    for accel, world in ((rtw.RTW_ACCEL_BRUTE, 1), (rtw.RTW_ACCEL_BVH, 5)):
        h, i, st = query(soa, rays, t_min, accel=accel)
        assert st.kernel == world
        out.append((h, i))
    return out


def test_degenerate_directions_and_nan_rays():
    case = cc.scene("axis_one_zero_offset")
    sc = case.scene
    soa = rtw.SceneSoA(spheres=sc.spheres, sphere_mat=sc.sphere_mat, planes=sc.planes, plane_mat=sc.plane_mat,
                       mat_type=sc.mat_type, mat_params=sc.mat_params, lights=sc.lights)
    nan = float("nan")
    rays = [[0.3, y, 5.0, 0.0, dy, -4.0] for y in (0.0, 0.25, -0.5) for dy in (0.0, 0.1, -0.3, 1e-9)]   # d.x = 0, o.x = 0.3
    rays += [[0.3, 0.0, 5.0, 0.0, 0.0, -4.0], [0.0, 0.0, 5.0, 0.0, 0.0, -1.0], [0.0, 0.0, 5.0, 0.0, 0.0, 1.0]]
    rays += [[0.3, 0.0, 5.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]                           # the zero direction
    rays += [[nan, 0.0, 5.0, 0.0, 0.0, -1.0], [0.0, 0.0, 5.0, nan, 0.0, -1.0], [0.0, 0.0, 5.0, 0.0, 0.0, nan],
             [nan] * 6]
    rays += [[0.0, 0.0, 0.2, 0.3, 0.1, 1.0], [1.0, 0.0, 2.5, -1.0, 0.2, 0.1]]                          # origins inside a sphere
    rays = np.array(rays, np.float64)
    want_id, want_t = _oracle_records(sc, rays)
    assert (want_id[-6:-2] == -1).all() and (want_id[-8:-6] == -1).all()      # NaN and zero directions miss
    assert (want_id[:12] >= 0).sum() >= 6 and (want_id[-2:] >= 0).all()
    for h, i in _both_worlds(soa, rays):
        assert np.array_equal(i[:, 0], want_id) and same(h[:, 0], want_t)
        assert not h[want_id < 0].any() and not i[want_id < 0, 1:].any()


def test_negative_radius_and_coincident_spheres():
    grey, red = rtw.Lambertian((0.5, 0.5, 0.5)), rtw.Metal((0.9, 0.1, 0.1), 0.0)
    world = rtw.HittableList([rtw.Sphere((0.0, 0.0, 0.0), -1.0, grey),       # id 0: never hit
                              rtw.Sphere((3.0, 0.0, 0.0), 1.0, grey),        # ids 1, 2: coincident
                              rtw.Sphere((3.0, 0.0, 0.0), 1.0, red),
                              rtw.Sphere((0.0, 0.0, -4.0), 1.0, red)])       # id 3: behind the negative sphere
    soa = rtw.flatten(world, rtw.HittableList())
    sc = O.Scene(**soa.__dict__)
    rays = np.array([[0.0, 0.0, 5.0, 0.0, 0.0, -1.0],      # through the negative sphere to id 3
                     [0.0, 0.0, 0.0, 0.0, 0.0, -1.0],      # from its centre
                     [0.0, 0.0, 5.0, 0.01, 0.02, -1.0],
                     [3.0, 0.0, 5.0, 0.0, 0.0, -1.0],      # the coincident pair, from outside
                     [3.0, 0.0, 0.0, 0.3, 0.2, -1.0],      # ... from inside
                     [-3.0, 0.5, 0.0, 1.0, -0.1, 0.0]])    # through the negative sphere to the pair
    want_id, want_t = _oracle_records(sc, rays)
    assert 0 not in want_id and list(want_id[3:]) == [1, 1, 1] and list(want_id[:3]) == [3, 3, 3]
    for h, i in _both_worlds(soa, rays):
        assert np.array_equal(i[:, 0], want_id) and same(h[:, 0], want_t)
        assert list(i[3:, 1]) == [1, 1, 1]                  # the material of the lower id


def _restate_closest(world, o, d, t_min):
    """hittable_list.rs hit over t_min..=INFINITY: bounded_hit of every object, first minimum"""
    best, best_id = None, -1
    for k, ob in enumerate(world.objects):
        if not ob.aabb.is_hit(o, d, t_min, R.INF):
            continue
        rec = ob.hit(o, d, t_min, R.INF)
        if rec is not None and (best is None or rec.t < best.t):
            best, best_id = rec, k
    return best_id, (best.t if best is not None else 0.0)


def test_t_min_zero_against_epsilon_on_rehit_rays():
    seg = Q.segments("simple")
    rehit = (seg.ids >= 0) & (seg.ids == seg.prev)
    rays = np.ascontiguousarray(seg.rays[rehit])
    assert len(rays) >= 100
    world = R.World(seg.soa)
    differ = 0
    for t_min in (0.0, EPS):
        want = [_restate_closest(world, tuple(r[:3]), tuple(r[3:]), t_min) for r in rays]
        want_id, want_t = np.array([w[0] for w in want]), np.array([w[1] for w in want])
        if t_min == EPS:
            assert np.array_equal(want_id, seg.ids[rehit]) and same(want_t, seg.t[rehit])
            differ = int((want_t != t0).sum())
        t0 = want_t
        for h, i in _both_worlds(seg.soa, rays, t_min):
            assert np.array_equal(i[:, 0], want_id), t_min
            assert same(h[:, 0], want_t), t_min
    print(f"{len(rays)} re-hit rays, t differs between t_min 0 and EPSILON on {differ}")
