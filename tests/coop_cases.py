"""Inputs of tests/native/coop_probe.hip (tests/test_gpu_coop_probe.py): small
adversarial light sets, rays, and the waves -- which ray sits in which lane,
which lanes are pending, the piece length P and the LDS words of the slots --
that the wave-cooperative light-grid walks of light_pdf.hpp are run on.

Everything is deterministic (numpy default_rng with fixed seeds) and small: at
most MAX_LIGHTS lights, MAX_RAYS rays and MAX_WAVES waves per case.

A case is a Case: lights (n, 4) f64 {c, r}; rays (m, 6) f64 {o, d} with m a
multiple of 64; family (m,) the ray's family (FAMILIES); target (m,) the light a
ray was aimed at (-1: none); sampled (m,) the light handed to
lights_pdf_sum_pk's `sampled` (-1: none); waves, a list of Wave; `big` the ids
the set places in the grid's big list by construction; `cluster` the ids of the
one-cell cluster.
"""
from dataclasses import dataclass, field

import numpy as np

MAX_LIGHTS, MAX_RAYS, MAX_WAVES = 512, 4096, 64
P_VALUES = (1, 3, 16, 1 << 20)
# cells per light: the render plan's default (RenderKnobs::light_grid = 8, in
# sixteenths), and once each 1/16 and 16
DENSITY = 0.5
DENSITIES = (0.5, 1.0 / 16.0, 16.0)
CAP_MIN = 512                      # one round of 64 pieces (kCoop64Slot = 8 words each)
CAP_WORDS = (512, 1536)
CAP_SHORT = 448                    # < 512: the f64 walk returns NaN (pending) / 0 at once

FAMILIES = ("skim", "vertical", "inside_grid", "inside_light", "axis", "miss_grid_hit_big", "miss_all",
            "scaled_dir", "nan", "cluster", "bigs", "row", "tangent", "pad")
R0 = 0.2                            # the layer's radius


@dataclass
class Wave:
    P: int
    cap_words: int
    ray: np.ndarray                # (64,) ray indices
    pend: np.ndarray               # (64,) 0 / 1
    kind: str = "main"             # "main", "perm" (the same rays, other lanes), or a pend pattern


@dataclass
class Case:
    name: str
    lights: np.ndarray
    rays: np.ndarray
    family: np.ndarray
    target: np.ndarray
    sampled: np.ndarray
    waves: list
    big: tuple = ()
    cluster: tuple = ()
    scale: float = 1.0
    shift: tuple = (0.0, 0.0, 0.0)
    extra: dict = field(default_factory=dict)


# ---- light sets (base coordinates: the layer spans x, z in [-10, 10] at y = 0.2)
def layer_lights(seed=1):
    """~400 lights of r = 0.2 on a jittered lattice at y = 0.2, plus one r = 1:
    the shape of the 50 000-light scene"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(20), np.arange(20), indexing="ij")
    x = i.ravel() - 9.5 + rng.uniform(-0.25, 0.25, 400)
    z = j.ravel() - 9.5 + rng.uniform(-0.25, 0.25, 400)
    L = np.stack([x, np.full(400, R0), z, np.full(400, R0)], axis=1)
    return np.concatenate([L, [[0.3, 1.0, -0.4, 1.0]]])      # id 400: the one big light


def _shuffle_in(base, extra, seed):
    """`extra` dealt into `base` at fixed random list positions; returns the
    list and the ids of the extras"""
    rng = np.random.default_rng(seed)
    n = len(base) + len(extra)
    pos = np.sort(rng.choice(n, len(extra), replace=False))
    out = np.empty((n, 4))
    mask = np.zeros(n, bool)
    mask[pos] = True
    out[mask] = extra
    out[~mask] = base
    return out, tuple(int(p) for p in pos)


def cluster_lights():
    """the layer plus 12 lights of r = 0.3 whose centres are 0.05 apart along x
    (every one holds x in [2.25, 2.3]: one cell lists all 12)"""
    ex = np.array([[2.0 + 0.05 * k, R0, 1.0, 0.3] for k in range(12)])
    return _shuffle_in(layer_lights(), ex, 2)


def bigs_lights():
    """the layer plus 4 nested lights larger than 3 x the median radius"""
    ex = np.array([[3.0, 0.3, -4.0, r] for r in (0.7, 0.9, 1.1, 1.3)])
    return _shuffle_in(layer_lights(), ex, 3)


def row_lights(n):
    """n lights in a row along x: lights_pdf_sum_pk's tail (odd n) and its
    32-light block boundary (n = 33)"""
    return np.array([[0.5 * k, R0, 0.0, R0] for k in range(n)], float)


def degenerate_lights():
    """a 10 x 10 piece of the layer with lights of zero, negative and NaN
    radius and coincident centres (same and different radii) dealt in (an
    infinite radius: row_case(2, inf_radius=True))"""
    L = layer_lights()[:400].reshape(20, 20, 4)[5:15, 5:15].reshape(-1, 4)
    ex = np.array([[0.1, R0, 0.2, 0.0], [1.1, R0, 0.15, -R0], [-1.2, R0, 2.1, -0.15], [2.2, R0, -1.1, np.nan],
                   [-2.1, R0, -2.2, R0], [-2.1, R0, -2.2, R0], [3.1, R0, 3.2, R0], [3.1, R0, 3.2, 0.1],
                   [-3.2, R0, 1.1, 0.0]])
    return _shuffle_in(L, ex, 4)


# ---- rays
class _Rays:
    def __init__(self):
        self.o, self.d, self.fam, self.tgt = [], [], [], []

    def add(self, fam, o, d, target=-1):
        self.o.append(np.asarray(o, float))
        self.d.append(np.asarray(d, float))
        self.fam.append(FAMILIES.index(fam))
        self.tgt.append(int(target))

    def done(self, scale, shift):
        while len(self.o) % 64:                       # whole waves: rays that miss everything
            self.add("pad", (0.0, 50.0 + len(self.o), 0.0), (0.1, 1.0, 0.2))
        o = np.array(self.o) * scale + np.asarray(shift, float)
        d = np.array(self.d) * scale
        nan = np.array(self.fam) == FAMILIES.index("nan")
        o[nan] = np.nan
        return np.concatenate([o, d], axis=1), np.array(self.fam, np.int32), np.array(self.tgt, np.int32)


def _layer_rays(R, L, rng, finite_small, n_skim=96):
    """the ray families over a layer-like set L (base coordinates);
    finite_small: ids of the plain r = 0.2 lights"""
    ids = np.asarray(finite_small)
    for k in range(n_skim):                           # skimming the layer: ~10 lights, > 100 cells at 16 cells per light
        t = int(ids[rng.integers(len(ids))])
        side = k % 4
        u = rng.uniform(-9.0, 9.0)
        o = [(-11.0, 0.0, u), (11.0, 0.0, u), (u, 0.0, -11.0), (u, 0.0, 11.0)][side]
        o = np.array([o[0], R0 + rng.uniform(-0.05, 0.05), o[2]])
        c = L[t, :3] + np.array([rng.uniform(-0.1, 0.1), 0.0, rng.uniform(-0.1, 0.1)])
        R.add("skim", o, c - o, t)
    for k in range(32):                               # vertical: one cell
        t = int(ids[rng.integers(len(ids))])
        off = rng.uniform(-0.3, 0.3, 2)
        R.add("vertical", (L[t, 0] + off[0], 5.0, L[t, 2] + off[1]), (0.0, -1.0, 0.0), t)
    finite = np.isfinite(L).all(axis=1)

    def in_a_light(o, slack):                         # (an f32 pdf term of a ray that starts inside a light is NaN)
        return bool((finite & (np.linalg.norm(L[:, :3] - o, axis=1) < np.abs(L[:, 3]) + slack)).any())

    k = 0
    while k < 48:                                     # starting inside the grid, outside every light
        o = np.array([rng.uniform(-8, 8), R0 + rng.uniform(-0.1, 0.1), rng.uniform(-8, 8)])
        a = rng.uniform(0, 2 * np.pi)
        if in_a_light(o, 0.05):
            continue
        R.add("inside_grid", o, (np.cos(a), rng.uniform(-0.02, 0.02), np.sin(a)))
        k += 1
    # starting inside one light and no other, leaving upward and away from the large ones: m <= 2
    alone = [int(t) for t in ids
             if (finite & (np.linalg.norm(L[:, [0, 2]] - L[t, [0, 2]], axis=1) < np.abs(L[:, 3]) + 0.3)).sum() == 1]
    for k in range(16):
        t = alone[int(rng.integers(len(alone)))]
        R.add("inside_light", L[t, :3] + rng.uniform(-0.05, 0.05, 3), (0.01 * (k % 3), 1.0, 0.02 * (k % 2)), t)
    for k in range(24):                               # axis-parallel: one or two zero direction components
        row = rng.integers(20) - 9.5
        y = R0 + rng.uniform(-0.1, 0.1)
        o, d = [((-10.5, y, row), (1.0, 0.0, 0.0)), ((row, y, 10.5), (0.0, 0.0, -1.0)), ((10.5, y, row), (-1.0, 0.0, 0.0)),
                ((row, y, -10.5), (0.0, 0.0, 1.0)), ((-10.5, y, row), (1.0, 0.0, 1.0)), ((-10.5, y, row), (1.0, 0.0, -0.5))][k % 6]
        R.add("axis", o, d)
    for k in range(16):                               # over the grid box, through the r = 1 light
        R.add("miss_grid_hit_big", (-8.0, 1.2 + 0.04 * k, -0.4 + rng.uniform(-0.3, 0.3)),
              (1.0, 0.0 if k % 2 == 0 else 0.01, 0.0))
    for k in range(16):                               # missing everything
        R.add("miss_all", (rng.uniform(-9, 9), 3.0 + k, rng.uniform(-9, 9)), (rng.uniform(-1, 1), 1.0, rng.uniform(-1, 1)))
    base_o, base_d, base_t = list(R.o[:32]), list(R.d[:32]), list(R.tgt[:32])
    for k in range(32):                               # directions scaled by 2^+-20
        R.add("scaled_dir", base_o[k], base_d[k] * (2.0 ** (20 if k % 2 else -20)), base_t[k])
    R.add("nan", (0.0, 0.0, 0.0), (1.0, 0.0, 0.0))


def _sampled(target, n_lights, seed):
    """the `sampled` light of each ray: the light it was aimed at, another one,
    or none"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, n_lights, len(target)).astype(np.int32)
    aimed = (target >= 0) & (np.arange(len(target)) % 2 == 0)
    s[aimed] = target[aimed]
    s[(np.arange(len(target)) % 8 == 7) & ~aimed] = -1
    return s


def _waves(n_rays, seed, full=True):
    """every block of 64 rays at every P, in order and in a second lane
    permutation (over the whole case), then the pend patterns on block 0"""
    rng = np.random.default_rng(seed)
    blocks = n_rays // 64
    perm = rng.permutation(n_rays)
    ones = np.ones(64, np.uint32)
    W = []
    ps = P_VALUES if full else (3, 1 << 20)
    for pi, P in enumerate(ps):
        for b in range(blocks):
            cap = CAP_WORDS[(b + pi) % 2]
            W.append(Wave(P, cap, np.arange(64 * b, 64 * b + 64), ones.copy(), "main"))
            W.append(Wave(P, CAP_WORDS[(b + pi + 1) % 2], perm[64 * b:64 * b + 64].copy(), ones.copy(), "perm"))
    lane = np.arange(64)
    b0 = np.arange(64)
    for kind, P, cap, pend in (("none", 16, 512, lane < 0), ("alternating", 1 << 20, 512, lane % 2 == 0),
                               ("lane0", 1 << 20, 1536, lane == 0), ("lane63", 3, 512, lane == 63),
                               ("alternating", 1, 512, lane % 2 == 1), ("short", 16, CAP_SHORT, lane % 2 == 0)):
        W.append(Wave(P, cap, b0.copy(), pend.astype(np.uint32), kind))
    return W


def _case(name, L, R, scale=1.0, shift=(0.0, 0.0, 0.0), big=(), cluster=(), seed=10, full=True):
    rays, fam, tgt = R.done(scale, shift)
    Ls = L.copy()
    Ls[:, :3] = Ls[:, :3] * scale + np.asarray(shift, float)
    Ls[:, 3] *= scale
    return Case(name, Ls, rays, fam, tgt, _sampled(tgt, len(L), seed), _waves(len(rays), seed + 1, full), tuple(big),
                tuple(cluster), scale, tuple(shift))


def layer_case(name="layer", scale=1.0, shift=(0.0, 0.0, 0.0)):
    L = layer_lights()
    R = _Rays()
    _layer_rays(R, L, np.random.default_rng(11), np.arange(400))
    return _case(name, L, R, scale, shift, big=(400,))


def cluster_case():
    L, ids = cluster_lights()
    small = np.array([k for k in range(len(L)) if L[k, 3] == R0])
    R = _Rays()
    # along x through all 12 (they sit between two lattice rows): > 8 in an owner
    # list, > 6 in one piece
    R.add("cluster", (-12.0, R0, 1.0), (1.0, 0.0, 0.0), ids[0])
    R.add("cluster", (12.0, R0 + 0.01, 1.02), (-1.0, 0.0, -0.001), ids[5])
    R.add("cluster", (-3.0, R0 - 0.02, 0.98), (1.0, 0.001, 0.002), ids[11])
    _layer_rays(R, L, np.random.default_rng(12), small, n_skim=61)
    big = tuple(int(k) for k in range(len(L)) if L[k, 3] == 1.0)
    return _case("cluster", L, R, big=big, cluster=ids, seed=20)


def bigs_case():
    L, ids = bigs_lights()
    small = np.array([k for k in range(len(L)) if L[k, 3] == R0])
    R = _Rays()
    # from above and from the side through all four nested lights (and from
    # outside them: no f32 term is NaN)
    R.add("bigs", (3.0, 8.0, -4.0), (0.0, -1.0, 0.0), ids[0])
    R.add("bigs", (3.1, 6.0, -3.9), (0.0, -1.0, 0.01), ids[1])
    R.add("bigs", (-9.0, 0.6, -4.0), (1.0, -0.02, 0.0), ids[3])
    _layer_rays(R, L, np.random.default_rng(13), small, n_skim=61)
    big = ids + tuple(int(k) for k in range(len(L)) if L[k, 3] == 1.0)
    return _case("bigs", L, R, big=big, seed=30)


def row_case(n, inf_radius=False):
    """n lights in a row; inf_radius: the last one's radius is +inf (every f32
    term of it is NaN: only with n = 2, where no row has m >= 3)"""
    L = row_lights(n)
    if inf_radius:
        L[n - 1, 3] = np.inf
    rng = np.random.default_rng(40 + n)
    R = _Rays()
    for k in range(8):                                # along the row: every light
        R.add("row", (-1.0 - 0.5 * k, R0 + 0.01 * k, 0.02 * k), (1.0, 0.0, 0.0), n - 1)
        R.add("row", (0.5 * n + 1.0 + k, R0, -0.03), (-1.0, 0.001 * k, 0.0), 0)
    for k in range(24):                               # across it, down on it, past it
        t = int(rng.integers(n))
        R.add("vertical", (L[t, 0] + rng.uniform(-0.3, 0.3), 4.0, rng.uniform(-0.3, 0.3)), (0.0, -1.0, 0.0), t)
        R.add("skim", (L[t, 0] + rng.uniform(-2, 2), R0, -5.0), (rng.uniform(-0.2, 0.2), 0.0, 1.0), t)
    for k in range(8):
        R.add("miss_all", (0.0, 3.0 + k, 0.0), (0.3, 1.0, 0.1))
    c = _case(f"row{n}" + ("_inf" if inf_radius else ""), L, R, seed=50 + n, full=False)
    # the last light of the list (the odd tail, the second 32-block) as `sampled` on the rays that miss it
    c.sampled[c.family == FAMILIES.index("vertical")] = n - 1
    return c


def degenerate_case():
    L, ids = degenerate_lights()
    small = np.array([k for k in range(len(L)) if L[k, 3] == R0 and k not in ids])
    R = _Rays()
    for k, i in enumerate(ids):                       # at each odd light: down on it and through it sideways
        R.add("vertical", (L[i, 0] + 0.03, 4.0, L[i, 2] - 0.02), (0.0, -1.0, 0.0), i)
        R.add("skim", (L[i, 0] - 7.0, R0 + 0.01, L[i, 2] + 0.01), (1.0, 0.0, 0.0), i)
    rng = np.random.default_rng(14)
    for k in range(46):
        t = int(small[rng.integers(len(small))])
        u = rng.uniform(-4.0, 4.0)
        o = np.array([(-6.0, R0, u), (u, R0, 6.0)][k % 2])
        R.add("skim", o, L[t, :3] - o, t)
    nan_id = [i for i in ids if np.isnan(L[i, 3])]
    return _case("degenerate", L, R, big=tuple(nan_id), seed=60, full=False)


def boundary_case(base, header, max_lights=100):
    """`base` (a layer case) with the radii of interior lights nudged so that
    c + r or c - r lies on a cell plane of the grid the probe reported for it
    (header: lo, cell, n), and rays whose closest approach to such a light lies
    within f32 rounding of that plane, on both sides.  Fewer than half of the
    lights change and none grows, so the median radius, the box and the grid
    stay (the test re-stages and checks)."""
    lo, cell, n = np.asarray(header["lo"]), np.asarray(header["cell"]), np.asarray(header["n"])
    s, shift = base.scale, np.asarray(base.shift)
    L = base.lights.copy()
    r0 = R0 * s
    picked = []
    for k in range(400):
        c = L[k, :3]
        if np.any(np.abs((c - shift) / s)[[0, 2]] > 8.0) or len(picked) >= max_lights:
            continue
        for a, sign in ((0, 1), (2, -1), (2, 1), (0, -1))[k % 4:] + ((0, 1), (2, -1), (2, 1), (0, -1))[:k % 4]:
            if n[a] < 2:
                continue
            u = (c[a] - lo[a]) / cell[a]
            plane = lo[a] + (np.ceil(u) if sign > 0 else np.floor(u)) * cell[a]
            dist = abs(plane - c[a])
            if 0.4 * r0 <= dist <= r0:
                picked.append((k, a, sign, float(plane)))
                L[k, 3] = dist * (1.0 - 2.0 ** -30)           # the sphere ends just inside the plane
                break
    O, D, T = [], [], []
    for (k, a, sign, plane) in picked:
        c = L[k, :3]
        b = 2 - a                                             # the ray runs along the other horizontal axis
        ulp = float(np.spacing(np.float32(abs(plane))))
        # start outside every light (an f32 pdf term of a ray that starts inside one is NaN)
        for back in (3.0, 3.4, 2.6, 3.8, 2.2, 4.2):
            o = c.copy()
            o[a], o[b] = plane, c[b] - back * s
            if not (np.linalg.norm(L[:, :3] - o, axis=1) < np.abs(L[:, 3]) + 0.06 * s).any():
                break
        else:
            raise AssertionError("no free start for a tangent ray")
        for q in (0.25, 1.0, 4.0, 16.0):
            for side in (1.0, -1.0):                          # on the sphere's side of the plane, and beyond it
                for slope in (0.0, 2.0 ** -10, -(2.0 ** -10)):
                    o, d = c.copy(), np.zeros(3)
                    d[b], d[a] = s, slope * s
                    o[b] = c[b] - back * s
                    # passes the centre's b-coordinate q ulps (of f32 at the plane) from the plane
                    o[a] = (plane - sign * side * q * ulp) - back * s * slope
                    O.append(o)
                    D.append(d)
                    T.append(k)
    fam = [FAMILIES.index("tangent")] * len(O)
    while len(O) % 64:                                        # whole waves: rays that miss everything
        O.append(shift + s * np.array([0.0, 50.0 + len(O), 0.0]))
        D.append(s * np.array([0.1, 1.0, 0.2]))
        T.append(-1)
        fam.append(FAMILIES.index("pad"))
    rays = np.concatenate([np.array(O), np.array(D)], axis=1)
    tgt = np.array(T, np.int32)
    return Case(base.name + "_boundary", L, rays, np.array(fam, np.int32), tgt, _sampled(tgt, len(L), 70),
                _waves(min(len(rays), 512), 71, full=False), base.big, (), s, tuple(shift), {"picked": picked})


SHIFT = (1e4, 0.0, 1e4)


def base_cases():
    """every case that needs no grid from the probe: (case, densities)"""
    return [(layer_case(), DENSITIES),
            (cluster_case(), (DENSITY, 16.0)),
            (bigs_case(), (DENSITY,)),
            (row_case(1), (DENSITY,)), (row_case(2), (DENSITY,)), (row_case(3), (DENSITY,)),
            (row_case(33), (DENSITY, 16.0)), (row_case(2, inf_radius=True), (DENSITY,)),
            (degenerate_case(), (DENSITY,)),
            (layer_case("shifted", 1.0, SHIFT), DENSITIES),
            (layer_case("scaled_up", 2.0 ** 10), (DENSITY,)),
            (layer_case("scaled_down", 2.0 ** -10), (DENSITY,))]


BOUNDARY_OF = ("layer", "shifted")      # boundary_case(case, the probe's header) at DENSITY


def pack(case, density):
    """the probe's IN file"""
    n, m, w = len(case.lights), len(case.rays), len(case.waves)
    out = [np.array([n, m, w], "<u8").tobytes(), np.array([density], "<f8").tobytes(),
           np.ascontiguousarray(case.lights, "<f8").tobytes(), np.ascontiguousarray(case.rays, "<f8").tobytes(),
           np.ascontiguousarray(case.sampled, "<i4").tobytes()]
    for wv in case.waves:
        out.append(np.array([wv.P, wv.cap_words], "<u4").tobytes())
        out.append(np.ascontiguousarray(wv.ray, "<u4").tobytes())
        out.append(np.ascontiguousarray(wv.pend, "<u4").tobytes())
    return b"".join(out)


def records(case, ray_ids=None):
    """(rays x lights, 10) {o, d, c, r} records for the oracle's batch calls"""
    rays = case.rays if ray_ids is None else case.rays[ray_ids]
    m, n = len(rays), len(case.lights)
    rec = np.empty((m, n, 10))
    rec[:, :, :6] = rays[:, None, :]
    rec[:, :, 6:] = case.lights[None, :, :]
    return rec.reshape(-1, 10)
