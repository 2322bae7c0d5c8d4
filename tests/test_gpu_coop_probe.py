"""The wave-cooperative light-grid walks, ray by ray, against a sweep.

tests/native/coop_probe.hip stages the light sets of tests/coop_cases.py with
the product's own stage_scene (f32 and f64: the renderer's grid, cell records,
lg_sph32 and padding) and runs lights_pdf_grid_coop, lights_pdf_grid_coop64 and
with it lights_pdf_grid_coop_list themselves, one wave per block, next to the
lane walk, the linear sums, lights_pdf_sum_pk and a sweep of the piece walk
over the cuts 1, 2, 3, 7 and `cells`.

Walk counts: no light is counted twice at any cut, and every light the
reference gives a pdf (f64 instance, light_may_hit) or the kernel's own
light_hit_f32 hits (f32 instance, both kRobust) is counted exactly once -- on
the layer, at 1/16 to 16 cells per light, 10^4 from the origin, at 2^+-10, and
with spheres that end on a cell plane and rays that graze them there.

f64: cooperative walk, lane walk, linear sum and the reference's list-order sum
are the same bits.  f32: the paths sum the same terms in another order: equal
bits for m <= 2 hit lights, and within 2 (m - 1) 2^-24 1.01 max(path, linear)
for m >= 3 -- the worst case of two orderings of m non-negative f32 terms
(each ordering is within (m - 1) u (1 + O(m u)) of the exact sum, u = 2^-24) --
on inputs whose smallest term is at least 16 (m - 1) 2^-24 of the sum, so that
a lost or doubled term cannot hide in the bound.

Reach: the overflow paths the stock scenes rarely take are asserted from the
probe's own mark counts (a second walk, several rounds, an owner merged again,
big_over, a ray that misses the grid but hits big lights, the adapted piece
length, linked cell records).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import coop_cases as cc
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

HEADER = np.dtype([("lo", "<f8", 3), ("cell", "<f8", 3), ("n", "<u4", 3), ("n_big", "<u4"), ("n_cells", "<u4"),
                   ("n_items", "<u4"), ("pad", "<u4", 2)])
LANE64 = np.dtype([("coop", "<f8"), ("walk", "<f8"), ("lin", "<f8"), ("nbig", "<u4"), ("cells", "<u4"),
                   ("m13", "<u4"), ("m14", "<u4"), ("m16", "<u4"), ("pad", "<u4"), ("lw_tests", "<u4"),
                   ("lw_cells", "<u4")])
LANE32 = np.dtype([("coop", "<f4"), ("walk", "<f4"), ("lin", "<f4"), ("pk", "<f4"), ("pks", "<f4"), ("plain", "<f4"),
                   ("forced", "<f4"), ("minterm", "<f4"), ("sterm", "<f4"), ("m", "<u4"), ("s_hit", "<u4"),
                   ("cells", "<u4"), ("m13", "<u4"), ("m14", "<u4"), ("lw_tests", "<u4"), ("lw_cells", "<u4")])
N_PRED, N_CUT = 3, 6          # the last cut slot: the predicate alone over the light list
CUTS = ("1", "2", "3", "7", "cells")
PREDS = ("f64 grid, light_may_hit", "f32 grid, light_hit_f32<false>", "f32 grid, light_hit_f32<true>")
U = 2.0 ** -24


def compile_probe(out_dir):
    exe = os.path.join(str(out_dir), "coop_probe")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "coop_probe.hip"),
                    "-x", "hip", os.path.join(CSRC, "host", "stage_scene.cpp"), os.path.join(CSRC, "host", "bvh.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=600)
    return exe


class Run:
    """one probe run of a case at a density, parsed"""

    def __init__(self, case, density, raw):
        self.case, self.density = case, density
        n, m, w = len(case.lights), len(case.rays), len(case.waves)
        at = 0

        def take(dtype, count):
            nonlocal at
            a = np.frombuffer(raw, dtype, count, at)
            at += a.nbytes
            return a
        self.header = take(HEADER, 1)[0]
        self.big_ids = take("<u4", int(self.header["n_big"]))
        self.cell_len = take("<u4", int(self.header["n_cells"]))
        self.counts = take("u1", m * N_PRED * N_CUT * n).reshape(m, N_PRED, N_CUT, n)
        self.l64 = take(LANE64, w * 64).reshape(w, 64)
        self.l32 = [take(LANE32, w * 64).reshape(w, 64) for _ in range(2)]
        assert at == len(raw)
        self.ray = np.array([wv.ray for wv in case.waves]).reshape(w, 64)
        self.pend = np.array([wv.pend for wv in case.waves]).reshape(w, 64) != 0
        self.P = np.array([wv.P for wv in case.waves])
        self.cap = np.array([wv.cap_words for wv in case.waves])
        self.kind = np.array([wv.kind for wv in case.waves])

    @property
    def label(self):
        return f"{self.case.name} @ {self.density:g} cells/light"

    def grid_key(self):
        h = self.header
        return (h["lo"].tobytes(), h["cell"].tobytes(), tuple(h["n"]), int(h["n_big"]), tuple(self.big_ids))


def run_probe(exe, case, density, tmp):
    assert len(case.lights) <= cc.MAX_LIGHTS and len(case.rays) <= cc.MAX_RAYS and len(case.waves) <= cc.MAX_WAVES
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(cc.pack(case, density))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{case.name}: " + r.stdout + r.stderr
    with open(fout, "rb") as f:
        return Run(case, density, f.read())


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """compile once, run each case once: (the runs, {name: (base run, boundary run)})"""
    tmp = str(tmp_path_factory.mktemp("coop_probe"))
    exe = compile_probe(tmp)
    out, boundary = [], {}
    for case, densities in cc.base_cases():
        for dens in densities:
            out.append(run_probe(exe, case, dens, tmp))
            if dens == cc.DENSITY and case.name in cc.BOUNDARY_OF:
                base = out[-1]
                h = base.header
                bc = cc.boundary_case(case, {"lo": h["lo"], "cell": h["cell"], "n": h["n"]})
                out.append(run_probe(exe, bc, dens, tmp))
                boundary[case.name] = (base, out[-1])
    return out, boundary


_PDF = {}


def reference_pdf(case):
    """(rays, lights) Sphere::pdf_value of the reference, once per case"""
    if case.name not in _PDF:
        _PDF[case.name] = O.sphere_pdf_value_batch(cc.records(case)).reshape(len(case.rays), len(case.lights))
    return _PDF[case.name]


def reference_sum(case):
    """HittableList::pdf_value's sum: light by light in list order, in f64"""
    pdf = reference_pdf(case)
    acc = np.zeros(len(case.rays))
    with np.errstate(invalid="ignore"):
        for k in range(pdf.shape[1]):
            acc = acc + pdf[:, k]
    return acc


def same_bits(a, b):
    """bit for bit; a NaN matches a NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


def describe(run, wave_lane):
    """the first offenders of a (waves, 64) mask"""
    lines = []
    for w, l in np.argwhere(wave_lane)[:8]:
        r = run.ray[w, l]
        lines.append(f"  {run.label}: wave {w} ({run.kind[w]}, P={run.P[w]}, cap_words={run.cap[w]}) lane {l} "
                     f"pend={int(run.pend[w, l])} ray {r} ({cc.FAMILIES[run.case.family[r]]}) "
                     f"o={run.case.rays[r, :3].tolist()} d={run.case.rays[r, 3:].tolist()}")
    return f"{int(wave_lane.sum())} lanes\n" + "\n".join(lines)


# ---- walk counts
def _need(run, pred):
    if pred == 0:
        pdf = reference_pdf(run.case)
        return np.isnan(pdf) | (pdf != 0.0)
    return run.counts[:, pred, N_CUT - 1, :] == 1


@pytest.mark.parametrize("pred", range(N_PRED), ids=["f64_may_hit", "f32_plain", "f32_robust"])
def test_walk_counts_every_needed_light_once_at_every_cut(runs, pred):
    """no count above 1; 1 for every light the reference gives a pdf (the f64
    instance) / the probe's own light_hit_f32 hits (the f32 instances)"""
    total = sharp = 0
    for run in runs[0]:
        c = run.counts[:, pred, :N_CUT - 1, :]
        twice = c > 1
        assert not twice.any(), f"{PREDS[pred]}, {run.label}: a light counted twice: (ray, cut, light) " \
            f"{np.argwhere(twice)[:8].tolist()}"
        need = _need(run, pred)
        lost = need[:, None, :] & (c != 1)
        total += int(need.sum())
        if run.case.name.startswith("shifted") or run.case.name.endswith("_boundary"):
            sharp += int(need.sum())
        if lost.any():
            lines = []
            for r, k, l in np.argwhere(lost)[:8]:
                lines.append(f"  ray {r} ({cc.FAMILIES[run.case.family[r]]}) o={run.case.rays[r, :3].tolist()} "
                             f"d={run.case.rays[r, 3:].tolist()} cut {CUTS[k]} light {l} "
                             f"{run.case.lights[l].tolist()}")
            raise AssertionError(f"{PREDS[pred]}, {run.label}: {int(lost.sum())} (ray, cut, light) not counted:\n"
                                 + "\n".join(lines))
    print(f"{PREDS[pred]}: {total} required (ray, light) pairs, {sharp} of them in the boundary and shifted cases")
    assert total > 10000 and sharp > 1000


def test_boundary_lights_leave_the_grid_unchanged(runs):
    for name, (base, nudged) in runs[1].items():
        assert len(nudged.case.extra["picked"]) >= 20, name
        assert (nudged.case.lights[:, 3] != base.case.lights[:, 3]).sum() == len(nudged.case.extra["picked"])
        assert base.grid_key() == nudged.grid_key(), name
    assert sorted(runs[1]) == sorted(cc.BOUNDARY_OF)


# ---- f64
def test_f64_coop_walk_linear_and_reference_are_the_same_bits(runs):
    checked = nans = 0
    for run in runs[0]:
        ref = reference_sum(run.case)[run.ray]
        L = run.l64
        ok_cap = (run.cap >= cc.CAP_MIN)[:, None]
        for name in ("walk", "lin"):            # every lane computes these, pending or not
            bad = ~same_bits(L[name], ref)
            assert not bad.any(), f"f64 {name} against the reference's list-order sum: " + describe(run, bad)
        live = run.pend & ok_cap
        bad = live & ~same_bits(L["coop"], ref)
        assert not bad.any(), "lights_pdf_grid_coop64 against the reference's list-order sum: " + describe(run, bad)
        idle = ~run.pend
        bad = idle & (L["coop"].view(np.uint64) != 0)
        assert not bad.any(), "a non-pending lane does not return +0.0: " + describe(run, bad)
        # cap_words < 512: NaN for the pending lanes, by the function's comment
        short = run.pend & ~ok_cap
        bad = short & ~np.isnan(L["coop"])
        assert not bad.any(), "cap_words < 512, pending: not NaN: " + describe(run, bad)
        checked += int(live.sum())
        nans += int((live & np.isnan(ref)).sum())
    print(f"f64: {checked} pending lanes checked, {nans} of them NaN by the reference")
    assert checked > 10000
    assert any((r.pend & (r.cap < cc.CAP_MIN)[:, None]).any() for r in runs[0])


# ---- f32
@pytest.mark.parametrize("robust", [0, 1], ids=["plain", "robust"])
def test_f32_paths_sum_the_same_terms(runs, robust):
    rows3 = 0
    for run in runs[0]:
        L = run.l32[robust]
        lin, m = L["lin"], L["m"].astype(np.float64)
        bad = ~same_bits(L["plain"], lin)
        assert not bad.any(), "lights_pdf_sum against the probe's own loop: " + describe(run, bad)
        bad = ~same_bits(L["pk"], lin)
        assert not bad.any(), "lights_pdf_sum_pk(sampled = -1) against lights_pdf_sum: " + describe(run, bad)
        # condition on the inputs: on every m >= 3 row the smallest term is at least
        # 16 (m - 1) 2^-24 of the sum (so it is finite, too)
        many = L["m"] >= 3
        with np.errstate(invalid="ignore"):
            weak = many & ~(L["minterm"].astype(np.float64) >= 16.0 * (m - 1.0) * U * lin.astype(np.float64))
        assert not weak.any(), "inputs: a term too small for the bound to notice its loss: " + describe(run, weak)
        rows3 += int(many.sum())
        idle = ~run.pend
        bad = idle & (L["coop"].view(np.uint32) != 0)
        assert not bad.any(), "a non-pending lane does not return +0.0: " + describe(run, bad)
        for name, live in (("coop", run.pend), ("walk", np.ones_like(run.pend))):
            path = L[name]
            bad = live & ~many & ~same_bits(path, lin)
            assert not bad.any(), f"f32 {name}, m <= 2: not the linear sum's bits: " + describe(run, bad)
            a, b = path.astype(np.float64), lin.astype(np.float64)
            with np.errstate(invalid="ignore"):
                bad = live & many & ~(np.abs(a - b) <= 2.0 * (m - 1.0) * U * 1.01 * np.maximum(a, b))
            assert not bad.any(), f"f32 {name}, m >= 3: beyond two orderings of the same terms: " + describe(run, bad)
        # a one-piece ray sums exactly as lights_pdf_grid (lights_pdf_grid_coop's comment)
        one = run.pend & (L["cells"] <= run.P[:, None])
        bad = one & ~same_bits(L["coop"], L["walk"])
        assert not bad.any(), "a one-piece ray does not sum as lights_pdf_grid: " + describe(run, bad)
    print(f"f32 kRobust={robust}: {rows3} rows with m >= 3")
    assert rows3 > 1000


@pytest.mark.parametrize("robust", [0, 1], ids=["plain", "robust"])
def test_f32_sum_pk_sampled_override(runs, robust):
    forced = already = tail = 0
    for run in runs[0]:
        L = run.l32[robust]
        s = run.case.sampled[run.ray]
        bad = ~same_bits(L["pks"], L["forced"])
        assert not bad.any(), "lights_pdf_sum_pk(sampled = s) against the sweep with s forced in: " + describe(run, bad)
        same = (s < 0) | (L["s_hit"] != 0)
        bad = same & ~same_bits(L["pks"], L["pk"])
        assert not bad.any(), "sampled was hit anyway, yet the sum changed: " + describe(run, bad)
        new = (s >= 0) & (L["s_hit"] == 0)
        forced += int((new & ~same_bits(L["pks"], L["pk"])).sum())
        already += int(((s >= 0) & (L["s_hit"] != 0)).sum())
        n = len(run.case.lights)
        tail += int((new & (s == n - 1) & (n % 2 == 1)).sum())
    print(f"sum_pk kRobust={robust}: {forced} rows changed by `sampled`, {already} where it was hit anyway, "
          f"{tail} on an odd list's last light")
    assert forced > 1000 and already > 1000 and tail > 0


def test_result_does_not_depend_on_which_rays_share_the_wave(runs):
    """the same ray in another lane of another wave, pending: the same bits --
    f32 at the same P, f64 at any P"""
    pairs = 0
    for run in runs[0]:
        full = run.pend.all(axis=1) & (run.cap >= cc.CAP_MIN)
        first64 = {}
        first32 = [{}, {}]
        for w in np.flatnonzero(full):
            for l in range(64):
                r = int(run.ray[w, l])
                v = run.l64["coop"][w, l].tobytes()
                assert first64.setdefault(r, v) == v, f"f64, {run.label}: ray {r} differs in wave {w} lane {l}"
                for k in range(2):
                    v = run.l32[k]["coop"][w, l].tobytes()
                    key = (r, int(run.P[w]))
                    pairs += key in first32[k]
                    assert first32[k].setdefault(key, v) == v, \
                        f"f32 kRobust={k}, {run.label}: ray {r} at P={run.P[w]} differs in wave {w} lane {l}"
    assert pairs > 10000


# ---- reach
def test_the_overflow_paths_are_reached(runs):
    second_walk = rounds = remerge = big_over = off_grid = adapted = linked = False
    for run in runs[0]:
        L = run.l64
        ok = run.cap >= cc.CAP_MIN
        m13, m14, m16 = L["m13"][:, 0], L["m14"][:, 0], L["m16"][:, 0]
        second_walk |= bool((ok & (m13 >= 2)).any())
        rounds |= bool((ok & (m14 > m13)).any())
        remerge |= bool((ok & (m16 > m14)).any())
        live = run.pend & ok[:, None]
        big_over |= bool((live & (L["nbig"] >= 3)).any())
        off_grid |= bool((live & (L["cells"] == 0) & (L["coop"] != 0) & ~np.isnan(L["coop"])).any())
        walking = (live & (L["cells"] > 0)).sum(axis=1)
        adapted |= bool((ok & (run.P == 1 << 20) & (walking > 0) & (walking < 64)).any())
        if run.case.cluster:
            assert run.cell_len.max() > 4, "no cell of the cluster set lists more than 4 lights"
            linked = True
        print(f"{run.label}: marks 13/14/16 max {m13.max()}/{m14.max()}/{m16.max()}, most big candidates "
              f"{L['nbig'].max()}, longest cell list {run.cell_len.max()}, most cells {L['cells'].max()}")
    assert second_walk, "no wave walked twice (mark 13 >= 2: a piece dropped candidates)"
    assert rounds, "no wave took several rounds (mark 14 > mark 13)"
    assert remerge, "no owner merged again (mark 16 > mark 14)"
    assert big_over, "no pending lane with 3 accepted big lights"
    assert off_grid, "no pending lane that misses the grid and sums big lights"
    assert adapted, "no wave with fewer than 64 walking lanes at P = 2^20"
    assert linked
