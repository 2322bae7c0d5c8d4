"""The f64 kernels' f32 culling filters, primitive by primitive, on the GPU.

tests/native/cull_probe.hip runs one thread per record of tests/cull_cases.py
through sphere_t<double> / sphere_pdf_value<double> (which must BE the
reference: same flag, same bits) and through the f32 filters in front of them
-- sphere_may_hit on the sphere as stage_scene.cpp rounds it, LightPre /
light_may_hit, the widened slab test of bvh_traverse_ww and the slab test of
bvh4_traverse on a one-node tree -- which must be conservative: whatever the
reference accepts, the filter keeps.  Zero exceptions, at every scale from
2^-130 to 2^130.

The filters' rejection rate on the clear misses is printed per scale and not
asserted: a filter that stopped culling is a performance matter.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cull_cases as cc
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAD_REL = 1e-12          # host/stage_scene.cpp: build_bvh's pad_rel of the f64 tree

ROW = np.dtype([("t_world", "<f8"), ("t_light", "<f8"), ("pdf", "<f8"), ("hit_world", "<u4"),
                ("hit_light", "<u4"), ("may_sphere", "<u4"), ("may_light", "<u4")])
BOXROW = np.dtype([("ww", "<u4"), ("wide4", "<u4")])


def _tree_boxes(B):
    """the box as the tree holds it: padded like build_bvh pads (pad_rel (scale + 1),
    with the box's own extent for the scene's scale: the least any scene pads
    it), then -- the f32 tree -- rounded outward"""
    lo, hi = B[:, 6:9], B[:, 9:12]
    pad = PAD_REL * (np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True) + 1.0)
    lo, hi = lo - pad, hi + pad
    l32, h32 = cc.f32_box_outward(lo, hi)
    dev = B.copy()
    dev[:, 6:9], dev[:, 9:12] = lo, hi
    return dev, np.concatenate([l32, h32], axis=1).astype(np.float32)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """compile once, run once: (sphere rows, box rows)"""
    tmp = tmp_path_factory.mktemp("cull_probe")
    exe = str(tmp / "cull_probe")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "cull_probe.hip"),
                    "-o", exe], check=True, capture_output=True, timeout=600)
    R = cc.records()
    B, _, _ = cc.box_records()
    dev_boxes, b32 = _tree_boxes(B)
    n, m = len(R.rec), len(B)
    assert n <= 1 << 20 and m <= 1 << 20
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, m], "<u8").tobytes())
        f.write(np.ascontiguousarray(R.rec, "<f8").tobytes())
        f.write(np.ascontiguousarray(cc.f32_sphere(R.rec), "<f4").tobytes())
        f.write(np.ascontiguousarray(dev_boxes, "<f8").tobytes())
        f.write(np.ascontiguousarray(b32, "<f4").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    assert len(raw) == n * ROW.itemsize + m * BOXROW.itemsize
    rows = np.frombuffer(raw[: n * ROW.itemsize], ROW)
    boxes = np.frombuffer(raw[n * ROW.itemsize:], BOXROW)
    return rows, boxes


@pytest.fixture(scope="module")
def reference():
    R = cc.records()
    hit_w, t_w = O.sphere_hit_batch(R.rec)
    hit_l, t_l = O.sphere_hit_batch(R.rec, 0.0)
    return hit_w, t_w, hit_l, t_l, O.sphere_pdf_value_batch(R.rec)


def _offenders(bad, R, extra=None):
    """the first offenders, by family and scale"""
    idx = np.flatnonzero(bad)
    lines = [f"{len(idx)} of {len(bad)} records"]
    seen = {}
    for i in idx:
        key = (cc.FAMILIES[R.family[i]], int(R.k[i]), int(R.tier[i]))
        seen[key] = seen.get(key, 0) + 1
    lines.append("  by (family, 2^k, tier): " + ", ".join(f"{k}: {v}" for k, v in sorted(seen.items())[:40]))
    for i in idx[:8]:
        lines.append(f"  #{i} {cc.FAMILIES[R.family[i]]} 2^{R.k[i]} tier {R.tier[i]}: o={R.rec[i, 0:3].tolist()} "
                     f"d={R.rec[i, 3:6].tolist()} c={R.rec[i, 6:9].tolist()} r={R.rec[i, 9]!r}"
                     + (f" {extra(i)}" if extra else ""))
    return "\n".join(lines)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_p1_sphere_t_is_the_reference(probe, reference):
    rows, _ = probe
    hit_w, t_w, hit_l, t_l, _ = reference
    R = cc.records()
    for name, gh, gt, rh, rt in (("world", rows["hit_world"], rows["t_world"], hit_w, t_w),
                                 ("light", rows["hit_light"], rows["t_light"], hit_l, t_l)):
        bad = (gh != 0) != rh
        bad |= rh & (_bits(gt) != _bits(rt))
        assert not bad.any(), f"sphere_t<double>, {name} query:\n" + _offenders(
            bad, R, lambda i: f"gpu ({gh[i]}, {gt[i]!r}) oracle ({rh[i]}, {rt[i]!r})")


def test_p2_sphere_pdf_value_is_the_reference(probe, reference):
    rows, _ = probe
    pdf = reference[4]
    R = cc.records()
    both_nan = np.isnan(rows["pdf"]) & np.isnan(pdf)
    bad = ~both_nan & (_bits(rows["pdf"]) != _bits(pdf))
    assert np.isnan(pdf).any() and (pdf > 0).any()
    assert not bad.any(), "sphere_pdf_value<double>:\n" + _offenders(
        bad, R, lambda i: f"gpu {rows['pdf'][i]!r} oracle {pdf[i]!r}")


def _print_cull_share(name, kept, R):
    miss = R.family == cc.FAMILIES.index("clear_miss")
    print(f"{name}: share of the clear misses rejected, by scale")
    for k in sorted(set(R.k.tolist())):
        m = miss & (R.k == k)
        print(f"  2^{k}: {1.0 - kept[m].mean():.3f} of {m.sum()}")


def test_p3_sphere_may_hit_keeps_every_hit(probe, reference):
    rows, _ = probe
    R = cc.records()
    kept = rows["may_sphere"] != 0
    _print_cull_share("sphere_may_hit", kept, R)
    # the leaf pre-pass stands in front of the world query; the light query's
    # hits (t_min = 0) are a superset and must be kept as well
    need = reference[0] | reference[2]
    assert need.sum() > 10000
    bad = need & ~kept
    assert not bad.any(), "sphere_may_hit culls a sphere the reference hits:\n" + _offenders(bad, R)


def test_p4_light_may_hit_keeps_every_light_with_a_pdf(probe, reference):
    rows, _ = probe
    R = cc.records()
    kept = rows["may_light"] != 0
    _print_cull_share("light_may_hit", kept, R)
    pdf = reference[4]
    need = np.isnan(pdf) | (pdf != 0.0)
    assert need.sum() > 10000
    bad = need & ~kept
    assert not bad.any(), "light_may_hit culls a light whose pdf is not 0:\n" + _offenders(
        bad, R, lambda i: f"pdf {pdf[i]!r}")


@pytest.mark.parametrize("which", ["ww", "wide4"])
def test_slab_test_enters_every_box_the_reference_hits(probe, which):
    """rtwo_aabb_hit on the f64 box within [0, tb] => both children (the same
    box, leaves of 1 and 2 spheres) are entered: ntest == 3."""
    _, boxes = probe
    B, fam, ks = cc.box_records()
    need = O.aabb_hit_batch(B)
    assert need.sum() > 1000
    got = boxes[which]
    names = ("o on a face", "in a face plane, zero component", "edge", "plain")
    print(f"{which}: share of the boxes the reference misses that are skipped: "
          f"{(got[~need] == 0).mean():.3f}")
    assert np.isin(got, [0, 3]).all()        # both children are the same box
    bad = need & (got != 3)
    lines = []
    for i in np.flatnonzero(bad)[:8]:
        lines.append(f"  #{i} {names[fam[i]]} 2^{ks[i]}: o={B[i, 0:3].tolist()} d={B[i, 3:6].tolist()} "
                     f"lo={B[i, 6:9].tolist()} hi={B[i, 9:12].tolist()} tb={B[i, 12]!r} ntest={got[i]}")
    by = {}
    for i in np.flatnonzero(bad):
        by[(names[fam[i]], int(ks[i]))] = by.get((names[fam[i]], int(ks[i])), 0) + 1
    assert not bad.any(), f"{which}: {bad.sum()} boxes the reference hits are not entered: {sorted(by.items())}\n" + \
        "\n".join(lines)
