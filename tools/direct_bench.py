#!/usr/bin/env python3
"""Direct lighting as one query (rtw_direct_light_device) against the composition
of the existing queries that gives the same sums, timed in the same run:

  fused        Renderer.direct_light(points, seed, S) -- one call, 48 B in (f64) and
               24 B out per point whatever S
  composition  per sample: light_sample -> torch.cat -> hit_rays -> shade_rays (for
               `emitted`, with a spare RNG state) -> the scattering pdf, the term and
               the fold in torch

Points: 2^22 first hits of a grid of camera rays (tools/query_bench.py) of C2
(scenes::simple, 484 spheres, 19 sphere lights that do not emit: the traversal
and the records are the work) and of cornell_box (a quad light and a sphere in
a mixed list).  S = 1 and 8, both precisions, one warm-up, the minimum of
`--repeats` wall times between device events (the composition's torch glue is
part of what its caller pays); kernel_ms is the sum of the library's own kernel
times.  peak_bytes: torch's peak allocation above the inputs during one call
-- the records a form moves through memory.  One JSON line per measurement.

  python tools/direct_bench.py [--points 4194304] [--repeats 5] [--scenes C2,cornell_box] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_tracing_weekend_amd as rtw  # noqa: E402
from query_bench import SCENES, SEED, camera_rays  # noqa: E402


def composition(r, pts, seed, S, kms):
    """the sums of direct_light from the existing queries; kms collects their kernel times"""
    n = len(pts)
    o, nrm = pts[:, :3].contiguous(), pts[:, 3:6]
    direct = torch.zeros((n, 3), dtype=torch.float64, device=pts.device)
    rng = torch.ones((n, 4), dtype=torch.int64, device=pts.device)
    for s in range(S):
        d, pdf, _ = r.light_sample(o, seed, 0, s)
        kms.append(r.get_query_stats().kernel_ms)
        rays = torch.cat([o, d], 1)
        hits, ids = r.hit_rays(rays)
        kms.append(r.get_query_stats().kernel_ms)
        emitted = r.shade_rays(rays, hits, ids, rng.clone())[2]
        kms.append(r.get_query_stats().kernel_ms)
        spdf = ((nrm * (d / d.norm(dim=1, keepdim=True))).sum(1) / math.pi).clamp_min(0.0)
        adds = (ids[:, 0] >= 0) & (pdf > 0) & (spdf > 0)
        term = emitted * (spdf / pdf)[:, None]
        direct += torch.where(adds[:, None], term, torch.zeros_like(term)).double()
    return direct


def timed(run, repeats):
    """(min wall ms between device events over `repeats` runs after a warm-up, the last result)"""
    out, ms = run(), []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return min(ms), out


def peak(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = run()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", default="C2,cornell_box")
    ap.add_argument("--samples", default="1,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for sname in a.scenes.split(","):
        if sname in SCENES:
            cfg = SCENES[sname]
            soa, b = rtw.scenes.simple_soa(SEED, cfg["n"])
            b = b.with_image_width(cfg["w"]).with_image_height(cfg["h"])
        else:
            soa, b = rtw.scenes.named_soa(sname)
            b = b.with_image_width(1200).with_image_height(1200)
        cam = b.with_samples_per_pixel(1).with_max_depth(50).build()
        for pname, prec, dtype in (("f32", rtw.RTW_F32, torch.float32), ("f64", rtw.RTW_F64, torch.float64)):
            with rtw.Renderer(device=0, precision=prec) as r:
                r.set_scene(soa)
                hits, ids = r.hit_rays(camera_rays(cam, a.points, dtype, dev))
                hit = torch.nonzero(ids[:, 0] >= 0)[:, 0]
                pts = hits[hit[torch.arange(a.points, device=dev) % len(hit)], 1:7].contiguous()
                del hits, ids, hit
                for S in map(int, a.samples.split(",")):
                    kms = []
                    ms_f, fused = timed(lambda: r.direct_light(pts, 7, S), a.repeats)
                    st = r.get_query_stats()
                    ms_c, comp = timed(lambda: composition(r, pts, 7, S, kms), a.repeats)
                    k_c = sum(kms[-3 * S:])
                    scale = float(comp.abs().max().clamp_min(1e-30))
                    line = {"scene": sname, "dtype": pname, "points": len(pts), "samples": S,
                            "fused_ms": round(ms_f, 3), "composition_ms": round(ms_c, 3),
                            "ratio": round(ms_c / ms_f, 3), "fused_kernel_ms": round(st.kernel_ms, 3),
                            "composition_kernel_ms": round(k_c, 3),
                            "fused_mpairs_per_s": round(len(pts) * S / ms_f / 1e3, 1), "kernel": int(st.kernel),
                            "terms_share": round(st.hits / max(st.rays, 1), 4),
                            "node_visits_per_pair": round(st.node_visits / max(st.rays, 1), 2),
                            "light_tests_per_pair": round(st.light_tests / max(st.rays, 1), 2),
                            "max_rel_diff": float((fused - comp).abs().max()) / scale,
                            "fused_peak_bytes": peak(lambda: r.direct_light(pts, 7, S)),
                            "composition_peak_bytes": peak(lambda: composition(r, pts, 7, S, [])),
                            "input_bytes": pts.numel() * pts.element_size()}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    del fused, comp
                del pts
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
