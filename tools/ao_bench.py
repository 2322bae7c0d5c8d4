#!/usr/bin/env python3
"""Ambient occlusion as one query (rtw_ambient_occlusion_device) against the
any-hit query on the same pairs, timed in the same run:

  fused      Renderer.ambient_occlusion(points, seed, S, t_max) -- one call: 48 B in
             (f64) and 4 B out per point whatever S; directions drawn in registers
  traversal  Renderer.occluded on the fused call's own recorded rays {p, d} (n * S x 6,
             made once, outside the timing) with t_max per ray, then the count
             reduce in torch -- the traversal alone, without generating directions,
             reading 48 B (f64) per pair

Points: 2^22 first hits of a grid of camera rays (tools/query_bench.py) of C2
(scenes::simple, 484 spheres; t_max = +inf: the sky) and of cornell_box (t_max =
200, a finite reach).  S = 1 and 8, both precisions.  The two forms alternate;
one warm-up each, the minimum of `--repeats` wall times between device events;
*_kernel_ms are the library's own kernel times of the last run.  One JSON line
per measurement.

  python tools/ao_bench.py [--points 4194304] [--repeats 5] [--scenes C2,cornell_box] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_tracing_weekend_amd as rtw  # noqa: E402
from query_bench import SCENES, SEED, camera_rays  # noqa: E402

T_MIN = 1e-3
T_MAX = {"cornell_box": 200.0}


def event_ms(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


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
        t_max = T_MAX.get(sname, float("inf"))
        for pname, prec, dtype in (("f32", rtw.RTW_F32, torch.float32), ("f64", rtw.RTW_F64, torch.float64)):
            with rtw.Renderer(device=0, precision=prec) as r:
                r.set_scene(soa)
                hits, ids = r.hit_rays(camera_rays(cam, a.points, dtype, dev))
                hit = torch.nonzero(ids[:, 0] >= 0)[:, 0]
                pts = hits[hit[torch.arange(a.points, device=dev) % len(hit)], 1:7].contiguous()
                del hits, ids, hit
                n = len(pts)
                for S in map(int, a.samples.split(",")):
                    # the pairs of the fused call, as rays (outside the timing)
                    want, dirs, _ = r.ambient_occlusion(pts, 7, S, t_max, T_MIN, records=True)
                    rays = torch.cat([pts[:, :3].repeat_interleave(S, 0), dirs], 1).contiguous()
                    tm = torch.full((n * S,), t_max, dtype=dtype, device=dev)
                    del dirs

                    def fused():
                        return r.ambient_occlusion(pts, 7, S, t_max, T_MIN)

                    def traversal():
                        occ = r.occluded(rays, tm, T_MIN)
                        return (occ == 0).view(n, S).sum(1, dtype=torch.int32)

                    fused(), traversal()                               # the warm-up
                    ms_f, ms_t = [], []
                    for _ in range(a.repeats):                         # alternated
                        ms, got_f = event_ms(fused)
                        ms_f.append(ms)
                        k_f = r.get_query_stats()
                        ms, got_t = event_ms(traversal)
                        ms_t.append(ms)
                        k_t = r.get_query_stats()
                    assert torch.equal(got_f, want) and torch.equal(got_t, want), "the two forms count alike"
                    f, t = min(ms_f), min(ms_t)
                    line = {"scene": sname, "dtype": pname, "points": n, "samples": S, "t_max": t_max,
                            "fused_ms": round(f, 3), "traversal_ms": round(t, 3), "ratio": round(t / f, 3),
                            "fused_kernel_ms": round(k_f.kernel_ms, 3), "traversal_kernel_ms": round(k_t.kernel_ms, 3),
                            "fused_gpairs_per_s": round(n * S / f / 1e6, 3),
                            "traversal_gpairs_per_s": round(n * S / t / 1e6, 3), "kernel": int(k_f.kernel),
                            "open_share": round(1.0 - k_f.hits / max(k_f.rays, 1), 4),
                            "node_visits_per_pair": round(k_f.node_visits / max(k_f.rays, 1), 2),
                            "fused_bytes_in": pts.numel() * pts.element_size(),
                            "traversal_bytes_in": rays.numel() * rays.element_size() + tm.numel() * tm.element_size()}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    del rays, tm, want
                del pts
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
