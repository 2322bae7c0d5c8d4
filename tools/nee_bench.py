#!/usr/bin/env python3
"""Throughput of the any-hit and light-sample queries (rtw_occluded_rays_device /
rtw_light_sample_device) on the scenes and rays of tools/query_bench.py (C2:
scenes::simple, 484 spheres; C3: 10k spheres, 488 lights; 2^22 rays), under the
default tuning, both precisions:

  any_hit_inf   the any-hit at t_max = +inf against hit_rays of the same context
                on the same rays (coherent camera rays and incoherent bounces),
                alternated; "spread" is that of repeating the same query
  shadow        rays from the camera rays' first hits towards a sampled light
                direction (light_sample), t_max = just short of the light's surface
                (sphere lights: (|c - o| - |r|) (1 - 1e-4) along the unit direction, so
                that the light's own sphere is not the blocker), t_min = 1e-3: any hit against the closest-hit query on the same rays,
                Mrays/s and node visits per ray
  light_sample  with and without the fused pdf against light_pdf alone, from the
                same first hits

Timing: the library's device events around each kernel
(rtw_query_stats.kernel_ms), one warm-up, then `--repeats` rounds that visit
every query in turn.  One JSON line per measurement.

  python tools/nee_bench.py [--rays 4194304] [--repeats 5] [--scenes C2,C3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_tracing_weekend_amd as rtw  # noqa: E402
from query_bench import SCENES, SEED, bounce_rays, camera_rays  # noqa: E402


def line_of(sname, pname, what, query, n, ms, st, **more):
    rate = n / np.array(ms) / 1e3
    out = {"scene": sname, "dtype": pname, "measure": what, "query": query, "rays": n,
           "mrays_per_s": round(float(np.median(rate)), 1),
           "spread": [round(float(rate.min()), 1), round(float(rate.max()), 1)],
           "kernel_ms": round(float(np.median(ms)), 4), "kernel": int(st.kernel),
           "hit_share": round(st.hits / max(st.rays, 1), 4), "node_visits_per_ray": round(st.node_visits / max(st.rays, 1), 2),
           "sphere_tests_per_ray": round(st.sphere_tests / max(st.rays, 1), 2),
           "light_tests_per_ray": round(st.light_tests / max(st.rays, 1), 2)}
    out.update(more)
    print(json.dumps(out), flush=True)
    return out


def alternate(r, queries, repeats):
    """{name: ([kernel_ms per repeat], last stats)}: one warm-up, then every query in turn"""
    ms = {k: [] for k in queries}
    st = {}
    for rep in range(1 + repeats):
        for k, run in queries.items():
            run()
            st[k] = r.get_query_stats()
            if rep:
                ms[k].append(st[k].kernel_ms)
    return ms, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", default="C2,C3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for sname in a.scenes.split(","):
        cfg = SCENES[sname]
        soa, b = rtw.scenes.simple_soa(SEED, cfg["n"])
        cam = b.with_image_width(cfg["w"]).with_image_height(cfg["h"]).with_samples_per_pixel(cfg["spp"]) \
               .with_max_depth(50).build()
        lights = torch.tensor(np.asarray(soa.lights), dtype=torch.float64, device=dev).reshape(-1, 4)
        for pname, prec, dtype in (("f32", rtw.RTW_F32, torch.float32), ("f64", rtw.RTW_F64, torch.float64)):
            with rtw.Renderer(device=0, precision=prec) as r:
                r.set_scene(soa)
                coherent = camera_rays(cam, a.rays, dtype, dev)
                hits, ids = r.hit_rays(coherent)
                sets = {"coherent": coherent, "incoherent": bounce_rays(hits, ids, a.rays, dtype, dev)}
                # 1. any hit at +inf against the closest hit, alternated
                for s, rays in sets.items():
                    ms, st = alternate(r, {"hit_rays": lambda: r.hit_rays(rays), "occluded": lambda: r.occluded(rays),
                                        "hit_rays again": lambda: r.hit_rays(rays)}, a.repeats)
                    for q in ms:
                        lines.append(line_of(sname, pname, "any_hit_inf", q, len(rays), ms[q], st[q], rays_set=s))
                # 2. shadow rays from the first hits towards sampled lights
                hit = torch.nonzero(ids[:, 0] >= 0)[:, 0]
                pick = hit[torch.arange(a.rays, device=dev) % len(hit)]
                origins = hits[pick, 1:4].contiguous()
                d, _, light = r.light_sample(origins, 7, 0, 0)
                L = lights[light.long()]
                way = ((L[:, :3] - origins.double()).norm(dim=1) - L[:, 3].abs()).clamp_min(0.0) * (1.0 - 1e-4)
                ok = torch.isfinite(d).all(1)
                shadow = torch.cat([origins, d], 1)[ok].contiguous()
                t_max = way[ok].to(dtype).contiguous()
                t_min = 1e-3
                ms, st = alternate(r, {"hit_rays": lambda: r.hit_rays(shadow, t_min),
                                    "occluded": lambda: r.occluded(shadow, t_max, t_min),
                                    "occluded t_max inf": lambda: r.occluded(shadow, None, t_min)}, a.repeats)
                for q in ms:
                    lines.append(line_of(sname, pname, "shadow", q, len(shadow), ms[q], st[q], lights=len(lights)))
                # 3. light sampling with and without the fused pdf, and the pdf alone
                pairs = torch.cat([origins, d], 1).contiguous()
                ms, st = alternate(r, {"light_sample + pdf": lambda: r.light_sample(origins, 7, 0, 0),
                                    "light_sample": lambda: r.light_sample(origins, 7, 0, 0, pdf=False),
                                    "light_pdf": lambda: r.light_pdf(pairs)}, a.repeats)
                for q in ms:
                    lines.append(line_of(sname, pname, "light_sample", q, len(origins), ms[q], st[q], lights=len(lights)))
                del hits, ids, sets, coherent, shadow, pairs, origins
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
