#!/usr/bin/env python3
"""Throughput of the path queries (rtw_camera_rays_device / rtw_shade_rays_device)
and of the wavefront loop they make with rtw_hit_rays, under the default tuning,
both precisions, on scenes::simple (the Book-1 scene, 484 spheres):

  camera_rays   2^22 rays of one sample of a 2048 x 2048 image (no defocus, and
                with a wide aperture: the UnitDisk loop)
  shade_rays    the bounce of those rays' first hits (coherent), and of the second
                segment's hits (incoherent), with and without the pdfs
  wavefront     Renderer.render_wavefront (torch tensors on the GPU) against
                Renderer.render on the same camera, wall clock after one warm-up:
                Mpaths/s of each and their ratio

Timing of the queries: the library's device events around each kernel
(rtw_query_stats.kernel_ms), one warm-up, then `--repeats` rounds that visit
every query in turn.  One JSON line per measurement.

  python tools/path_bench.py [--rays 4194304] [--repeats 5] [--width 256] [--height 160] [--spp 4] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ray_tracing_weekend_amd as rtw  # noqa: E402

SEED = 7


def line_of(pname, what, query, n, ms, st, **more):
    rate = n / np.array(ms) / 1e3
    out = {"scene": "C2", "dtype": pname, "measure": what, "query": query, "rays": n,
           "mpaths_per_s": round(float(np.median(rate)), 1),
           "spread": [round(float(rate.min()), 1), round(float(rate.max()), 1)],
           "kernel_ms": round(float(np.median(ms)), 4), "kernel": int(st.kernel),
           "continue_share": round(st.hits / max(st.rays, 1), 4),
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
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=160)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    soa, b = rtw.scenes.simple_soa(0x5EED0001, 11)
    side = int(round(a.rays ** 0.5))
    big = b.copy().with_image_width(side).with_image_height(a.rays // side).with_samples_per_pixel(1).with_max_depth(50)
    n = side * (a.rays // side)
    for pname, prec in (("f32", rtw.RTW_F32), ("f64", rtw.RTW_F64)):
        with rtw.Renderer(device=0, precision=prec) as r:
            r.set_scene(soa)
            cam, dcam = big.build(), big.copy().with_defocus_angle(2.0).with_focus_dist(10.0).build()
            ms, st = alternate(r, {"camera_rays": lambda: r.camera_rays(cam, SEED, 0, as_torch=True),
                                   "camera_rays defocus": lambda: r.camera_rays(dcam, SEED, 0, as_torch=True)},
                               a.repeats)
            for q in ms:
                lines.append(line_of(pname, "camera_rays", q, n, ms[q], st[q]))
            rays, rng0 = r.camera_rays(cam, SEED, 0, as_torch=True)
            for s in ("coherent", "incoherent"):
                hits, ids = r.hit_rays(rays)
                state = rng0.clone()
                ms, st = alternate(r, {"shade_rays": lambda: r.shade_rays(rays, hits, ids, state.copy_(rng0)),
                                       "shade_rays + pdfs": lambda: r.shade_rays(rays, hits, ids, state.copy_(rng0),
                                                                                 pdfs=True)}, a.repeats)
                for q in ms:
                    lines.append(line_of(pname, "shade_rays", q, len(rays), ms[q], st[q], rays_set=s))
                if s == "coherent":            # the next segment: the paths that go on
                    nxt, _, _, event = r.shade_rays(rays, hits, ids, state.copy_(rng0))
                    keep = torch.nonzero(event >= 2).reshape(-1)
                    keep = keep[torch.arange(len(rays), device=rays.device) % len(keep)]
                    rays, rng0 = nxt[keep].contiguous(), state[keep].contiguous()
            del rays, rng0, hits, ids, state
            # the wavefront loop against the megakernel
            small = b.copy().with_image_width(a.width).with_image_height(a.height).with_samples_per_pixel(a.spp) \
                     .with_max_depth(50).build()
            paths = a.width * a.height * a.spp
            wall = {}
            for what, run in (("render", lambda: r.render(small, SEED)),
                              ("render_wavefront", lambda: r.render_wavefront(small, SEED, as_torch=True).cpu())):
                run()
                t = []
                for _ in range(a.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run()
                    torch.cuda.synchronize()
                    t.append(time.perf_counter() - t0)
                wall[what] = float(np.median(t))
            out = {"scene": "C2", "dtype": pname, "measure": "wavefront", "width": a.width, "height": a.height,
                   "spp": a.spp, "paths": paths, "render_ms": round(wall["render"] * 1e3, 2),
                   "wavefront_ms": round(wall["render_wavefront"] * 1e3, 2),
                   "render_mpaths_per_s": round(paths / wall["render"] / 1e6, 2),
                   "wavefront_mpaths_per_s": round(paths / wall["render_wavefront"] / 1e6, 2),
                   "wavefront_over_render": round(wall["render_wavefront"] / wall["render"], 2)}
            print(json.dumps(out), flush=True)
            lines.append(out)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
