#!/usr/bin/env python3
"""The wavefront loops against each other and against the megakernel, on
scenes::simple (the Book-1 scene), 4 spp, depth 50, both precisions, in one
process:

  render             Renderer.render (the megakernel)
  host_loop          Renderer.render_wavefront(as_torch=True): a round per sample,
                     compaction by torch operations
  driver b=1|4|0     Renderer.render_wavefront_batched: rtw_render_wavefront with
                     that batch (0: the planner's), host sums in and out as render's
  driver_torch b=0   ... its device form on torch's stream (device sums)
  hook_loop          the same batched loop in Python over path_advance, an empty hook

Wall clock after one warm-up, the minimum of `--repeats` runs, the GPU idle
before and after each.  And the advance kernel alone at `--paths` paths on
second-segment records (made as tools/path_bench.py makes them), timed by the
library's device events: Gpaths/s and the bytes it moves per second (per path
the round's event / weight / emitted / next / rng and the state's mult / res /
slot in; a survivor's state, or an ended path's colour, out).
One JSON line per measurement.

  python tools/wavefront_bench.py [--repeats 5] [--paths 4194304] [--sizes 256x160,1200x800] [--out FILE]
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


def wall_min(run, repeats):
    run()
    t = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return min(t), t


def advance_alone(r, pname, b, n_paths, repeats):
    side = int(round(n_paths ** 0.5))
    cam = b.copy().with_image_width(side).with_image_height(n_paths // side).with_samples_per_pixel(1) \
           .with_max_depth(50).build()
    rays, rng = r.camera_rays(cam, SEED, 0, as_torch=True)
    n = len(rays)
    hits, ids = r.hit_rays(rays)
    nxt, _, _, event = r.shade_rays(rays, hits, ids, rng)
    keep = torch.nonzero(event >= 2).reshape(-1)
    keep = keep[torch.arange(n, device=rays.device) % len(keep)]       # the second segment, n of them
    rays, rng = nxt[keep].contiguous(), rng[keep].contiguous()
    del nxt, keep
    hits, ids = r.hit_rays(rays)
    nxt, weight, emitted, event = r.shade_rays(rays, hits, ids, rng)
    del hits, ids, rays
    mult, res, slot = r.path_begin(n)
    colour = torch.zeros((n, 3), dtype=mult.dtype, device=mult.device)
    out = (torch.empty_like(nxt), torch.empty_like(rng), torch.empty_like(mult), torch.empty_like(res),
           torch.empty_like(slot))
    ms, m = [], 0
    for rep in range(1 + repeats):
        m = len(r.path_advance(mult, res, slot, event, weight, emitted, nxt, rng, colour, cam.background, out=out)[4])
        if rep:
            ms.append(r.get_query_stats().kernel_ms)
    esz = mult.element_size()
    bytes_in = 4 + 3 * esz * 2 + 6 * esz + 32 + 3 * esz * 2 + 4
    bytes_out_go, bytes_out_end = 6 * esz + 32 + 3 * esz * 2 + 4, 3 * esz
    moved = n * bytes_in + m * bytes_out_go + (n - m) * bytes_out_end
    best = min(ms)
    return {"scene": "C2", "dtype": pname, "measure": "path_advance", "paths": n, "survivors": m,
            "survivor_share": round(m / n, 4), "kernel_ms": round(best, 4),
            "kernel_ms_all": [round(v, 4) for v in ms], "gpaths_per_s": round(n / best / 1e6, 2),
            "bytes_per_path_in": bytes_in, "bytes_per_survivor_out": bytes_out_go,
            "tb_per_s": round(moved / best / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths", type=int, default=1 << 22)
    ap.add_argument("--sizes", default="256x160,1200x800")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    soa, b = rtw.scenes.simple_soa(0x5EED0001, 11)
    for pname, prec in (("f32", rtw.RTW_F32), ("f64", rtw.RTW_F64)):
        with rtw.Renderer(device=0, precision=prec) as r:
            r.set_scene(soa)
            for W, H in sizes:
                cam = b.copy().with_image_width(W).with_image_height(H).with_samples_per_pixel(a.spp) \
                       .with_max_depth(50).build()
                loops = {
                    "render": lambda: r.render(cam, SEED),
                    "host_loop": lambda: r.render_wavefront(cam, SEED, as_torch=True),
                    "driver b=1": lambda: r.render_wavefront_batched(cam, SEED, batch=1),
                    "driver b=4": lambda: r.render_wavefront_batched(cam, SEED, batch=4),
                    "driver b=0": lambda: r.render_wavefront_batched(cam, SEED, batch=0),
                    "driver_torch b=0": lambda: r.render_wavefront_batched(cam, SEED, batch=0, as_torch=True),
                    "hook_loop": lambda: r.render_wavefront_batched(cam, SEED, on_bounce=lambda *x: None, as_torch=True),
                }
                ms = {}
                for what, run in loops.items():
                    best, every = wall_min(run, a.repeats)
                    ms[what] = best * 1e3
                    emit({"scene": "C2", "dtype": pname, "measure": "wavefront_loops", "loop": what, "width": W,
                          "height": H, "spp": a.spp, "wall_ms_min": round(best * 1e3, 3),
                          "wall_ms_all": [round(v * 1e3, 3) for v in every]})
                st = None
                r.render_wavefront_batched(cam, SEED)
                st = r.get_query_stats()
                emit({"scene": "C2", "dtype": pname, "measure": "wavefront_ratios", "width": W, "height": H, "spp": a.spp,
                      "host_loop_over_driver_b0": round(ms["host_loop"] / ms["driver b=0"], 2),
                      "host_loop_over_driver_b1": round(ms["host_loop"] / ms["driver b=1"], 2),
                      "host_loop_over_hook_loop": round(ms["host_loop"] / ms["hook_loop"], 2),
                      "driver_b0_over_render": round(ms["driver b=0"] / ms["render"], 2),
                      "driver_torch_b0_over_render": round(ms["driver_torch b=0"] / ms["render"], 2),
                      "host_loop_over_render": round(ms["host_loop"] / ms["render"], 2),
                      "driver_device_ms": round(st.kernel_ms, 3), "segments": int(st.rays)})
            emit(advance_alone(r, pname, b, a.paths, a.repeats))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
