#!/usr/bin/env python3
"""Radiance as one query (rtw_radiance_rays_device) against the two forms that
trace the same paths, timed in the same run:

  fused        per sample s: camera_rays(s) -> radiance(rays, rng=rng, radiance=sums): one
               sample of the render per pair of calls, the sums continued on the device
  seeded       radiance(rays of sample 0, seed, S): the S samples of a ray in one launch,
               the lanes regenerating in the kernel (other streams: the same work, not the
               same paths)
  composition  rtw_render_wavefront_device (the parent's device-side rounds: camera_rays,
               hit_rays, shade_rays, path_advance, fold), batch 0
  render       Renderer.render of the same samples: the megakernel on the same work

Rays: the 2^22 camera rays of a 2048 x 2048 image of C2 (scenes::simple, 484
spheres) and of cornell_box, S = 1 and 8, depth 50, both precisions.  One
warm-up, the minimum of `--repeats` wall times between device events (host time
included: it is what a caller pays); kernel_ms is the library's own device time
of the last run (fused: the sum over its S radiance launches).  In f64 the three
camera forms give the same sums bit for bit: checked here.  peak_bytes: torch's
peak allocation above the rays during one call of the two query forms (the
driver's path state lives in the library's own buffers, not torch's).  One JSON
line per measurement.

  python tools/radiance_bench.py [--side 2048] [--repeats 5] [--scenes C2,cornell_box] [--out FILE]
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
from query_bench import SCENES, SEED  # noqa: E402


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
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", default="C2,cornell_box")
    ap.add_argument("--samples", default="1,8")
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for sname in a.scenes.split(","):
        if sname in SCENES:
            soa, b = rtw.scenes.simple_soa(SEED, SCENES[sname]["n"])
        else:
            soa, b = rtw.scenes.named_soa(sname)
        b = b.with_image_width(a.side).with_image_height(a.side).with_max_depth(a.depth)
        for pname, prec in (("f32", rtw.RTW_F32), ("f64", rtw.RTW_F64)):
            with rtw.Renderer(device=0, precision=prec) as r:
                r.set_chunk(1)
                r.set_scene(soa)
                for S in map(int, a.samples.split(",")):
                    cam = b.copy().with_samples_per_pixel(S).build()
                    n = a.side * a.side
                    kms = []

                    def fused():
                        sums = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
                        for s in range(S):
                            rays, rng = r.camera_rays(cam, 7, s, as_torch=True)
                            r.radiance(rays, 7, 1, a.depth, cam.background, rng=rng, radiance=sums)
                            kms.append(r.get_query_stats().kernel_ms)
                        return sums

                    rays0, _ = r.camera_rays(cam, 7, 0, as_torch=True)
                    ms_f, sums_f = timed(fused, a.repeats)
                    k_f = sum(kms[-S:])
                    st = r.get_query_stats()
                    ms_s, _ = timed(lambda: r.radiance(rays0, 7, S, a.depth, cam.background), a.repeats)
                    st_s = r.get_query_stats()
                    ms_c, sums_c = timed(lambda: r.render_wavefront_batched(cam, 7, 0, S, as_torch=True), a.repeats)
                    st_c = r.get_query_stats()
                    ms_r, sums_r = timed(lambda: r.render(cam, 7), a.repeats)
                    st_r = r.stats
                    f, c = sums_f.cpu().numpy().reshape(-1), sums_c.cpu().numpy().reshape(-1)
                    same_c = bool(np.array_equal(f, c, equal_nan=True))
                    same_r = bool(np.array_equal(f, np.asarray(sums_r).reshape(-1), equal_nan=True))
                    line = {"scene": sname, "dtype": pname, "rays": n, "samples": S, "depth": a.depth,
                            "fused_ms": round(ms_f, 3), "seeded_ms": round(ms_s, 3),
                            "composition_ms": round(ms_c, 3), "render_ms": round(ms_r, 3),
                            "composition_over_fused": round(ms_c / ms_f, 3), "fused_over_render": round(ms_f / ms_r, 3),
                            "fused_kernel_ms": round(k_f, 3), "seeded_kernel_ms": round(st_s.kernel_ms, 3),
                            "composition_device_ms": round(st_c.kernel_ms, 3), "render_kernel_ms": round(st_r.kernel_ms, 3),
                            "segments": int(st_c.rays), "seeded_segments": int(st_s.rays),
                            "fused_gsegments_per_s": round(st_c.rays / ms_f / 1e6, 3),
                            "seeded_gsegments_per_s": round(st_s.rays / ms_s / 1e6, 3),
                            "composition_gsegments_per_s": round(st_c.rays / ms_c / 1e6, 3),
                            "render_gsegments_per_s": round(st_r.segments / ms_r / 1e6, 3),
                            "kernel": int(st.kernel), "same_sums_as_composition": same_c, "same_sums_as_render": same_r,
                            "fused_peak_bytes": peak(fused),
                            "seeded_peak_bytes": peak(lambda: r.radiance(rays0, 7, S, a.depth, cam.background)),
                            "input_bytes": rays0.numel() * rays0.element_size()}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    del sums_f, sums_c, sums_r, rays0
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
