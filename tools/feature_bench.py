#!/usr/bin/env python3
"""What the feature pass (rtw_render_features_device) costs on C2 -- the Book-1
final scene, 1200 x 800, 500 samples -- in both precisions, against two scales
measured in the same command:

  render      the render step of the same camera on the same build
              (rtw_stats.kernel_ms): the pass traces one segment of its several
  hit_rays    rtw_hit_rays_device over 1200 x 800 x `--ray-samples` pre-generated
              primary rays of the same camera (jittered pixel positions, image
              order): the unfused alternative, in Mrays/s, without the cost of
              shipping rays in and records out or of folding them

Timing: the library's device events around each kernel (rtw_query_stats.kernel_ms,
rtw_stats.kernel_ms), one warm-up round, then `--repeats` rounds that visit the
three in turn; medians with the spread.  One JSON line per precision, then one
with the differences between the f32 and the f64 features (written down, not
gated: no bound can be derived): the share of pixels whose sample-0 id differs,
and the largest albedo-mean difference on pixels where the ids agree.

  python tools/feature_bench.py [--spp 500] [--repeats 3] [--ray-samples 4] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ray_tracing_weekend_amd as rtw  # noqa: E402

SEED = 0x5EED0001
W, H = 1200, 800


def primary_rays(cam, samples, dtype, dev):
    """samples jittered primary rays per pixel, pixel-major in image order: [H * W * samples, 6]"""
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    n = cam.image_height * cam.image_width * samples
    k = torch.arange(n, device=dev) // samples
    i = (k % cam.image_width).double() + torch.rand(n, generator=g, device=dev, dtype=torch.float64) - 0.5
    j = (k // cam.image_width).double() + torch.rand(n, generator=g, device=dev, dtype=torch.float64) - 0.5
    t = lambda v: torch.tensor(list(v), dtype=torch.float64, device=dev)   # noqa: E731
    tgt = t(cam.pixel00_loc) + i[:, None] * t(cam.pixel_delta_u) + j[:, None] * t(cam.pixel_delta_v)
    c = t(cam.center).expand_as(tgt)
    return torch.cat([c, tgt - c], 1).to(dtype).contiguous()


def med(v):
    v = np.asarray(v, np.float64)
    return round(float(np.median(v)), 4), [round(float(v.min()), 4), round(float(v.max()), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ray-samples", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    soa, b = rtw.scenes.simple_soa(SEED, 11)
    cam = b.with_image_width(W).with_image_height(H).with_samples_per_pixel(a.spp).with_max_depth(50).build()
    lines, kept = [], {}
    for pname, prec, dtype in (("f64", rtw.RTW_F64, torch.float64), ("f32", rtw.RTW_F32, torch.float32)):
        rays = primary_rays(cam, a.ray_samples, dtype, dev)
        feat = torch.zeros((H, W, 8), dtype=torch.float64, device=dev)
        t_feat, t_render, t_rays = [], [], []
        with rtw.Renderer(device=0, precision=prec) as r:
            r.set_scene(soa)
            for rep in range(1 + a.repeats):            # rep 0: warm-up
                _, ids = r.render_features(cam, 7, 0, a.spp, features=feat)
                fs = r.get_query_stats()
                stats = (int(fs.rays), int(fs.hits), int(fs.kernel), fs.node_visits / max(fs.rays, 1))
                r.render(cam, 7)
                render_ms, kernel = r.stats.kernel_ms, r.last_kernel()
                r.hit_rays(rays)
                qs = r.get_query_stats()
                if rep:
                    t_feat.append(fs.kernel_ms)
                    t_render.append(render_ms)
                    t_rays.append(qs.kernel_ms)
            torch.cuda.synchronize()
        kept[pname] = (feat.cpu().numpy(), ids.cpu().numpy())
        n_rays, hits, world, visits = stats
        f_ms, f_spread = med(t_feat)
        r_ms, r_spread = med(t_render)
        q_ms, q_spread = med(t_rays)
        lines.append({"config": "C2", "dtype": pname, "width": W, "height": H, "spp": a.spp, "world": world,
                      "features_ms": f_ms, "features_ms_spread": f_spread, "rays": n_rays,
                      "features_mrays_per_s": round(n_rays / f_ms / 1e3, 1), "hit_share": round(hits / n_rays, 4),
                      "node_visits_per_ray": round(visits, 2),
                      "render_ms": r_ms, "render_ms_spread": r_spread, "render_kernel": list(kernel),
                      "features_over_render": round(f_ms / r_ms, 4),
                      "hit_rays": len(rays), "hit_rays_ms": q_ms, "hit_rays_ms_spread": q_spread,
                      "hit_rays_mrays_per_s": round(len(rays) / q_ms / 1e3, 1),
                      "features_over_hit_rays_rate": round((n_rays / f_ms) / (len(rays) / q_ms), 3)})
        print(json.dumps(lines[-1]), flush=True)
        del rays, feat
    (f64, i64), (f32, i32) = kept["f64"], kept["f32"]
    agree = (i64 == i32).all(-1)
    diff = np.abs(f64[..., :3] - f32[..., :3]) / a.spp
    lines.append({"config": "C2", "f32_against_f64": True, "spp": a.spp,
                  "sample0_id_differs_share": round(float(1.0 - agree.mean()), 6),
                  "max_albedo_mean_difference_where_ids_agree": float(diff[agree].max()),
                  "mean_albedo_mean_difference": float(diff.mean())})
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
