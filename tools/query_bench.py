#!/usr/bin/env python3
"""Throughput of the batched closest-hit query (rtw_hit_rays_device), in Mrays/s,
on the C2 scene (scenes::simple, 484 spheres) and a C3-sized field (10k
spheres), for every world and both precisions, on two ray sets:

  coherent    camera rays in image order (neighbouring lanes, neighbouring pixels)
  incoherent  rays leaving the coherent set's first hits: a seeded cosine
              direction about the query's own normal, from the query's own point

against the render's whole-segment rate on the same scene (rtw_stats.segments /
kernel_ms of a short render): a segment is a closest hit plus the hit record,
the scatter and the light pdf, but the render refills its lanes from an item
pool while a query's wave waits for its slowest ray.

Timing: the library's device events around the query kernel
(rtw_query_stats.kernel_ms), one warm-up, then `--repeats` rounds that visit
every configuration in turn (alternated, so that drift hits all alike); the
median is reported with the spread.  One JSON line per configuration.

  python tools/query_bench.py [--rays 4194304] [--repeats 3] [--scenes C2,C3] [--out FILE]
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
SCENES = {"C2": dict(n=11, w=1200, h=800, spp=128), "C3": dict(n=50, w=1920, h=1080, spp=32)}
WORLDS = [("brute lds 0", rtw.RTW_ACCEL_BRUTE, {"lds": 0}), ("brute lds 1", rtw.RTW_ACCEL_BRUTE, {"lds": 1}),
          ("bvh_kind 0", rtw.RTW_ACCEL_BVH, {"bvh_kind": 0}), ("bvh_kind 1", rtw.RTW_ACCEL_BVH, {"bvh_kind": 1}),
          ("bvh_kind 2", rtw.RTW_ACCEL_BVH, {"bvh_kind": 2}), ("bvh_kind 3", rtw.RTW_ACCEL_BVH, {"bvh_kind": 3})]
BRUTE_SHARE = 16      # the brute-force sweeps run rays / 16 (10k spheres per ray on C3)


def camera_rays(cam, n, dtype, dev):
    """n rays through a sqrt(n)-wide grid of sub-pixel positions of the image, row by row"""
    side = int(round(n ** 0.5))
    k = torch.arange(side * side, device=dev)
    i = (k % side).double() * (cam.image_width / side)
    j = (k // side).double() * (cam.image_height / side)
    t = lambda v: torch.tensor(list(v), dtype=torch.float64, device=dev)   # noqa: E731
    tgt = t(cam.pixel00_loc) + i[:, None] * t(cam.pixel_delta_u) + j[:, None] * t(cam.pixel_delta_v)
    c = t(cam.center).expand_as(tgt)
    return torch.cat([c, tgt - c], 1).to(dtype).contiguous()


def bounce_rays(hits, ids, n, dtype, dev):
    """n rays from the hits' points along a seeded cosine direction about their normals"""
    g = torch.Generator(device=dev)
    g.manual_seed(12345)
    hit = torch.nonzero(ids[:, 0] >= 0)[:, 0]
    pick = hit[torch.randint(len(hit), (n,), generator=g, device=dev)]
    p, nrm = hits[pick, 1:4].double(), hits[pick, 4:7].double()
    r1, r2 = torch.rand(n, generator=g, device=dev, dtype=torch.float64), \
        torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    phi = 2 * np.pi * r2
    loc = torch.stack([torch.cos(phi) * torch.sqrt(r1), torch.sin(phi) * torch.sqrt(r1), torch.sqrt(1 - r1)], 1)
    w = nrm / nrm.norm(dim=1, keepdim=True)
    a = torch.where((w[:, 0].abs() > 0.9)[:, None], torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=dev),
                    torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device=dev))
    v = torch.linalg.cross(w, a)
    v = v / v.norm(dim=1, keepdim=True)
    u = torch.linalg.cross(w, v)
    d = loc[:, :1] * u + loc[:, 1:2] * v + loc[:, 2:] * w
    return torch.cat([p, d], 1).to(dtype).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=3)
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
        for pname, prec, dtype in (("f32", rtw.RTW_F32, torch.float32), ("f64", rtw.RTW_F64, torch.float64)):
            # the yardstick: the render's segments per ms on this scene
            with rtw.Renderer(device=0, precision=prec) as r:
                r.set_scene(soa)
                rates = []
                for k in range(1 + a.repeats):
                    r.render(cam, 7 + k)
                    if k:
                        rates.append(r.stats.segments / r.stats.kernel_ms / 1e3)
                render_rate = float(np.median(rates))
                render_kernel = r.last_kernel()
            coherent = camera_rays(cam, a.rays, dtype, dev)
            rs = []
            for wname, accel, tuning in WORLDS:
                r = rtw.Renderer(device=0, precision=prec)
                for key, v in tuning.items():
                    r.set_tuning(key, v)
                r.set_accel(accel)
                r.set_scene(soa)
                rs.append(r)
            hits, ids = rs[-1].hit_rays(coherent)
            sets = {"coherent": coherent, "incoherent": bounce_rays(hits, ids, a.rays, dtype, dev)}
            del hits, ids
            ms = {(w[0], s): [] for w in WORLDS for s in sets}
            info = {}
            for rep in range(1 + a.repeats):            # rep 0: warm-up
                for (wname, accel, _), r in zip(WORLDS, rs):
                    for s, rays in sets.items():
                        sub = rays[: len(rays) // BRUTE_SHARE] if accel == rtw.RTW_ACCEL_BRUTE else rays
                        r.hit_rays(sub)
                        st = r.get_query_stats()
                        if rep:
                            ms[(wname, s)].append(st.kernel_ms)
                        info[(wname, s)] = (len(sub), int(st.kernel), st.hits / max(st.rays, 1),
                                            st.node_visits / max(st.rays, 1), st.sphere_tests / max(st.rays, 1))
            for r in rs:
                r.close()
            for (wname, s), t in ms.items():
                n, kernel, hit_share, nv, nt = info[(wname, s)]
                rate = n / np.array(t) / 1e3
                lines.append({"scene": sname, "spheres": len(soa.sphere_mat), "dtype": pname, "tuning": wname,
                              "world": kernel, "rays_set": s, "rays": n, "mrays_per_s": round(float(np.median(rate)), 1),
                              "spread": [round(float(rate.min()), 1), round(float(rate.max()), 1)],
                              "kernel_ms": round(float(np.median(t)), 4), "hit_share": round(hit_share, 4),
                              "node_visits_per_ray": round(nv, 2), "sphere_tests_per_ray": round(nt, 2),
                              "render_msegments_per_s": round(render_rate, 1), "render_kernel": list(render_kernel),
                              "ratio_to_render": round(float(np.median(rate)) / render_rate, 3)})
                print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
