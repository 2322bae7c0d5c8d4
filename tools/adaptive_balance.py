#!/usr/bin/env python3
"""How well static tile ownership balances an adaptive render over n ranks,
computed on the CPU from ONE one-device adaptive render's counts (the n-rank
render gives the same counts bit for bit, so nothing here needs n GPUs).

The C2 frame (1200 x 800, depth 50, min 32 / window 32 / max 500) is rendered
adaptively per tolerance (1/64 and 1/32 by default) and once fixed, to read the
tile costs the context counts for its longest-first order (rtw_tile_costs: BVH
node visits + sphere tests + 12 per segment of each pixel's first samples -- a
cost per sample of the tile, in arbitrary units).  For n = 2, 4, 8 ranks under
the round robin (tile T to rank T mod n) one JSON line each:

  samples:   per-rank sum of counts over the rank's pixels, and max / mean;
  work:      the same with each tile's samples weighted by its cost;
  passes:    per pass the ranks' active-tile counts as max / mean, the number
             of ranks without an active tile, and the same weighted by cost;
  lockstep:  sum over passes of the slowest rank's weighted work over the sum
             of the mean rank's -- what waiting for the slowest rank in every
             pass costs against perfectly balanced passes, by this cost model
             (not a measured time).

    python tools/adaptive_balance.py [--tolerances 0.015625,0.03125] [--ranks 2,4,8] [--precision f64]
                                     [--size 1200x800] [--samples 32,32,500]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH, SEED = 50, 1000


def balance(tile_count, tile_px, tile_cost, ends, n):
    """The figures of one (counts, n): see the module docstring."""
    import numpy as np
    samples = tile_count.astype(np.float64) * tile_px
    work = samples * tile_cost
    rank = np.arange(tile_count.size) % n
    per = lambda v: np.array([v[rank == k].sum() for k in range(n)])    # noqa: E731
    ratio = lambda v: round(float(v.max() / v.mean()), 4) if v.mean() else None    # noqa: E731
    s, w = per(samples), per(work)
    passes, slow, mean = [], 0.0, 0.0
    first = 0
    for e in ends:
        on = tile_count >= e
        if not on.any():
            break
        tiles = per(on.astype(np.float64))
        pw = per(on * tile_px * tile_cost * (e - first))
        passes.append({"end": int(e), "active": int(on.sum()), "tiles_max_over_mean": ratio(tiles),
                       "idle_ranks": int((tiles == 0).sum()), "work_max_over_mean": ratio(pw)})
        slow += float(pw.max())
        mean += float(pw.mean())
        first = e
    return {"ranks": n, "samples_per_rank": [int(x) for x in s], "samples_max_over_mean": ratio(s),
            "work_max_over_mean": ratio(w), "passes": passes,
            "lockstep_over_balanced": round(slow / mean, 4) if mean else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tolerances", default="0.015625,0.03125")
    ap.add_argument("--ranks", default="2,4,8")
    ap.add_argument("--precision", choices=["f32", "f64"], default="f64")
    ap.add_argument("--size", default="1200x800")
    ap.add_argument("--samples", default="32,32,500", help="min,window,max")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import ray_tracing_weekend_amd as rtw
    w, h = (int(x) for x in a.size.split("x"))
    mn, win, mx = (int(x) for x in a.samples.split(","))
    prec = rtw.RTW_F64 if a.precision == "f64" else rtw.RTW_F32
    scene, b = rtw.scenes.simple_soa(0x5EED0001)
    cam = b.with_image_width(w).with_image_height(h).with_samples_per_pixel(mx).with_max_depth(DEPTH).build()
    ends = [min(mn + k * win, mx) for k in range(1 + -(-(mx - mn) // win))]
    tile_px = np.array([min(8, w - tx) * min(8, h - ty) for ty in range(0, h, 8) for tx in range(0, w, 8)], np.float64)
    with rtw.Renderer(device=0, precision=prec) as r:
        r.set_scene(scene)
        r.render(cam, SEED)                               # the fixed render counts the tile costs
        cost = r.tile_costs(cam).astype(np.float64)
        cost /= tile_px                                   # per pixel sample, whatever the tile's size
        for tol in (float(t) for t in a.tolerances.split(",")):
            _, counts = r.render_adaptive(cam, SEED, mn, mx, win, tol)
            tile_count = counts[::8, ::8].reshape(-1)
            for n in (int(x) for x in a.ranks.split(",")):
                print(json.dumps({"tolerance": tol, "size": f"{w}x{h}", "min_window_max": [mn, win, mx],
                                  "precision": a.precision, "total_samples": int(counts.astype(np.uint64).sum()),
                                  **balance(tile_count, tile_px, cost, ends, n)}), flush=True)


if __name__ == "__main__":
    main()
