#!/usr/bin/env python3
"""What adaptive sampling (rtw_render_adaptive_device) buys and costs on the
C2 frame: 1200 x 800, depth 50, min 32 / window 32 / max 500.  Each setting in
its own process with a fresh Renderer, W warm-up renders, then K renders timed
by a host clock that ends in a device synchronise:

  a tolerance (0, 1/256, 1/128, 1/64 by default): wall time, samples rendered,
      passes, the histogram of tile counts, Msamples/s, and the RMS difference
      of the displayed value sqrt(sum / count) from a fixed 2000-spp render of
      another seed (so the two share no sample);
  "fixed": the one-shot render at max samples -- its RMS from the same
      reference is what the tolerances are read against;
  "window": the fixed render in sample windows of `window` samples (tuning
      "window"): at tolerance 0 the adaptive render does the same passes plus
      its machinery -- per pass a stream synchronisation with an 8-byte
      read-back, the compaction and the statistic in the fold -- so the two
      Msamples/s figures are the machinery's cost.

  --virtual N: every setting on N virtual ranks of the one GPU
      (rtw_create_virtual; the adaptive settings through
      rtw_render_adaptive_image_device).  Against the same run without it this is
      the cost of the n-rank orchestration, the gather and the assembly; the
      ranks share the GPU, so it is no scaling figure.

    python tools/adaptive_bench.py [--tolerances 0,0.00390625,0.0078125,0.015625] [--precision f64]
                                   [--size 1200x800] [--samples 32,32,500] [--ref-spp 2000] [--rounds 1]
                                   [--virtual N]
    python tools/adaptive_bench.py --one SETTING --ref FILE      (internal: one measurement)
"""
import argparse
import collections
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH, SEED, REF_SEED = 50, 1000, 777000


def _setup(precision, size, spp):
    sys.path.insert(0, ROOT)
    import ray_tracing_weekend_amd as rtw
    prec = rtw.RTW_F64 if precision == "f64" else rtw.RTW_F32
    scene, b = rtw.scenes.simple_soa(0x5EED0001)
    cam = b.with_image_width(size[0]).with_image_height(size[1]).with_samples_per_pixel(spp).with_max_depth(DEPTH).build()
    return rtw, prec, scene, cam


def _rms(shown, ref):
    import numpy as np
    ok = np.isfinite(shown).all(-1) & np.isfinite(ref).all(-1)
    return float(np.sqrt(np.mean((shown[ok] - ref[ok]) ** 2)))


def reference(path, precision, size, ref_spp):
    """The displayed values sqrt(sum / spp) of a ref_spp render of another seed -> path (.npy)."""
    import numpy as np
    rtw, prec, scene, cam = _setup(precision, size, ref_spp)
    with rtw.Renderer(device=0, precision=prec) as r:
        r.set_tuning("window", 250)        # (bounded chunk sums at any ref_spp)
        r.set_scene(scene)
        sums = r.render(cam, REF_SEED)
    with np.errstate(all="ignore"):
        np.save(path, np.sqrt(sums / ref_spp))


def one(setting, precision, steps, warmup, size, samples, ref_path, virtual=0):
    import numpy as np
    import torch
    mn, win, mx = samples
    rtw, prec, scene, cam = _setup(precision, size, mx)
    w, h = size
    ref = np.load(ref_path)
    out = {"setting": setting, "precision": precision, "size": f"{w}x{h}", "min_window_max": list(samples),
           "virtual_ranks": virtual}
    with rtw.Renderer(device=0, precision=prec, virtual_ranks=virtual or None) as r:
        if setting == "window":
            r.set_tuning("window", win)
        r.set_scene(scene)
        if setting in ("fixed", "window"):
            img = torch.empty((h, w, 3), dtype=torch.float64 if precision == "f64" else torch.float32, device="cuda:0")
            nbytes = img.numel() * img.element_size()

            def go(seed):
                r.render_image_device(cam, seed, img.data_ptr(), nbytes)
        else:
            d_sums = torch.empty((h, w, 3), dtype=torch.float64, device="cuda:0")
            d_counts = torch.empty((h, w), dtype=torch.int32, device="cuda:0")

            def go(seed):
                r.render_adaptive_device(cam, seed, mn, mx, win, float(setting), d_sums.data_ptr(),
                                         d_sums.numel() * 8, d_counts.data_ptr(), d_counts.numel() * 4)
        for k in range(warmup):
            go(SEED + 100 + k)
        torch.cuda.synchronize()
        wall = []
        for k in range(steps):
            t0 = time.perf_counter()
            go(SEED if k == steps - 1 else SEED + 1 + k)     # the last render is the one reported
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        st = r.get_stats()
        n_samples, kernel_ms = int(st.samples), float(st.kernel_ms)
        if setting in ("fixed", "window"):
            sums = img.double().cpu().numpy()
            counts = np.full((h, w), mx, np.uint32)
        else:
            sums, counts = d_sums.cpu().numpy(), d_counts.cpu().numpy().astype(np.uint32)
    ends = [min(mn + k * win, mx) for k in range(1 + -(-(mx - mn) // win))]
    tiles = counts[::8, ::8]
    with np.errstate(all="ignore"):
        shown = np.sqrt(sums / counts[..., None])
    wall_ms = sum(wall) / len(wall)
    out.update({"wall_ms": round(wall_ms, 3), "wall_min_ms": round(min(wall), 3), "kernel_ms": round(kernel_ms, 3),
                "samples": n_samples, "msamples_per_s": round(n_samples / min(wall) / 1e3, 1),
                "passes": 1 if setting == "fixed" else ends.index(int(counts.max())) + 1,
                "tile_counts": sorted(collections.Counter(int(c) for c in tiles.ravel()).items()),
                "mean_count": round(float(counts.mean()), 2), "rms_vs_ref": round(_rms(shown, ref), 6)})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tolerances", default="0,0.00390625,0.0078125,0.015625")
    ap.add_argument("--precision", choices=["f32", "f64"], default="f64")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", default="1200x800")
    ap.add_argument("--samples", default="32,32,500", help="min,window,max")
    ap.add_argument("--ref-spp", type=int, default=2000)
    ap.add_argument("--virtual", type=int, default=0, help="N virtual ranks on the one GPU (0: a one-device context)")
    ap.add_argument("--one")
    ap.add_argument("--ref")
    a = ap.parse_args()
    size = tuple(int(x) for x in a.size.split("x"))
    samples = tuple(int(x) for x in a.samples.split(","))
    if a.one == "reference":
        reference(a.ref, a.precision, size, a.ref_spp)
        return
    if a.one is not None:
        one(a.one, a.precision, a.steps, a.warmup, size, samples, a.ref, a.virtual)
        return
    with tempfile.TemporaryDirectory() as d:
        ref = os.path.join(d, "ref.npy")
        common = ["--precision", a.precision, "--steps", str(a.steps), "--warmup", str(a.warmup), "--size", a.size,
                  "--samples", a.samples, "--ref-spp", str(a.ref_spp), "--ref", ref, "--virtual", str(a.virtual)]
        subprocess.run([sys.executable, __file__, "--one", "reference", *common], check=True, timeout=900)
        for rd in range(a.rounds):
            for setting in ["fixed", "window", *a.tolerances.split(",")]:
                out = subprocess.run([sys.executable, __file__, "--one", setting, *common], capture_output=True,
                                     text=True, timeout=900)
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
                if out.returncode != 0 or not line:
                    print(json.dumps({"setting": setting, "error": out.stderr[-500:]}), flush=True)
                    sys.exit(1)
                print(json.dumps({"round": rd, **json.loads(line[-1])}), flush=True)


if __name__ == "__main__":
    main()
