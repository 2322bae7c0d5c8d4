#!/usr/bin/env python3
"""What sample windows (tuning "window") cost: the C2 frame rendered one-shot
and in windows, each setting in its own process with a fresh Renderer, W
warm-up renders, then K renders timed two ways -- kernel_ms from the library's
HIP events around the whole render (every window's kernel and fold), step_ms
from a host clock around the K renders ending in a device synchronise -- and
the chunk-sum bytes the setting needs (ceil(window / chunk) x tiles x 64 x 3 x
element size; the f64 accumulator of a window render adds tiles x 64 x 3 x 8).

    python tools/window_bench.py [--windows 0,100,250,-1] [--precision f64] [--size 1200x800x500]
                                 [--tuning partial_max=2147483648] [--rounds 2]
    python tools/window_bench.py --one WINDOW      (internal: one measurement)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH = 1200, 800, 500, 50


def one(window, precision, steps, warmup, size, tuning):
    sys.path.insert(0, ROOT)
    import torch
    import ray_tracing_weekend_amd as rtw
    prec = rtw.RTW_F64 if precision == "f64" else rtw.RTW_F32
    esz = 8 if precision == "f64" else 4
    w, h, spp = size
    scene, b = rtw.scenes.simple_soa(0x5EED0001)
    cam = b.with_image_width(w).with_image_height(h).with_samples_per_pixel(spp).with_max_depth(DEPTH).build()
    tiles = rtw.tiles_for_rank(w, h, 0, 1)
    with rtw.Renderer(device=0, precision=prec) as r:
        for k, v in tuning.items():
            r.set_tuning(k, int(v))
        r.set_tuning("window", window)
        r.set_scene(scene)
        buf = torch.empty((tiles * 64 * 3,), dtype=torch.float64 if esz == 8 else torch.float32, device="cuda:0")
        nbytes = buf.numel() * buf.element_size()
        for k in range(warmup):
            r.render_device(cam, 1000 + k, buf.data_ptr(), nbytes)
        torch.cuda.synchronize()
        kernel_ms = []
        t0 = time.perf_counter()
        for k in range(steps):
            r.render_device(cam, 1000 + warmup + k, buf.data_ptr(), nbytes)
            kernel_ms.append(r.get_stats().kernel_ms)      # waits for the render
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t0) * 1e3 / steps
        got = len(r.get_timings(64)[0])                    # one entry per pass, the last 64 at most
        windows = got // (warmup + steps) if got < 64 else None
        chunk = int(r.stats.chunk)
        checksum = float(torch.nan_to_num(buf.double()).sum().item())
    # the samples whose chunk sums are held at once (an auto window's length is
    # the plan's: not reported by the library, so no byte count then)
    per = spp if windows == 1 else (window if windows and window > 0 else None)
    print(json.dumps({"window": window, "precision": precision, "tuning": tuning, "chunk": chunk, "passes": windows,
                      "kernel_ms": round(sum(kernel_ms) / len(kernel_ms), 3), "kernel_min_ms": round(min(kernel_ms), 3),
                      "step_ms": round(step_ms, 3),
                      "chunk_sum_bytes": None if per is None else -(-per // chunk) * tiles * 64 * 3 * esz,
                      "accumulator_bytes": 0 if not windows or windows == 1 else tiles * 64 * 3 * 8,
                      "image_checksum": checksum}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="0,100,250,-1")
    ap.add_argument("--precision", choices=["f32", "f64"], default="f64")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", default=f"{W}x{H}x{SPP}")
    ap.add_argument("--tuning", default="", help="k=v,... (rtw_set_tuning), applied before the window")
    ap.add_argument("--one", type=int)
    a = ap.parse_args()
    size = tuple(int(x) for x in a.size.split("x"))
    tuning = dict(kv.split("=") for kv in filter(None, a.tuning.split(",")))
    if a.one is not None:
        one(a.one, a.precision, a.steps, a.warmup, size, tuning)
        return
    for rd in range(a.rounds):
        for win in a.windows.split(","):
            out = subprocess.run([sys.executable, __file__, "--one", win, "--precision", a.precision, "--steps",
                                  str(a.steps), "--warmup", str(a.warmup), "--size", a.size, "--tuning", a.tuning],
                                 capture_output=True, text=True, timeout=900)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
            if out.returncode != 0 or not line:
                print(json.dumps({"window": win, "error": out.stderr[-500:]}), flush=True)
                sys.exit(1)
            print(json.dumps({"round": rd, **json.loads(line[-1])}), flush=True)


if __name__ == "__main__":
    main()
