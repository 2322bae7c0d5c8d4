#!/usr/bin/env python3
"""What the denoiser (rtw_denoise_device) costs and buys.  Each setting runs in
its own process with a fresh Renderer: the render and the feature pass of the
workload once (their device times are the scales), a warm-up denoise, then
`--repeats` denoises timed by the library's device events
(rtw_denoise_stats.kernel_ms: prepare + iterations + finish).

Workloads: C2 -- scenes::simple at 1200 x 800 -- at 16, 32, 64 and 500 spp, and
cornell_box at 600 x 600 at 16 and 64 spp, all f64 (the filter's arithmetic does
not depend on the precision), depth 50.

  pass     the whole pass with the library's defaults and the default plan, as a share of the render step
           and of the feature pass of the same command; the bytes the algorithm
           must move (96 B per pixel and iteration: two 32-byte records read, one
           written) over the time of the iterations, against the HBM and
           Infinity-Cache rates; and the quality: the RMS of sqrt(mean) against a
           2000-spp render of another seed over the pixels finite in both, noisy
           against denoised, with the filled count.
  ab       tuning denoise_lds 0 against 2 in alternating rounds of one process,
           at iterations 1..5: the time of step 2^k is the pass at k + 1
           iterations minus the pass at k.  The default plan stages what this
           shows to be faster (host/denoise_plan.hpp kDenoiseLdsDefaultMaxStep).
  sweep    sigma_colour {0.5, 1, 2, 0} x normal_power_log2 {3, 5} at the low
           sample counts: the RMS after the filter, which picks the defaults.
  kernels  `rocprofv3 --kernel-trace --stats` around one `pass` process, a run of
           its own: the time of each denoise kernel.
  vpass    the variance-guided filter (rtw_denoise_variance_device) next to the old
           one in one process, alternating, on the sums and moments of one
           rtw_render_window_moments_device call: both passes' times, and the
           quality of the old filter and of the new one at sigma_var {1, 1.5, 2,
           3, 4} against the same reference.
  vab      `ab` for the variance-guided filter: it stages up to step 4.
  moments  rtw_render_window_moments against rtw_render_window, the workload's
           samples in one window, alternating rounds of one process (kernel_ms of
           the render stats: the render kernel and its folds).

    python tools/denoise_bench.py [--what pass,ab,sweep,kernels,vpass,vab,moments] [--repeats 5] [--ref-spp 2000] [--out FILE]
    python tools/denoise_bench.py --one KIND --workload NAME:WxH:SPP ...   (internal: one measurement)
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, REF_SEED, DEPTH = 1000, 777000, 50
WORKLOADS = ["simple:1200x800:16", "simple:1200x800:32", "simple:1200x800:64", "simple:1200x800:500",
             "cornell_box:600x600:16", "cornell_box:600x600:64"]
# MI355X: HBM3E 8.0 TB/s peak (about 6.3 TB/s achievable); gathers served by the Infinity Cache 8.6 TB/s
HBM_BYTES_PER_S, INFINITY_CACHE_BYTES_PER_S = 8.0e12, 8.6e12
# the parameters the sweep and the a/b vary from (the filter's start values)
START = dict(iterations=5, normal_power_log2=5, sigma_colour=1.0, sigma_depth=0.125, demodulate=1, fill_nonfinite=1)


def parse(workload):
    name, size, spp = workload.split(":")
    w, h = (int(x) for x in size.split("x"))
    return name, w, h, int(spp)


def setup(workload, spp=None):
    sys.path.insert(0, ROOT)
    import ray_tracing_weekend_amd as rtw
    name, w, h, wspp = parse(workload)
    scene, b = rtw.scenes.named_soa(name, 0x5EED0001)
    cam = b.with_image_width(w).with_image_height(h).with_samples_per_pixel(spp or wspp).with_max_depth(DEPTH).build()
    return rtw, scene, cam


def reference(path, workload, ref_spp):
    """The per-sample means of a ref_spp render of another seed -> path (.npy)."""
    import numpy as np
    rtw, scene, cam = setup(workload, ref_spp)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_tuning("window", 250)        # (bounded chunk sums at any ref_spp)
        r.set_scene(scene)
        np.save(path, r.render(cam, REF_SEED) / ref_spp)


def inputs(rtw, r, cam):
    """(d_sums, d_features, render_ms, features_ms) of the workload on the device."""
    import torch
    h, w = cam.image_height, cam.image_width
    d_sums = torch.empty((h, w, 3), dtype=torch.float64, device="cuda:0")
    r.render_image_device(cam, SEED, d_sums.data_ptr(), d_sums.numel() * 8)
    render_ms = float(r.get_stats().kernel_ms)
    d_feat = torch.zeros((h, w, 8), dtype=torch.float64, device="cuda:0")
    r.render_features(cam, SEED, features=d_feat, want_ids=False)
    return d_sums, d_feat, render_ms, float(r.get_query_stats().kernel_ms)


def rms(mean, ref, ok):
    import numpy as np
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.mean((np.sqrt(mean[ok]) - np.sqrt(ref[ok])) ** 2)))


def med(v):
    import numpy as np
    v = np.asarray(v, np.float64)
    return round(float(np.median(v)), 4), [round(float(v.min()), 4), round(float(v.max()), 4)]


def one_pass(workload, repeats, ref_path, params):
    import numpy as np
    rtw, scene, cam = setup(workload)
    params = rtw.DenoiseParams(**params).as_dict()      # the library's defaults where nothing is given
    name, w, h, spp = parse(workload)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(scene)
        d_sums, d_feat, render_ms, feat_ms = inputs(rtw, r, cam)
        times, first = [], []
        for rep in range(1 + repeats):                  # rep 0: warm-up
            out = r.denoise(d_sums, d_feat, spp, **params)
            st = r.denoise_stats()
            if rep:
                times.append(st.kernel_ms)
            one = r.denoise(d_sums, d_feat, spp, **dict(params, iterations=1))
            if rep:
                first.append(r.denoise_stats().kernel_ms)
        sums, mean = d_sums.cpu().numpy(), out.cpu().numpy()
        del one
    ms, spread = med(times)
    ms1, _ = med(first)
    it = params["iterations"]
    line = {"what": "pass", "workload": workload, "params": params, "denoise_ms": ms, "denoise_ms_spread": spread,
            "lds_iterations": int(st.lds_iterations), "render_ms": round(render_ms, 3),
            "features_ms": round(feat_ms, 3), "denoise_over_render": round(ms / render_ms, 5),
            "denoise_over_features": round(ms / feat_ms, 4), "filled": int(st.filled),
            "left_nonfinite": int(st.left_nonfinite)}
    if it > 1:
        # the iterations after the first: the pass minus a one-iteration pass
        per_iter_ms = (ms - ms1) / (it - 1)
        rate = 96.0 * w * h / (per_iter_ms * 1e-3) if per_iter_ms > 0 else 0.0
        line.update({"iteration_ms": round(per_iter_ms, 4), "algorithmic_bytes_per_s": round(rate, -9),
                     "share_of_hbm_rate": round(rate / HBM_BYTES_PER_S, 3),
                     "share_of_infinity_cache_rate": round(rate / INFINITY_CACHE_BYTES_PER_S, 3)})
    if ref_path:
        ref = np.load(ref_path)
        noisy = sums / spp
        ok = np.isfinite(noisy).all(-1) & np.isfinite(ref).all(-1) & np.isfinite(mean).all(-1)
        line.update({"nonfinite_in": int((~np.isfinite(noisy).all(-1)).sum()), "rms_noisy": round(rms(noisy, ref, ok), 6),
                     "rms_denoised": round(rms(mean, ref, ok), 6)})
    print(json.dumps(line), flush=True)


def one_ab(workload, repeats):
    rtw, scene, cam = setup(workload)
    name, w, h, spp = parse(workload)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r0, rtw.Renderer(device=0, precision=rtw.RTW_F64) as r2:
        r0.set_scene(scene)
        r0.set_tuning("denoise_lds", 0)
        r2.set_tuning("denoise_lds", 2)
        d_sums, d_feat, _, _ = inputs(rtw, r0, cam)
        t = {(lds, it): [] for lds in (0, 2) for it in range(1, 6)}
        for rep in range(1 + repeats):                  # rep 0: warm-up; the two forms alternate
            for it in range(1, 6):
                for lds, r in ((0, r0), (2, r2)) if rep % 2 else ((2, r2), (0, r0)):
                    r.denoise(d_sums, d_feat, spp, **dict(START, iterations=it))
                    if rep:
                        t[(lds, it)].append(r.denoise_stats().kernel_ms)
    line = {"what": "ab", "workload": workload, "steps": []}
    prev = {0: 0.0, 2: 0.0}
    for it in range(1, 6):
        m0, s0 = med(t[(0, it)])
        m2, s2 = med(t[(2, it)])
        line["steps"].append({"step": 1 << (it - 1), "pass_direct_ms": m0, "pass_direct_spread": s0,
                              "pass_lds_ms": m2, "pass_lds_spread": s2,
                              "step_direct_ms": round(m0 - prev[0], 4), "step_lds_ms": round(m2 - prev[2], 4)})
        prev = {0: m0, 2: m2}
    print(json.dumps(line), flush=True)


def one_sweep(workload, ref_path):
    import numpy as np
    rtw, scene, cam = setup(workload)
    name, w, h, spp = parse(workload)
    ref = np.load(ref_path)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(scene)
        d_sums, d_feat, _, _ = inputs(rtw, r, cam)
        noisy = d_sums.cpu().numpy() / spp
        ok = np.isfinite(noisy).all(-1) & np.isfinite(ref).all(-1)
        rows = []
        for m in (3, 5):
            for sc in (0.5, 1.0, 2.0, 0.0):
                mean = r.denoise(d_sums, d_feat, spp, **dict(START, sigma_colour=sc, normal_power_log2=m)).cpu().numpy()
                rows.append({"sigma_colour": sc, "normal_power_log2": m,
                             "rms_denoised": round(rms(mean, ref, ok & np.isfinite(mean).all(-1)), 6),
                             "filled": int(r.denoise_stats().filled)})
    print(json.dumps({"what": "sweep", "workload": workload, "rms_noisy": round(rms(noisy, ref, ok), 6), "rows": rows}),
          flush=True)


SIGMA_VARS = (1.0, 1.5, 2.0, 3.0, 4.0)


def moments_inputs(rtw, r, cam, spp):
    """(d_sums, d_moments, d_features) of the workload on the device, one moments window."""
    import torch
    h, w = cam.image_height, cam.image_width
    d_sums = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    d_mom = torch.zeros((h, w, 2), dtype=torch.float64, device="cuda:0")
    r.render_window_moments_device(cam, SEED, 0, spp, d_sums.data_ptr(), d_sums.numel() * 8, d_mom.data_ptr(),
                                   d_mom.numel() * 8)
    d_feat = torch.zeros((h, w, 8), dtype=torch.float64, device="cuda:0")
    r.render_features(cam, SEED, features=d_feat, want_ids=False)
    torch.cuda.synchronize()
    return d_sums, d_mom, d_feat


def one_vpass(workload, repeats, ref_path):
    import numpy as np
    rtw, scene, cam = setup(workload)
    name, w, h, spp = parse(workload)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(scene)
        d_sums, d_mom, d_feat = moments_inputs(rtw, r, cam, spp)
        t = {"old": [], "new": []}
        for rep in range(1 + repeats):                  # rep 0: warm-up; the two filters alternate
            for which in ("old", "new") if rep % 2 else ("new", "old"):
                if which == "old":
                    old = r.denoise(d_sums, d_feat, spp)
                else:
                    new = r.denoise_variance(d_sums, d_feat, d_mom, spp)
                st = r.denoise_stats()
                if rep:
                    t[which].append(st.kernel_ms)
                if which == "new":
                    lds_new = int(st.lds_iterations)
        old_ms, old_spread = med(t["old"])
        new_ms, new_spread = med(t["new"])
        line = {"what": "vpass", "workload": workload, "old_params": rtw.DenoiseParams().as_dict(),
                "new_params": rtw.DenoiseVarianceParams().as_dict(), "old_ms": old_ms, "old_ms_spread": old_spread,
                "new_ms": new_ms, "new_ms_spread": new_spread, "new_over_old": round(new_ms / old_ms, 3),
                "new_lds_iterations": lds_new}
        if ref_path:
            ref = np.load(ref_path)
            noisy = d_sums.cpu().numpy() / spp
            ok = np.isfinite(noisy).all(-1) & np.isfinite(ref).all(-1)
            old_mean = old.cpu().numpy()
            line.update({"nonfinite_in": int((~np.isfinite(noisy).all(-1)).sum()),
                         "rms_noisy": round(rms(noisy, ref, ok), 6),
                         "rms_old": round(rms(old_mean, ref, ok & np.isfinite(old_mean).all(-1)), 6), "rms_new": {}})
            for sv in SIGMA_VARS:
                mean = r.denoise_variance(d_sums, d_feat, d_mom, spp, sigma_var=sv).cpu().numpy()
                line["rms_new"][str(sv)] = round(rms(mean, ref, ok & np.isfinite(mean).all(-1)), 6)
                line["left_nonfinite"] = int(r.denoise_stats().left_nonfinite)
        del new
    print(json.dumps(line), flush=True)


def one_vab(workload, repeats):
    rtw, scene, cam = setup(workload)
    name, w, h, spp = parse(workload)
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r0, rtw.Renderer(device=0, precision=rtw.RTW_F64) as r2:
        r0.set_scene(scene)
        r0.set_tuning("denoise_lds", 0)
        r2.set_tuning("denoise_lds", 2)
        d_sums, d_mom, d_feat = moments_inputs(rtw, r0, cam, spp)
        t = {(lds, it): [] for lds in (0, 2) for it in range(1, 6)}
        staged = {}
        for rep in range(1 + repeats):                  # rep 0: warm-up; the two forms alternate
            for it in range(1, 6):
                for lds, r in ((0, r0), (2, r2)) if rep % 2 else ((2, r2), (0, r0)):
                    r.denoise_variance(d_sums, d_feat, d_mom, spp, iterations=it)
                    st = r.denoise_stats()
                    staged[(lds, it)] = int(st.lds_iterations)
                    if rep:
                        t[(lds, it)].append(st.kernel_ms)
    line = {"what": "vab", "workload": workload, "steps": []}
    prev = {0: 0.0, 2: 0.0}
    for it in range(1, 6):
        m0, s0 = med(t[(0, it)])
        m2, s2 = med(t[(2, it)])
        line["steps"].append({"step": 1 << (it - 1), "staged_with_lds_2": staged[(2, it)] == it,
                              "pass_direct_ms": m0, "pass_direct_spread": s0, "pass_lds_ms": m2, "pass_lds_spread": s2,
                              "step_direct_ms": round(m0 - prev[0], 4), "step_lds_ms": round(m2 - prev[2], 4)})
        prev = {0: m0, 2: m2}
    print(json.dumps(line), flush=True)


def one_moments(workload, repeats):
    """rtw_render_window_moments against rtw_render_window: one window of the workload's samples."""
    import numpy as np
    rtw, scene, cam = setup(workload)
    name, w, h, spp = parse(workload)
    t = {"window": [], "moments": []}
    chunk = {}
    with rtw.Renderer(device=0, precision=rtw.RTW_F64) as r:
        r.set_scene(scene)
        sums, msums, moments = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w, 2))
        for rep in range(1 + repeats):                  # rep 0: warm-up; the two entries alternate
            for which in ("window", "moments") if rep % 2 else ("moments", "window"):
                if which == "window":
                    r.render_window(cam, SEED, 0, spp, sums)
                else:
                    r.render_window_moments(cam, SEED, 0, spp, msums, moments)
                chunk[which] = int(r.stats.chunk)
                if rep:
                    t[which].append(float(r.stats.kernel_ms))
    wm, ws = med(t["window"])
    mm, ms = med(t["moments"])
    same = bool(np.all((sums == msums) | (np.isnan(sums) & np.isnan(msums))))
    print(json.dumps({"what": "moments", "workload": workload, "window_ms": wm, "window_ms_spread": ws,
                      "window_chunk": chunk["window"], "moments_ms": mm, "moments_ms_spread": ms,
                      "moments_over_window": round(mm / wm, 4), "difference_ms": round(mm - wm, 3),
                      "same_sums": same}), flush=True)


def kernels(workload, repeats):
    """rocprofv3 --kernel-trace --stats around one `pass` process: the denoise kernels' rows."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "trace", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--one", "pass", "--workload", workload, "--repeats",
               str(repeats)]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            print(json.dumps({"what": "kernels", "workload": workload, "error": run.stderr[-500:]}), flush=True)
            return None
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "denoise_" in row["Name"]:
                    rows.append({"kernel": row["Name"].split("(")[0].replace("void rtw::dev::", ""),
                                 "calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                 "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)})
        line = {"what": "kernels", "workload": workload, "rows": rows}
        print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="pass,ab,sweep,kernels")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-spp", type=int, default=2000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one")
    ap.add_argument("--workload")
    ap.add_argument("--ref")
    ap.add_argument("--params", default=None, help="JSON of denoise parameters replacing the library's defaults")
    a = ap.parse_args()
    params = json.loads(a.params) if a.params else {}
    if a.one == "reference":
        return reference(a.ref, a.workload, a.ref_spp)
    if a.one == "pass":
        return one_pass(a.workload, a.repeats, a.ref, params)
    if a.one == "ab":
        return one_ab(a.workload, a.repeats)
    if a.one == "sweep":
        return one_sweep(a.workload, a.ref)
    if a.one == "vpass":
        return one_vpass(a.workload, a.repeats, a.ref)
    if a.one == "vab":
        return one_vab(a.workload, a.repeats)
    if a.one == "moments":
        return one_moments(a.workload, a.repeats)
    what, lines = a.what.split(","), []

    def child(*args):
        run = subprocess.run([sys.executable, os.path.abspath(__file__), *args], capture_output=True, text=True, timeout=900)
        got = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
        if run.returncode != 0 or not got:
            print(json.dumps({"args": args, "error": run.stderr[-500:]}), flush=True)
            sys.exit(1)
        lines.append(json.loads(got[-1]))
        print(got[-1], flush=True)

    with tempfile.TemporaryDirectory() as d:
        refs = {}
        for wl in a.workloads.split(","):
            name, w, h, spp = parse(wl)
            key = f"{name}_{w}x{h}"
            if key not in refs and ("pass" in what or "sweep" in what or "vpass" in what):
                refs[key] = os.path.join(d, key + ".npy")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "reference", "--workload", wl,
                                "--ref", refs[key], "--ref-spp", str(a.ref_spp)], check=True, timeout=900)
            if "pass" in what:
                child("--one", "pass", "--workload", wl, "--repeats", str(a.repeats), "--ref", refs[key],
                      "--params", json.dumps(params))
            if "ab" in what and spp == 64:
                child("--one", "ab", "--workload", wl, "--repeats", str(2 * a.repeats))
            if "sweep" in what and spp <= 64:
                child("--one", "sweep", "--workload", wl, "--ref", refs[key])
            if "vpass" in what:
                child("--one", "vpass", "--workload", wl, "--repeats", str(a.repeats), "--ref", refs[key])
            if "vab" in what and spp == 64:
                child("--one", "vab", "--workload", wl, "--repeats", str(2 * a.repeats))
            if "moments" in what and spp == 500:
                child("--one", "moments", "--workload", wl, "--repeats", str(a.repeats))
            if "kernels" in what and spp == 64:
                line = kernels(wl, a.repeats)
                if line is None:
                    sys.exit(1)
                lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
