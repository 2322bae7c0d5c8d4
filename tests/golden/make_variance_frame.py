"""Regenerates tests/golden/variance_frame_simple_64x40.npz: the frame the
quality test of the variance-guided denoiser (tests/test_denoise_variance_host.py)
runs on, from the repository's own CPU oracle alone.

scenes::simple (seed 0x5EED0001, grid 11) from its own camera narrowed to vfov
18, 64 x 40, depth 50.  Per (pixel, sample) of seed 7, O.trace_path gives the
colour and the primary ray's hit, O.world_hit the normal: folded in sample
order (sequential f64 sums) into the colour sums, the feature sums of
rtw_render_features and the luminance moments {sum Y, sum Y*Y} at 16, 64 and
256 samples.  ref: the means of a 4096-sample O.render of seed 8.

    python tests/golden/make_variance_frame.py        (about half a minute on 8 CPUs)
"""
import math
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import oracle as O  # noqa: E402

SCENE_SEED, GRID = 0x5EED0001, 11
W, H, DEPTH, VFOV = 64, 40, 50, 18.0
SEED, SPPS = 7, (16, 64, 256)
REF_SEED, REF_SPP = 8, 4096
LAMBERTIAN, METAL, DIELECTRIC, DIFFUSE_LIGHT = 0, 1, 2, 4
OUT = os.path.join(HERE, "variance_frame_simple_64x40.npz")


def camera(spp):
    kw = dict(O.simple_camera_kw(GRID), vfov=VFOV, image_width=W, image_height=H, samples_per_pixel=spp,
              max_depth=DEPTH)
    return O.camera_build(**kw)


def luma(c):
    return ((0.2126 * c[..., 0]) + (0.7152 * c[..., 1])) + (0.0722 * c[..., 2])


def row(j):
    """Per sample of row j: colours [W, S, 3] and features [W, S, 8]."""
    sc, cam = O.scene_simple(SCENE_SEED, GRID), camera(SPPS[-1])
    bg = tuple(cam.background)
    n_pl = len(sc.plane_mat)
    colour = np.zeros((W, SPPS[-1], 3))
    feat = np.zeros((W, SPPS[-1], 8))
    for i in range(W):
        for s in range(SPPS[-1]):
            rgb, path = O.trace_path(cam, sc, SEED, i, j, s, cap=1)
            colour[i, s] = rgb
            o, d = tuple(map(float, path[0][:3])), tuple(map(float, path[0][3:6]))
            oid, t = int(path[0][6]), float(path[0][7])
            if oid < 0:
                feat[i, s, :3] = bg
                continue
            _, _, _, nrm, _ = O.world_hit(sc, o, d)
            # (object ids: the planes, then the spheres -- simple has no quads or cuboids)
            m = int(sc.plane_mat[oid]) if oid < n_pl else int(sc.sphere_mat[oid - n_pl])
            kind = int(sc.mat_type[m])
            if kind in (LAMBERTIAN, METAL, DIFFUSE_LIGHT):
                albedo = tuple(map(float, sc.mat_params[m][:3]))
            elif kind == DIELECTRIC:
                albedo = (1.0, 1.0, 1.0)
            else:
                albedo = (0.0, 0.0, 0.0)
            dist = t * math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            feat[i, s] = (*albedo, *nrm, dist, 1.0)
    return colour, feat


def main():
    with ProcessPoolExecutor(max_workers=min(os.cpu_count() or 1, 16)) as ex:
        rows = list(ex.map(row, range(H)))
    colour = np.stack([r[0] for r in rows])       # [H, W, S, 3]
    feat = np.stack([r[1] for r in rows])
    with np.errstate(all="ignore"):
        y = luma(colour)
        c_sums, f_sums = np.cumsum(colour, axis=2), np.cumsum(feat, axis=2)   # (left to right: the sequential fold)
        s1, s2 = np.cumsum(y, axis=2), np.cumsum(y * y, axis=2)
    out = {}
    for n in SPPS:
        out[f"sums_{n}"] = c_sums[:, :, n - 1]
        out[f"features_{n}"] = f_sums[:, :, n - 1]
        out[f"moments_{n}"] = np.stack([s1[:, :, n - 1], s2[:, :, n - 1]], -1)
    ref, _ = O.render(camera(REF_SPP), O.scene_simple(SCENE_SEED, GRID), REF_SEED, chunk=1,
                      accel=O.ACCEL_BVH_CACHED)
    out["ref"] = ref / REF_SPP
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
