"""The traced renders of tests/test_gpu_hit64_replay.py, in a process of their own:

    RTW_LIB_OVERRIDE=<librtw.so of the RTW_TRACE=f32 build> python tests/hit64_trace_child.py OUT.npz

renders every variant of tests/hit64_cases.py once with its scene's pixels
traced (rtw_probes.hpp RTW_TRACE) and writes one .npz: per variant `seg/<name>`
[pixel, sample, segment, 12], `col/<name>` [pixel, sample, 4] and
`kernel/<name>` (world, options) as launched.  TEST INFRASTRUCTURE ONLY.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import hit64_cases as hc            # noqa: E402
import ray_tracing_weekend_amd as rtw   # noqa: E402

NPIX, NS, NSEG, NREC, NCOL = 64, 64, 64, 12, 4


def main(out):
    lib = rtw._lib
    set_list, read, read_col = (getattr(lib, f"rtw_probe_trace_{n}_f32") for n in ("set_list", "read", "read_col"))
    set_list.argtypes = [C.c_void_p, C.c_size_t]
    read.argtypes = read_col.argtypes = [C.c_void_p, C.c_size_t]
    seg = np.empty(NPIX * NS * NSEG * NREC)
    col = np.empty(NPIX * NS * NCOL)
    data = {}
    scenes = {}
    for name, (scene, accel, tuning, want) in hc.VARIANTS.items():
        if scene not in scenes:
            scenes[scene] = hc.SCENES[scene]()
        soa, cam = scenes[scene]
        pix = np.array([j * hc.W + i for i, j in hc.pixels(scene)], np.uint64)
        assert len(pix) <= NPIX
        with rtw.Renderer(device=0, precision=rtw.RTW_F32) as r:
            for k, v in tuning.items():
                r.set_tuning(k, v)
            r.set_accel(accel)
            r.set_scene(soa)
            assert set_list(pix.ctypes.data, len(pix)) == 0
            r.render(cam, hc.SEED)
            kernel = tuple(r.last_kernel())
        assert read(seg.ctypes.data, seg.size) == seg.size and read_col(col.ctypes.data, col.size) == col.size
        print(name, "launched", kernel, flush=True)
        assert kernel[1] & 16, (name, kernel)                 # kOptHit64
        assert want is None or kernel == want, (name, kernel, want)
        data["seg/" + name] = seg.reshape(NPIX, NS, NSEG, NREC)[:len(pix)].copy()
        data["col/" + name] = col.reshape(NPIX, NS, NCOL)[:len(pix)].copy()
        data["kernel/" + name] = np.array(kernel)
    np.savez_compressed(out, **data)


if __name__ == "__main__":
    main(sys.argv[1])
