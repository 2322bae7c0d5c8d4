"""The radiance query on the CPU (no GPU needed): the entry points are declared,
bound and exported with the ABI unchanged, refuse a NULL context before any HIP
call, exist on the Python surface; the argument checks and the launch plan
(tests/native/radiance_plan_check.cpp: the size and alignment table, the
refusals in their order, the limits, the loop bound, the LDS of every plan); the
kernel table is exactly the radiance_kernel instantiations of the built gfx950
code objects, none of which uses scratch; and the restatement of the law in
tests/radiance_cases.py is restate.trace_sample on camera rays."""
import atexit
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import path_cases as P
import radiance_cases as RC
import ray_tracing_weekend_amd as rtw
from indep import restate as R
from oracle import oracle as O
from ray_tracing_weekend_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HOST_UNITS = ("radiance_plan", "query_plan", "render_plan", "stage_scene", "bvh", "rtw_host")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
ENTRIES = ("rtw_radiance_rays", "rtw_radiance_rays_device")
# the substrings other host tests select kernel families by
TAKEN = ("render_kernel", "hit_rays_kernel", "light_pdf_rays_kernel", "occlusion_kernel", "light_sample_kernel",
         "direct_light_kernel", "ambient_kernel", "camera_rays_kernel", "shade_rays_kernel", "primary_features_kernel",
         "denoise_", "path_begin", "path_advance", "path_fold", "PathBegin", "PathAdvance", "PathFold")


@functools.lru_cache(maxsize=None)
def radiance_plan_check_exe():
    """tests/native/radiance_plan_check.cpp, compiled once per test run."""
    out = tempfile.mkdtemp(prefix="radiance_plan_check_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "radiance_plan_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "radiance_plan_check.cpp"),
                    *[os.path.join(CSRC, "host", u + ".cpp") for u in HOST_UNITS], "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


@needs_hipcc
def test_sizes_refusals_limits_and_every_plan():
    r = subprocess.run([radiance_plan_check_exe()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("\n0 wrong")


def _symbol(prec, world, robust):
    return f"_ZN3rtw3dev15radiance_kernelI{'f' if prec == 'f32' else 'd'}Li{world}ELb{robust}EEEvNS_7RParamsIT_EE"


@needs_hipcc
def test_kernel_table_is_the_library_radiance_kernels():
    """radiance_kernels.h radiance_kernel_exists -- what the launcher's table holds --
    names exactly the kernels of the built library (the worlds and test forms of the
    closest-hit query), and none of them counts as another family's kernel by name."""
    from ray_tracing_weekend_amd import isa
    out = subprocess.run([radiance_plan_check_exe(), "kernels"], capture_output=True, text=True, timeout=60,
                         check=True).stdout
    table = {_symbol(p, int(w), int(r)) for p, w, r in re.findall(r"^radiance (f32|f64) (-?\d+) (\d)$", out, flags=re.M)}
    built = {k for co in isa.gfx950_code_objects() for k in isa.kernel_bytes(co) if "radiance_kernel" in k}
    assert len(table) == 18
    assert table == built, (sorted(table - built), sorted(built - table))
    assert not any(t in k for k in built for t in TAKEN)
    # one code object per precision holds them, and nothing else
    homes = [set(isa.kernel_bytes(co)) for co in isa.gfx950_code_objects()]
    assert sorted(len(h) for h in homes if h & built) == [6, 12] and all(h <= built for h in homes if h & built)


def test_no_radiance_kernel_uses_scratch():
    """The kernel descriptor's private segment size (bytes 4..7 of the .kd) is 0 for every
    instantiation: the lane's state stays in registers."""
    from ray_tracing_weekend_amd import isa
    seen = 0
    for co in isa.gfx950_code_objects():
        for name, typ, shndx, value, size, secs in isa._symbols(co):
            if "radiance_kernel" in name and name.endswith(".kd"):
                _n, _t, addr, off, _s, _l = secs[shndx]
                kd = co[off + value - addr:off + value - addr + size]
                assert len(kd) == 64 and int.from_bytes(kd[4:8], "little") == 0, name
                seen += 1
    assert seen == 18


def test_entry_points_are_declared_bound_and_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtw.h")).read()
    bound = {p[0]: p for p in _capi.PROTOTYPES}
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in bound, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert len(bound["rtw_radiance_rays"][2]) == 14 and len(bound["rtw_radiance_rays_device"][2]) == 20
    assert re.search(r"#define RTW_ABI_VERSION 10\b", header) and _capi.ABI_VERSION == 10
    assert C.sizeof(_capi.rtw_query_stats) == 56      # the stats keep their layout
    # the header states the law, step by step, and the stats value
    flat = re.sub(r"\s*\n\s*\*\s*", " ", header)      # (the comment's line breaks are no part of a phrase)
    for text in ("camera.rs:460-522", "Rng(seed, first_stream + k, s)", "n_samples must be 1", "written back after the path",
                 "colour = mult * background + res", "colour = mult * emitted + res", "res += mult * emitted; mult *= weight",
                 "colour = 0 + res", "every colour is 0 + 0", "every product rounded before its add",
                 "radiance[k][c] += (double)colour_c", "NaN is not scrubbed", "k * S + (s - first_sample)",
                 "RTW_E_NO_LIGHTS where rtw_shade_rays gives it", "first_sample + n_samples over 2^32",
                 "n * S over 2^62", "is_light_pdf = 10", "10 radiance"):
        assert text in flat, text
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert re.search(r"\bfn " + name + r"\(", integration), name


def test_refusals_without_a_device():
    """A NULL context is RTW_E_INVALID from both entry points, before any HIP
    call (there is no GPU here)."""
    lib = rtw._lib
    inv = _capi.RTW_E_INVALID
    rays, rad = np.zeros((2, 6)), np.zeros((2, 3))
    col, seg, rng = np.zeros((2, 3)), np.zeros(2, np.uint32), np.ones((2, 4), np.uint64)
    bg = (C.c_double * 3)(0.5, 0.7, 1.0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.rtw_radiance_rays(None, vp(rays), 2, 7, 0, 0, 1, 8, bg, vp(rng), 0, vp(rad), vp(col), vp(seg)) == inv
    assert lib.rtw_radiance_rays(None, None, 0, 7, 0, 0, 1, 8, None, None, 0, None, None, None) == inv
    assert lib.rtw_radiance_rays_device(None, vp(rays), rays.nbytes, 2, 7, 0, 0, 1, 8, bg, vp(rng), rng.nbytes, 0,
                                        vp(rad), rad.nbytes, vp(col), col.nbytes, vp(seg), seg.nbytes, None) == inv
    assert lib.rtw_radiance_rays_device(None, None, 0, 0, 7, 0, 0, 1, 8, None, None, 0, 0, None, 0, None, 0, None, 0,
                                        None) == inv


def test_python_surface():
    for name in ("radiance", "render_radiance"):
        assert callable(getattr(rtw.Renderer, name))
    assert callable(rtw.HittableList.radiance)
    import inspect
    sig = inspect.signature(rtw.Renderer.radiance)
    assert list(sig.parameters)[1:] == ["rays", "seed", "n_samples", "max_depth", "background", "first_stream",
                                        "first_sample", "rng", "radiance", "records"]
    assert sig.parameters["max_depth"].default == 50 and sig.parameters["n_samples"].default == 1


@pytest.mark.parametrize("name", ["cornell_box", "simple", "lights64_emissive"])
def test_the_restated_law_is_trace_sample_on_camera_rays(name):
    """radiance_cases.law_path on get_ray's ray and state is restate.trace_sample: the colour bit
    for bit and the segment count, at depth 8 and with the survivors of a depth of 2."""
    soa, _ = RC.scene(name)
    shader = P.Shader(soa)
    pixels = list(range(3, RC.W * RC.H, 11))
    ended = set()
    for depth in (RC.DEPTH, 2):
        cam = O.camera_dict(RC.oracle_camera(name, depth))
        for s in (0, 2):
            for pix in pixels:
                o, d, g = P.get_ray(cam, RC.SEED, pix, s)
                colour, segs, _ = RC.law_path(shader, (*o, *d), g.s, depth, cam["background"])
                want, wsegs = R.trace_sample(cam, shader.world, RC.SEED, pix % RC.W, pix // RC.W, s)
                assert segs == wsegs and RC.same(np.array(colour), np.array(want)), (depth, s, pix, colour, want)
                ended.add("last round" if segs == depth else "earlier")
    assert ended == {"last round", "earlier"}


def test_expected_windows_states_and_zero_depth_on_the_cpu():
    """The case file's own algebra: the seeded mode is the rng mode on start_states, windows
    compose, depth 0 is 0 + 0 with nothing traced, a zero state that misses stays zero."""
    soa, _ = RC.scene("cornell_box")
    cam = O.camera_dict(RC.oracle_camera("cornell_box"))
    rays = P.camera_rays(cam, RC.SEED, list(range(0, RC.W * RC.H, 41)), 0)[0]
    n = len(rays)
    bg = cam["background"]
    whole = RC.Expected(soa, rays, RC.SEED, 3, RC.DEPTH, bg, first_stream=5)
    assert RC.same(whole.radiance, RC.fold(np.zeros((n, 3)), whole.colours, 3))
    acc = np.zeros((n, 3))
    for s in range(3):
        st = RC.start_states(RC.SEED, 5, n, s)
        one = RC.Expected(soa, rays, 0, 1, RC.DEPTH, bg, rng=st, radiance=acc)
        assert RC.same(one.colours, whole.colours[s::3]) and np.array_equal(one.segments, whole.segments[s::3])
        assert not np.array_equal(one.rng[whole.segments[s::3] > 1], st[whole.segments[s::3] > 1])
        acc = one.radiance
    assert RC.same(acc, whole.radiance)
    none = RC.Expected(soa, rays, RC.SEED, 2, 0, bg)
    assert not none.colours.any() and not none.segments.any() and not np.signbit(none.colours).any()
    away = RC.cornell_phase_rays(2)[:1]
    z = RC.Expected(soa, away, 0, 1, RC.DEPTH, (0.25, 0.5, 1.0), rng=np.zeros((1, 4), np.uint64))
    assert not z.rng.any() and z.segments[0] == 1 and tuple(z.colours[0]) == (0.25, 0.5, 1.0)
