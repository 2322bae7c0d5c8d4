"""The wavefront path rounds on the CPU (no GPU needed): the planner of
rtw_render_wavefront and the array rules of rtw_path_advance
(tests/native/wavefront_plan_check.cpp, a stand-alone host program, also run
under the address and undefined-behaviour sanitizers); the five entry points
are declared, bound and exported with the ABI unchanged and refuse a NULL
context before any HIP call; the built gfx950 code objects hold exactly the six
new kernels, named apart from every other kernel family; and the numpy
restatement of the advance rules (tests/wavefront_cases.py), which the GPU test
compares the kernel with, is Renderer.render_wavefront's own lines."""
import atexit
import ctypes as C
import functools
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import ray_tracing_weekend_amd as rtw
import wavefront_cases as WC
from ray_tracing_weekend_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
ENTRIES = ("rtw_path_begin_device", "rtw_path_advance", "rtw_path_advance_device", "rtw_render_wavefront",
           "rtw_render_wavefront_device")
# the substrings existing host tests pick kernel families out of the code objects by
TAKEN = ("render_kernel", "hit_rays_kernel", "light_pdf_rays_kernel", "occlusion_kernel", "light_sample_kernel",
         "camera_rays_kernel", "shade_rays_kernel", "primary_features_kernel", "denoise_")


@functools.lru_cache(maxsize=None)
def plan_check_exe(sanitize=False):
    """tests/native/wavefront_plan_check.cpp over the HIP-free planner, compiled once per test run."""
    out = tempfile.mkdtemp(prefix="wavefront_plan_check_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "wavefront_plan_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", *flags, "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "wavefront_plan_check.cpp"),
                    os.path.join(CSRC, "host", "wavefront_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


@needs_hipcc
def test_planner_batches_and_bytes():
    """W * H = 1; 40 x 24 with 4 samples and batch 3 (3 + 1); batch > n_samples;
    W * H > 2^22 (B = 1); n_samples 0; the bytes of every buffer; the array rules."""
    r = subprocess.run([plan_check_exe()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("0 wrong")


@needs_hipcc
def test_planner_runs_clean_under_the_sanitizers():
    """The same stand-alone host program, built with -fsanitize=address,undefined."""
    r = subprocess.run([plan_check_exe(True)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("0 wrong")
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_entry_points_are_declared_bound_and_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtw.h")).read()
    bound = {p[0]: p for p in _capi.PROTOTYPES}
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in bound, name
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(bound[name][2]), name     # as many parameters as the binding has
    assert re.search(r"#define RTW_ABI_VERSION 10\b", header) and _capi.ABI_VERSION == 10
    assert C.sizeof(_capi.rtw_query_stats) == 56      # the stats keep their layout
    for text in ("camera.rs:470-472", "is_light_pdf = 6", "is_light_pdf = 7", "clamp(2^22 / (W * H), 1, n_samples)",
                 "out of place", "6 one path advance", "7 the wavefront driver"):
        assert text in header, text


def test_refusals_without_a_device():
    """A NULL context is RTW_E_INVALID from every entry point, before any HIP
    call (there is no GPU here)."""
    lib = rtw._lib
    inv = _capi.RTW_E_INVALID
    _, b = rtw.scenes.simple_soa(0x5EED0001)
    cam = b.with_image_width(8).with_image_height(4).build()
    n = 2
    v3, v6, r4 = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros((n, 4), np.uint64)
    slot, ev, sums = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros((4, 8, 3))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    bg = (C.c_double * 3)(0, 0, 0)
    m = C.c_uint64(99)
    assert lib.rtw_path_begin_device(None, n, 0, vp(v3), 48, vp(v3), 48, vp(slot), 8, None) == inv
    host = [vp(a) for a in (v3, v3, slot, ev, v3, v3, v6, r4, v6, r4, v3, v3, slot, v3)]
    assert lib.rtw_path_advance(None, n, *host, n, bg, 0, C.byref(m)) == inv and m.value == 99
    dev = []
    for a in (v3, v3, slot, ev, v3, v3, v6, r4, v6, r4, v3, v3, slot, v3):
        dev += [vp(a), a.nbytes]
    assert lib.rtw_path_advance_device(None, n, *dev, n, bg, 0, vp(r4), None) == inv
    assert lib.rtw_render_wavefront(None, C.byref(cam.raw), 7, 0, 1, 0, sums.ctypes.data_as(C.POINTER(C.c_double))) == inv
    assert lib.rtw_render_wavefront_device(None, C.byref(cam.raw), 7, 0, 1, 0, vp(sums), sums.nbytes, None) == inv
    assert not sums.any()


def test_python_and_cpp_mirrors_have_the_surface():
    for name in ("path_begin", "path_advance", "render_wavefront_batched", "render_wavefront"):
        assert callable(getattr(rtw.Renderer, name))
    assert callable(rtw.Camera.render_wavefront_batched)
    sig = inspect.signature(rtw.Renderer.render_wavefront_batched)
    assert list(sig.parameters)[1:] == ["cam", "seed", "first_sample", "n_samples", "batch", "sums", "on_bounce", "as_torch"]
    assert sig.parameters["batch"].default == 0 and sig.parameters["batch"].kind is inspect.Parameter.KEYWORD_ONLY
    hpp = open(os.path.join(CSRC, "host", "rtw_host.hpp")).read()
    cpp = open(os.path.join(CSRC, "host", "ray_queries.cpp")).read()
    assert re.search(r"\bpath_advance\(const PathState& state", hpp) and re.search(r"\brender_wavefront\(const Camera& cam", hpp)
    for entry in ("rtw_path_advance", "rtw_render_wavefront"):
        assert re.search(r"\b" + entry + r"\(ctx,", cpp), entry


def _symbols():
    r = {"f32": "f", "f64": "d"}
    return {f"_ZN3rtw3dev17path_begin_kernelI{r[p]}EEvNS_9PathBeginIT_EE" for p in r} | \
           {f"_ZN3rtw3dev19path_advance_kernelI{r[p]}EEvNS_11PathAdvanceIT_EE" for p in r} | \
           {f"_ZN3rtw3dev16path_fold_kernelI{r[p]}EEvNS_8PathFoldE" for p in r}


def test_kernel_table_is_the_six_new_kernels():
    """path_begin_kernel, path_advance_kernel and path_fold_kernel in both
    precisions, and nothing else of theirs; no new symbol contains a name the
    other host tests select kernel families by."""
    from ray_tracing_weekend_amd import isa
    built = {k for co in isa.gfx950_code_objects() for k in isa.kernel_bytes(co)
             if "path_begin" in k or "path_advance" in k or "path_fold" in k or "PathAdvance" in k or "PathBegin" in k
             or "PathFold" in k}
    assert len(built) == 6
    assert built == _symbols(), (sorted(built - _symbols()), sorted(_symbols() - built))
    assert not any(t in k for k in built for t in TAKEN)
    # all six live in one code object: the unit of both precisions
    homes = [co for co in isa.gfx950_code_objects() if built & set(isa.kernel_bytes(co))]
    assert len(homes) == 1 and set(isa.kernel_bytes(homes[0])) >= built


def _render_wavefront_round(mult, res, paths, colour, event, weight, emitted, nxt, rng, bg, last):
    """Renderer.render_wavefront's bookkeeping of one round, its lines verbatim
    (numpy branch: where = nonzero, contig = ascontiguousarray)."""
    where = lambda m: np.nonzero(m)[0]                 # noqa: E731
    contig = np.ascontiguousarray
    miss, gone = where(event == _capi.RTW_EVENT_MISS), where(event == _capi.RTW_EVENT_ABSORBED)
    colour[paths[miss]] = mult[miss] * bg + res[miss]                  # camera.rs:473-475
    colour[paths[gone]] = mult[gone] * emitted[gone] + res[gone]       # camera.rs:484-486
    scat = where(event == _capi.RTW_EVENT_SCATTER)
    res[scat] = res[scat] + mult[scat] * emitted[scat]                 # camera.rs:519
    keep = where(event >= _capi.RTW_EVENT_REFLECT)
    mult = mult[keep] * weight[keep]                                   # camera.rs:496, 518
    res, paths = res[keep], paths[keep]
    rays, rng = contig(nxt[keep]), contig(rng[keep])
    if last and int(paths.shape[0]):
        colour[paths] = 0.0 + res                                          # camera.rs:470-472
    return rays, rng, mult, res, paths


LINES = ("colour[paths[miss]] = mult[miss] * bg + res[miss]", "colour[paths[gone]] = mult[gone] * emitted[gone] + res[gone]",
         "res[scat] = res[scat] + mult[scat] * emitted[scat]", "keep = where(event >= _capi.RTW_EVENT_REFLECT)",
         "mult = mult[keep] * weight[keep]", "res, paths = res[keep], paths[keep]",
         "rays, rng = contig(nxt[keep]), contig(rng[keep])", "colour[paths] = 0.0 + res")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("last", [False, True])
def test_restatement_is_render_wavefronts_lines(dtype, last):
    """wavefront_cases.advance against the lines of Renderer.render_wavefront (they
    are in its source, and in the helper above, character for character) on
    hand-made records: the four events with NaN, inf and -0 among the values,
    shuffled slots.  The loop only sees the events a bounce writes; an event
    value outside them is a miss into black by rtw.h's rule, checked by hand."""
    src = inspect.getsource(rtw.Renderer.render_wavefront)
    mine = inspect.getsource(_render_wavefront_round)
    for line in LINES:
        assert line in src and line in mine, line
    rec = WC.records(40, dtype, "mixed", seed=3)
    real = rec["event"] >= 0
    real &= rec["event"] <= 3
    rec = {k: v[real] for k, v in rec.items()}
    assert {0, 1, 2, 3} <= set(rec["event"].tolist())
    assert any(np.isnan(rec[k]).any() for k in ("mult", "emitted", "res")) and np.isinf(rec["mult"]).any()
    assert any((np.signbit(rec[k]) & (rec[k] == 0)).any() for k in ("mult", "res", "emitted", "weight"))
    bg = np.asarray([0.7, 0.8, 1.0], dtype)
    colour = np.full((40, 3), WC.SENTINEL, dtype)
    got, got_colour = WC.advance(rec, colour, bg, last)
    want_colour = colour.copy()
    with np.errstate(all="ignore"):
        rays, rng, mult, res, paths = _render_wavefront_round(
            rec["mult"].copy(), rec["res"].copy(), rec["slot"].astype(np.int64), want_colour, rec["event"],
            rec["weight"], rec["emitted"], rec["nxt"], rec["rng"], bg, last)
    assert WC.same(got_colour, want_colour)
    if last:
        assert len(got["slot"]) == 0 and (got_colour[rec["slot"]] != WC.SENTINEL).all()
    else:
        assert len(paths) > 5
        for name, want in (("rays", rays), ("rng", rng), ("mult", mult), ("res", res),
                           ("slot", paths.astype(np.uint32))):
            assert WC.same(got[name], want), name
    untouched = np.setdiff1d(np.arange(40), rec["slot"][~np.isin(rec["event"], (2, 3))] if not last else rec["slot"])
    assert (got_colour[untouched] == WC.SENTINEL).all()


def test_restatement_by_hand():
    """A few paths worked out by hand, f64: each rule, the other-event rule, the
    sign of zero through 0 + res' and mult * 0, and which slots are written."""
    z = np.zeros
    rec = {"mult": np.array([[0.5, 2.0, -0.0], [0.5, 0.5, 0.5], [2.0, 2.0, 2.0], [1.0, 1.0, 1.0], [np.inf, 1.0, -1.0]]),
           "res": np.array([[0.25, -0.0, -0.0], [1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [-0.0, 0.0, 1.0], [1.0, -0.0, -0.0]]),
           "emitted": np.array([[9.0, 9.0, 9.0], [4.0, 0.0, -2.0], [9.0, 9.0, 9.0], [0.5, 0.0, 0.0], [9.0, 9.0, 9.0]]),
           "weight": np.array([[9.0, 9.0, 9.0], [9.0, 9.0, 9.0], [0.5, 0.25, 0.0], [0.5, 0.5, 0.5], [9.0, 9.0, 9.0]]),
           "event": np.array([WC.MISS, WC.ABSORBED, WC.REFLECT, WC.SCATTER, 9], np.int32),
           "slot": np.array([4, 0, 3, 1, 2], np.uint32), "nxt": np.arange(30.0).reshape(5, 6),
           "rng": np.arange(20, dtype=np.uint64).reshape(5, 4)}
    bg = np.array([0.5, 0.25, 1.0])
    out, colour = WC.advance(rec, np.full((6, 3), WC.SENTINEL), bg)
    want = np.full((6, 3), WC.SENTINEL)
    want[4] = (0.5, 0.5, -0.0)          # MISS: 0.5 * 0.5 + 0.25; 2 * 0.25 + -0; -0 * 1 + -0 = -0
    want[0] = (3.0, 1.0, 0.0)           # ABSORBED: 0.5 * 4 + 1; 0.5 * 0 + 1; 0.5 * -2 + 1
    want[2] = (np.nan, 0.0, -0.0)       # no event: inf * 0 + 1 = NaN; 1 * 0 + -0 = +0; -1 * 0 + -0 = -0
    assert WC.same(colour, want)
    assert out["slot"].tolist() == [3, 1]
    assert WC.same(out["mult"], np.array([[1.0, 0.5, 0.0], [0.5, 0.5, 0.5]]))
    assert WC.same(out["res"], np.array([[0.5, 0.5, 0.5], [0.5, 0.0, 1.0]]))      # SCATTER: -0 + 1 * 0.5; 0 + 0; 1 + 0
    assert WC.same(out["rays"], rec["nxt"][[2, 3]]) and WC.same(out["rng"], rec["rng"][[2, 3]])
    out, colour = WC.advance(rec, np.full((6, 3), WC.SENTINEL), bg, last=True)
    want[3] = (0.5, 0.5, 0.5)
    want[1] = (0.5, 0.0, 1.0)           # 0 + res'
    assert WC.same(colour, want) and len(out["slot"]) == 0
    rec["res"][2] = (-0.0, -0.0, -0.0)  # REFLECT keeps res; 0 + -0 = +0
    _, colour = WC.advance(rec, z((6, 3)), bg, last=True)
    assert WC.same(colour[3], np.array([0.0, 0.0, 0.0]))
    # the block rule of the kernel's compaction, on a made-up order
    in_slot = np.arange(600, dtype=np.uint32)
    keep = in_slot % 3 != 0
    blocks = [in_slot[a:a + 256][keep[a:a + 256]] for a in (256, 512, 0)]
    assert WC.blocks_keep_their_order(in_slot, keep, np.concatenate(blocks))
    swapped = np.concatenate(blocks)
    swapped[[0, 1]] = swapped[[1, 0]]
    assert not WC.blocks_keep_their_order(in_slot, keep, swapped)
