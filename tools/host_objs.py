"""The host objects of librtw.so, as csrc/Makefile lists them: what a tool that
links a variant library (its own render units + the in-tree host objects)
puts on the link line, so that no tool names the units itself."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")


def _make(target):
    return subprocess.run(["make", "-s", "-C", CSRC, target], check=True, capture_output=True, text=True).stdout.split()


def host_objs():
    """Paths of the in-tree build's host objects (C-ABI + host units)."""
    return _make("host-objs")


def layout_units():
    """Paths of the host sources that include rtw_kernels.h: a probe build
    that changes its layouts must recompile them."""
    return _make("layout-units")
