#!/usr/bin/env python3
"""The ISA hash of every gfx950 kernel of a librtw.so, or the comparison of two
libraries' tables (ray_tracing_weekend_amd/isa.py: machine code + kernel
descriptor per symbol).

    python tools/isa_table.py [LIB] > table.json
    python tools/isa_table.py --against PARENT_LIB [LIB]     # symbols added / gone / changed
"""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_tracing_weekend_amd import isa   # noqa: E402


def table(lib):
    t = {}
    for co in isa.gfx950_code_objects(lib):
        t.update({k: hashlib.sha256(v).hexdigest()[:16] for k, v in isa.kernel_bytes(co).items()})
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", nargs="?", default=isa.LIB)
    ap.add_argument("--against", help="the parent build's librtw.so")
    a = ap.parse_args()
    now = table(a.lib)
    if not a.against:
        json.dump(now, sys.stdout, indent=0, sort_keys=True)
        return
    old = table(a.against)
    print(json.dumps(dict(kernels=len(now), parent_kernels=len(old), added=sorted(set(now) - set(old)),
                          gone=sorted(set(old) - set(now)),
                          changed=sorted(k for k in now if k in old and now[k] != old[k]),
                          table_sha256=hashlib.sha256(json.dumps(now, sort_keys=True).encode()).hexdigest())))


if __name__ == "__main__":
    main()
