"""The image <-> packed-rank helpers of host/tiles.hpp on the CPU (no GPU
needed): tests/native/rank_pack_check.cpp packs 37 x 23 and 16 x 8 images for
1, 2, 3 and 8 ranks, under the round robin and under a dealt split, checks them
against the assembly's slot map (tile_slots) and the round trip itself, and
prints every case; here the printed tiles and packed values are compared with
ray_tracing_weekend_amd/sharding.py's restatement (deal, rank_tiles, pack)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracing_weekend_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _cost(t):
    return (t * 7919) % 13 + (40 if t % 3 == 0 else 1)       # rank_pack_check.cpp cost_of


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_rank_pack_round_trip_and_restatement(tmp_path):
    import torch

    from ray_tracing_weekend_amd import sharding as S
    exe = str(tmp_path / "rank_pack_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "rank_pack_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    lines = r.stdout.rstrip().split("\n")
    assert lines[-1] == "0 wrong"
    cases, case = [], None
    for line in lines[:-1]:
        key, *vals = line.split()
        if key == "CASE":
            case = {"args": tuple(int(v) for v in vals), "split": None, "tiles": {}, "packed": {}}
            cases.append(case)
        elif key == "SPLIT":
            case["split"] = np.array(vals, np.uint32)
        elif key == "TILES":
            case["tiles"][int(vals[0])] = [int(v) for v in vals[1:]]
        elif key == "PACKED":
            case["packed"][int(vals[0])] = np.array(vals[1:], np.float64)
    assert [c["args"] for c in cases] == [(w, h, n, d) for (w, h) in ((37, 23), (16, 8)) for n in (1, 2, 3, 8)
                                          for d in (0, 1)]
    for c in cases:
        w, h, n, dealt = c["args"]
        split = None
        if dealt:
            split = S.deal([_cost(t) for t in range(S.n_tiles(w, h))], w, h, n)
            assert np.array_equal(c["split"], split), c["args"]
        image = torch.arange(1, w * h * 3 + 1, dtype=torch.float64).reshape(h, w, 3)
        gathered = []
        for k in range(n):
            assert c["tiles"][k] == S.rank_tiles(w, h, k, n, split), (c["args"], k)
            want = S.pack(image, k, n, split).numpy().reshape(-1)
            assert np.array_equal(c["packed"][k], want), (c["args"], k)
            outside = np.ones(want.size, bool)                # the slots of pixels inside the image hold >= 1
            outside[want > 0] = False
            assert (c["packed"][k][outside] == 0).all()
            gathered.append(torch.from_numpy(c["packed"][k].copy()))
        back = S.assemble(torch.zeros(h, w, 3, dtype=torch.float64), gathered, split=split)
        assert torch.equal(back, image), c["args"]
