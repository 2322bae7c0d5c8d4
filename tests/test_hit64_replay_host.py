"""The hit64 replay's driver, proved on the CPU before it judges a kernel: with
every f32 form switched off (f64 inputs, the reference's UnitSphere loop, f64
uniforms) and its hits from restate.World.hit, tests/hit64_replay.py must give
restate.trace_sample's colours and segment counts bit for bit -- the draw
counts, the branch order, the terminations and the f64 scatter forms
(specular_dir64's one-pass Metal / Dielectric, mixture_direction, mat64's host
constants) are then the reference's."""
import numpy as np
import pytest

import hit64_cases as hc
import hit64_replay as hr
from indep import restate as RS


@pytest.mark.parametrize("scene", ["simple", "inside", "walled"])
def test_the_f64_replay_is_the_restatement(scene):
    soa, cam = hc.SCENES[scene]()
    camd = hc.camera_dict(cam)
    world = RS.World(soa)
    rp = hr.Replay(soa, camd, hc.SEED, f32=False)
    kinds, n = set(), 0
    want_kinds = {"simple": {"lambertian to light sphere", "lambertian cosine sphere", "metal fuzz > 0",
                             "dielectric refract front", "dielectric refract back"},
                  "inside": {"lambertian to light sphere", "lambertian cosine sphere", "metal fuzz 0", "metal fuzz > 0",
                             "metal absorbed", "dielectric refract front", "dielectric refract back",
                             "dielectric Schlick reflect front", "dielectric TIR front", "dielectric TIR back",
                             "invisible"},
                  "walled": {"metal absorbed", "metal fuzz > 0"}}[scene]
    for (i, j) in hc.pixels(scene)[::3]:
        for s in range(3):
            want = RS.trace_sample(camd, world, hc.SEED, i, j, s)
            got = hr.host_sample(rp, world, i, j, s, kinds)
            assert got[1] == want[1] and hr.same(got[0], want[0]), (scene, i, j, s, got, want)
            n += want[1]
    assert n > 100
    assert want_kinds <= kinds, want_kinds - kinds          # the proof reached these branches


def test_dither64_keeps_the_f32_value_and_is_idempotent():
    rng = np.random.default_rng(7)
    for v in rng.standard_normal((200, 3)) * 10.0 ** rng.integers(-3, 4, (200, 1)):
        v = hr.v32(v)
        d = hr.dither64(v)
        assert hr.v32(d) == v and hr.is_dithered(d) and d != v
        assert all(abs(a - b) <= abs(b) * 2.0 ** -26 for a, b in zip(d, v))
    assert hr.dither64((0.0, -0.0, 1.0))[:2] == (0.0, -0.0)
