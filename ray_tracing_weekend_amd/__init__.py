"""ray_tracing_weekend_amd -- MI355X (gfx950) drop-in for the reference's
per-pixel / per-sample ray_colour loop (N9199/ray_tracing_weekend).

Python mirror of the reference's interface for this path, over the C-ABI in
include/rtw.h (librtw.so: hand-written HIP kernels + C++ host mirror):

    world, lights, builder = scenes.simple(seed)          # scenes/src/lib.rs:155-233
    cam = builder.with_image_width(400).with_image_height(225) \
                 .with_samples_per_pixel(100).with_max_depth(50).build()
    sums = cam.render(world, lights)                      # shared/src/camera.rs:295-297
    write_ppm("image.ppm", sums, cam.samples_per_pixel)   # bin/src/main.rs:89-104

`render` returns per-pixel SUMS (not means) as a float64 array [H, W, 3] with
row j = 0 at the BOTTOM, like render_internal's Vec<Vec<Colour>>.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import _capi
from ._capi import (RTW_ACCEL_AUTO, RTW_ACCEL_BRUTE, RTW_ACCEL_BVH, RTW_DIELECTRIC, RTW_F32,
                    RTW_F64, RTW_INVISIBLE, RTW_LAMBERTIAN, RTW_METAL, RTW_DIFFUSE_LIGHT, RTW_TEX_SOLID,
                    RTW_TEX_CHECKER, RTW_TEX_NOISE, RTW_LIGHT_SPHERE, RTW_LIGHT_QUAD, RTW_LIGHT_DEFAULT,
                    RTW_LIGHTS_BVH_LEAF)

__all__ = [
    "Material", "Lambertian", "Metal", "Dialectric", "DiffuseLight", "INVISIBLE", "Sphere", "Plane",
    "Quad", "Cuboid", "Transformation", "translation", "rotation", "SolidColour", "CheckerTexture",
    "NoiseTexture", "Perlin", "HittableList", "BoundedVolumeHierarchy", "SceneSoA", "flatten",
    "CameraBuilder", "Camera", "Renderer", "scenes", "encode_rgb8", "write_ppm", "RenderError",
    "RTW_F32", "RTW_F64", "feature_means", "DenoiseParams", "DenoiseVarianceParams",
]

_lib = _capi.load()   # raises if librtw.so is missing: there is no CPU fallback


class RenderError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{msg} (rtw error {code})")
        self.code = code


# ---------------------------------------------------------------- textures
class Perlin:                                # perlin.rs:13-58
    """Perlin::new with the build's seeded RNG (the reference draws the
    tables from thread_rng): rand_vec (256 x 3) and perm (3 x 256)."""

    def __init__(self, seed: int = 0x5EED0001):
        self.rand_vec = np.zeros((256, 3), np.float64)
        self.perm = np.zeros((3, 256), np.uint32)
        rc = _lib.rtw_perlin_generate(C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF),
                                      self.rand_vec.ctypes.data_as(_capi._f64p),
                                      self.perm.ctypes.data_as(_capi._u32p))
        if rc != 0:
            raise RenderError(rc, "rtw_perlin_generate failed")


@dataclass(frozen=True, eq=False)
class SolidColour:                           # texture.rs:15-22
    colour: tuple


@dataclass(frozen=True, eq=False)
class CheckerTexture:                        # texture.rs:24-55
    even: object
    odd: object
    inv_scale: float

    @staticmethod
    def new(even, odd, scale: float) -> "CheckerTexture":
        return CheckerTexture(even, odd, 1.0 / float(scale))          # scale.recip()

    @staticmethod
    def new_with_colours(even, odd, scale: float) -> "CheckerTexture":
        return CheckerTexture.new(SolidColour(tuple(map(float, even))), SolidColour(tuple(map(float, odd))), scale)


@dataclass(frozen=True, eq=False)
class NoiseTexture:                          # texture.rs:57-102
    scale: float
    noise: Perlin

    @staticmethod
    def new(scale: float, seed: int = 0x5EED0001) -> "NoiseTexture":
        return NoiseTexture(float(scale), Perlin(seed))


_TEXTURES = (SolidColour, CheckerTexture, NoiseTexture)


# ---------------------------------------------------------------- materials
@dataclass(frozen=True)
class Material:
    type: int
    albedo: tuple = (0.0, 0.0, 0.0)
    fuzz: float = 0.0
    ior: float = 0.0
    texture: object = None                   # Lambertian / DiffuseLight texture; None = SolidColour(albedo)


def Lambertian(albedo):                      # material.rs:347-355 (new / new_with_colour)
    if isinstance(albedo, _TEXTURES):
        return Material(RTW_LAMBERTIAN, texture=albedo)
    return Material(RTW_LAMBERTIAN, tuple(map(float, albedo)))


def Metal(albedo, fuzz):                     # material.rs:378-406
    return Material(RTW_METAL, tuple(map(float, albedo)), float(fuzz))


def Dialectric(index_of_refraction):         # material.rs:423-455
    return Material(RTW_DIELECTRIC, (1.0, 1.0, 1.0), 0.0, float(index_of_refraction))


INVISIBLE = Material(RTW_INVISIBLE)          # material.rs:321-325


def DiffuseLight(colour):                    # material.rs:490-514 (new / new_with_colour)
    if isinstance(colour, _TEXTURES):
        return Material(RTW_DIFFUSE_LIGHT, texture=colour)
    return Material(RTW_DIFFUSE_LIGHT, tuple(map(float, colour)))


@dataclass(frozen=True)
class Sphere:                                # entities/sphere.rs:24-47
    center: tuple
    radius: float
    mat: Material = INVISIBLE


@dataclass(frozen=True)
class Plane:                                 # entities/plane.rs:20-38 (normal normalized)
    point: tuple
    normal: tuple
    mat: Material = INVISIBLE

    def __post_init__(self):
        n = [float(v) for v in self.normal]
        ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        object.__setattr__(self, "normal", (n[0] / ln, n[1] / ln, n[2] / ln))


@dataclass(frozen=True)
class Quad:                                  # entities/quadrilateral.rs:21-56 (Quad::new(Q, u, v, mat))
    q: tuple
    u: tuple
    v: tuple
    mat: Material = INVISIBLE


@dataclass(frozen=True)
class Transformation:
    """geometry::transformations::Transformation (non-euclid build): point ->
    R p + T.  `then` composes like the reference (transformations.rs:97-108)."""
    R: tuple = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    T: tuple = (0.0, 0.0, 0.0)

    def then(self, b: "Transformation") -> "Transformation":
        def dot(u, v):
            return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
        cols = [[self.R[0][j], self.R[1][j], self.R[2][j]] for j in range(3)]
        R = tuple(tuple(dot(b.R[i], cols[j]) for j in range(3)) for i in range(3))
        bRT = [dot(b.R[i], self.T) for i in range(3)]
        return Transformation(R, tuple(b.T[i] + bRT[i] for i in range(3)))


def translation(v) -> Transformation:        # Translation3 = Vec3 -> Transformation (vec3.rs:11)
    return Transformation(T=tuple(map(float, v)))


def rotation(angle_deg: float, axis: int) -> Transformation:   # transformations.rs:37-58 (axis 0/1/2 = X/Y/Z)
    a = float(angle_deg) * (math.pi / 180.0)                  # f64::to_radians
    c, s = math.cos(a), math.sin(a)                           # libm, as f64::cos / f64::sin
    R = [((1.0, 0.0, 0.0), (0.0, c, -s), (0.0, s, c)),
         ((c, 0.0, s), (0.0, 1.0, 0.0), (-s, 0.0, c)),
         ((c, -s, 0.0), (s, c, 0.0), (0.0, 0.0, 1.0))][axis]
    return Transformation(R=R)


@dataclass(frozen=True)
class Cuboid:                                # entities/cuboid.rs:26-47, Cuboid::new(p, q, mat)
    p: tuple
    q: tuple
    mat: Material = INVISIBLE
    xform: Transformation = Transformation()

    def transform(self, t: Transformation) -> "Cuboid":
        """Transformable::transform (transformations.rs:187-211): the
        transformations compose in call order."""
        return Cuboid(self.p, self.q, self.mat, self.xform.then(t))


class HittableList:                          # hittable_collections/hittable_list.rs:247-294
    def __init__(self, objects=()):
        self.objects = []
        for o in objects:
            self.add(o)

    def add(self, obj):
        if not isinstance(obj, (Sphere, Plane, Quad, Cuboid)):
            raise TypeError("only Sphere, Plane, Quad and (transformed) Cuboid are in this build's scope")
        self.objects.append(obj)

    def __len__(self):
        return len(self.objects)

    def hit(self, rays, t_min: float | None = None, *, lights=None, precision: int = RTW_F64,
            device: int = 0, accel: int = RTW_ACCEL_AUTO):
        """Hittable::hit of this list as the world (hittable.rs:172-182), for
        n rays [n, 6] {origin, direction} over t_min..=INFINITY: (hits [n, 9],
        ids [n, 4]) as Renderer.hit_rays gives them.  Flattens and stages the
        scene as Camera.render does; keep a Renderer for repeated queries."""
        with Renderer(device=device, precision=precision) as r:
            r.set_accel(accel)
            r.set_scene(flatten(self, lights if lights is not None else HittableList()))
            return r.hit_rays(rays, t_min)

    def pdf_value(self, rays, *, world=None, precision: int = RTW_F64, device: int = 0,
                  accel: int = RTW_ACCEL_AUTO):
        """HittableList::pdf_value of this list as the light list
        (hittable_list.rs:408-412; a BoundedVolumeHierarchy: its leaf form) for
        n (origin, direction) pairs [n, 6]: the pdfs [n]."""
        with Renderer(device=device, precision=precision) as r:
            r.set_accel(accel)
            r.set_scene(flatten(world if world is not None else HittableList(), self))
            return r.light_pdf(rays)

    def occluded(self, rays, t_max=None, t_min: float | None = None, *, lights=None, precision: int = RTW_F64,
                 device: int = 0, accel: int = RTW_ACCEL_AUTO):
        """Hittable::hit of this list as the world over t_min..=t_max[i],
        .is_some(): uint8 [n] as Renderer.occluded gives them."""
        with Renderer(device=device, precision=precision) as r:
            r.set_accel(accel)
            r.set_scene(flatten(self, lights if lights is not None else HittableList()))
            return r.occluded(rays, t_max, t_min)

    def random(self, origins, seed: int, first_stream: int = 0, sample: int = 0, *, pdf: bool = True, world=None,
               precision: int = RTW_F64, device: int = 0, accel: int = RTW_ACCEL_AUTO):
        """HittableList::random of this list as the light list
        (hittable_list.rs:414-419) for n origins [n, 3]: (directions, pdf or
        None, light) as Renderer.light_sample gives them."""
        with Renderer(device=device, precision=precision) as r:
            r.set_accel(accel)
            r.set_scene(flatten(world if world is not None else HittableList(), self))
            return r.light_sample(origins, seed, first_stream, sample, pdf)

    def direct_light(self, points, seed: int, n_samples: int = 1, first_stream: int = 0, first_sample: int = 0,
                     t_min: float | None = None, *, lights, records: bool = False, precision: int = RTW_F64,
                     device: int = 0, accel: int = RTW_ACCEL_AUTO):
        """Direct lighting of n points [n, 6] {p, normal} in this list as the
        world, from the light list `lights`: the sums [n, 3] (and the sample
        records) as Renderer.direct_light gives them.  Stages the scene for
        this one call; keep a Renderer for repeated queries."""
        with Renderer(device=device, precision=precision) as r:
            r.set_accel(accel)
            r.set_scene(flatten(self, lights))
            return r.direct_light(points, seed, n_samples, first_stream, first_sample, t_min, records=records)

    def ambient_occlusion(self, points, seed: int, n_samples: int = 1, t_max: float | None = None,
                          t_min: float | None = None, first_stream: int = 0, first_sample: int = 0, *,
                          lights=None, records: bool = False, precision: int = RTW_F64, device: int = 0,
                          accel: int = RTW_ACCEL_AUTO):
        """The open counts of n points [n, 6] {p, normal} in this list as the
        world (and the sample records) as Renderer.ambient_occlusion gives
        them.  Stages the scene for this one call; keep a Renderer for repeated
        queries."""
        with Renderer(device=device, precision=precision) as r:
            r.set_accel(accel)
            r.set_scene(flatten(self, lights if lights is not None else HittableList()))
            return r.ambient_occlusion(points, seed, n_samples, t_max, t_min, first_stream, first_sample,
                                       records=records)

    def radiance(self, rays, seed: int, n_samples: int = 1, max_depth: int = 50, background=(0.0, 0.0, 0.0),
                 first_stream: int = 0, first_sample: int = 0, *, lights, records: bool = False,
                 precision: int = RTW_F64, device: int = 0, accel: int = RTW_ACCEL_AUTO):
        """Incoming radiance along n rays [n, 6] {origin, direction} in this list
        as the world, with the light list `lights`: the sums [n, 3] (and the
        sample records) as Renderer.radiance gives them.  Stages the scene for
        this one call; keep a Renderer for repeated queries."""
        with Renderer(device=device, precision=precision) as r:
            r.set_accel(accel)
            r.set_scene(flatten(self, lights))
            return r.radiance(rays, seed, n_samples, max_depth, background, first_stream, first_sample,
                              records=records)


class BoundedVolumeHierarchy(HittableList):  # hittable_collections/bvh.rs:106-143 (::from(list))
    """The reference's BVH over a list: as the world it gives the list's
    closest hit (the device builds its own tree); as a light list its
    pdf_value is (sum / n * n) / n for a leaf of <= 5 entries (bvh.rs:67-76,
    191-194).  Deeper BVH light lists are outside this build (their
    aux_random indexing, bvh.rs:78-92, is inconsistent)."""

    def __init__(self, lst=()):
        super().__init__(lst.objects if isinstance(lst, HittableList) else lst)


@dataclass
class SceneSoA:
    """Flattened world + lights in the C-ABI's struct-of-arrays layout."""
    spheres: np.ndarray = field(default_factory=lambda: np.zeros((0, 4)))
    sphere_mat: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint32))
    planes: np.ndarray = field(default_factory=lambda: np.zeros((0, 6)))
    plane_mat: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint32))
    mat_type: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint32))
    mat_params: np.ndarray = field(default_factory=lambda: np.zeros((0, 5)))
    lights: np.ndarray = field(default_factory=lambda: np.zeros((0, 4)))
    quads: np.ndarray = field(default_factory=lambda: np.zeros((0, 9)))
    quad_mat: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint32))
    light_quads: np.ndarray = field(default_factory=lambda: np.zeros((0, 9)))
    light_kinds: np.ndarray = None          # list order: 0 sphere / 1 quad; None = spheres first
    boxes: np.ndarray = field(default_factory=lambda: np.zeros((0, 18)))
    box_mat: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint32))
    mat_tex: np.ndarray = None              # texture id per material; None = SolidColour albedos
    tex_type: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint32))
    tex_params: np.ndarray = field(default_factory=lambda: np.zeros((0, 4)))
    tex_refs: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.uint32))
    perlin_vec: np.ndarray = field(default_factory=lambda: np.zeros((0, 256, 3)))
    perlin_perm: np.ndarray = field(default_factory=lambda: np.zeros((0, 3, 256), np.uint32))
    n_light_other: int = 0
    light_flags: int = 0

    def as_c(self):
        """(rtw_scene, keepalive) -- the struct points into these arrays."""
        keep = []

        def f(a, cols):
            a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, cols))
            keep.append(a)
            return a.ctypes.data_as(_capi._f64p)

        def u(a):
            a = np.ascontiguousarray(np.asarray(a, np.uint32).reshape(-1))
            keep.append(a)
            return a.ctypes.data_as(_capi._u32p)

        s = _capi.rtw_scene(len(self.sphere_mat), f(self.spheres, 4), u(self.sphere_mat),
                            len(self.plane_mat), f(self.planes, 6), u(self.plane_mat),
                            len(self.mat_type), u(self.mat_type), f(self.mat_params, 5),
                            len(np.asarray(self.lights).reshape(-1, 4)), f(self.lights, 4),
                            len(self.quad_mat), f(self.quads, 9), u(self.quad_mat),
                            len(np.asarray(self.light_quads).reshape(-1, 9)), f(self.light_quads, 9),
                            None if self.light_kinds is None else u(self.light_kinds),
                            len(self.box_mat), f(self.boxes, 18), u(self.box_mat),
                            None if self.mat_tex is None else u(self.mat_tex),
                            len(np.asarray(self.tex_type).reshape(-1)), u(self.tex_type), f(self.tex_params, 4),
                            u(self.tex_refs), len(np.asarray(self.perlin_vec).reshape(-1, 768)),
                            f(self.perlin_vec, 768), u(self.perlin_perm),
                            int(self.n_light_other), int(self.light_flags))
        return s, keep

    @staticmethod
    def from_c(s: "_capi.rtw_scene") -> "SceneSoA":
        def f(ptr, n, cols):
            return np.ctypeslib.as_array(ptr, shape=(n * cols,)).reshape(n, cols).copy() if n else np.zeros((0, cols))

        def u(ptr, n):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, np.uint32)

        return SceneSoA(f(s.spheres, s.n_spheres, 4), u(s.sphere_mat, s.n_spheres),
                        f(s.planes, s.n_planes, 6), u(s.plane_mat, s.n_planes),
                        u(s.mat_type, s.n_materials), f(s.mat_params, s.n_materials, 5),
                        f(s.lights, s.n_lights, 4), f(s.quads, s.n_quads, 9), u(s.quad_mat, s.n_quads),
                        f(s.light_quads, s.n_light_quads, 9),
                        u(s.light_kinds, s.n_lights + s.n_light_quads + s.n_light_other) if s.light_kinds else None,
                        f(s.boxes, s.n_boxes, 18), u(s.box_mat, s.n_boxes),
                        u(s.mat_tex, s.n_materials) if s.mat_tex else None,
                        u(s.tex_type, s.n_textures), f(s.tex_params, s.n_textures, 4),
                        u(s.tex_refs, 2 * s.n_textures).reshape(-1, 2),
                        f(s.perlin_vec, s.n_perlin, 768).reshape(-1, 256, 3),
                        u(s.perlin_perm, 768 * s.n_perlin).reshape(-1, 3, 256),
                        int(s.n_light_other), int(s.light_flags))


def flatten(world, lights) -> SceneSoA:
    """world: HittableList (or BoundedVolumeHierarchy) or SceneSoA; lights:
    a HittableList / BoundedVolumeHierarchy.  The light list's order is kept:
    it is the light pdf's sum order and the uniform pick's index.  Spheres
    and Quads sample themselves; Planes and Cuboids in a light list have the
    Hittable defaults (pdf 0, random (1, 0, 0); hittable.rs:175-181)."""
    if isinstance(world, SceneSoA):
        return world
    mats, mtypes, sph, smat, pl, pmat, qd, qmat = [], [], [], [], [], [], [], []
    textured = any(o.mat.texture is not None and o.mat.type in (RTW_LAMBERTIAN, RTW_DIFFUSE_LIGHT)
                   for o in world.objects)
    mtex, ttype, tpar, trefs, pvec, pperm = [], [], [], [], [], []
    tex_ids, perlin_ids = {}, {}

    def push_tex(t):
        if id(t) in tex_ids:
            return tex_ids[id(t)][0]
        k = len(ttype)
        tex_ids[id(t)] = (k, t)                       # keep t alive while its id() is a key
        if isinstance(t, SolidColour):
            ttype.append(RTW_TEX_SOLID)
            tpar.append(list(map(float, t.colour)) + [0.0])
            trefs.append([0, 0])
        elif isinstance(t, CheckerTexture):
            ttype.append(RTW_TEX_CHECKER)
            tpar.append([0.0, 0.0, 0.0, t.inv_scale])
            trefs.append([0, 0])
            trefs[k] = [push_tex(t.even), push_tex(t.odd)]
        else:
            ttype.append(RTW_TEX_NOISE)
            tpar.append([0.0, 0.0, 0.0, t.scale])
            if id(t.noise) not in perlin_ids:
                perlin_ids[id(t.noise)] = (len(pvec), t.noise)
                pvec.append(t.noise.rand_vec)
                pperm.append(t.noise.perm)
            trefs.append([perlin_ids[id(t.noise)][0], 0])
        return k

    def push(m: Material):
        mtypes.append(m.type)
        mats.append(list(m.albedo) + [m.fuzz, m.ior])
        if textured:
            if m.texture is not None and m.type in (RTW_LAMBERTIAN, RTW_DIFFUSE_LIGHT):
                mtex.append(push_tex(m.texture))
            else:
                mtex.append(push_tex(SolidColour(m.albedo)))
        return len(mtypes) - 1

    # materials numbered planes, spheres, quads, cuboids (as the C++ flatten)
    for o in world.objects:
        if isinstance(o, Plane):
            pl.append(list(o.point) + list(o.normal))
            pmat.append(push(o.mat))
    for o in world.objects:
        if isinstance(o, Sphere):
            sph.append(list(o.center) + [o.radius])
            smat.append(push(o.mat))
    for o in world.objects:
        if isinstance(o, Quad):
            qd.append(list(o.q) + list(o.u) + list(o.v))
            qmat.append(push(o.mat))
    bx, bmat = [], []
    for o in world.objects:
        if isinstance(o, Cuboid):
            bx.append(list(o.p) + list(o.q) + [v for row in o.xform.R for v in row] + list(o.xform.T))
            bmat.append(push(o.mat))
    li, lq, kinds = [], [], []
    for o in lights.objects:
        if isinstance(o, Sphere):
            li.append(list(o.center) + [o.radius])
            kinds.append(RTW_LIGHT_SPHERE)
        elif isinstance(o, Quad):
            lq.append(list(o.q) + list(o.u) + list(o.v))
            kinds.append(RTW_LIGHT_QUAD)
        else:
            kinds.append(RTW_LIGHT_DEFAULT)
    n_other = kinds.count(RTW_LIGHT_DEFAULT)
    flags = 0
    if isinstance(lights, BoundedVolumeHierarchy):
        if len(lights) > 5:
            raise RenderError(_capi.RTW_E_UNSUPPORTED, "a BVH light list of more than 5 entries (bvh.rs:78-92)")
        flags |= RTW_LIGHTS_BVH_LEAF
    return SceneSoA(np.array(sph, np.float64).reshape(-1, 4), np.array(smat, np.uint32),
                    np.array(pl, np.float64).reshape(-1, 6), np.array(pmat, np.uint32),
                    np.array(mtypes, np.uint32), np.array(mats, np.float64).reshape(-1, 5),
                    np.array(li, np.float64).reshape(-1, 4), np.array(qd, np.float64).reshape(-1, 9),
                    np.array(qmat, np.uint32), np.array(lq, np.float64).reshape(-1, 9),
                    np.array(kinds, np.uint32) if (lq or n_other) else None,
                    np.array(bx, np.float64).reshape(-1, 18), np.array(bmat, np.uint32),
                    np.array(mtex, np.uint32) if textured else None, np.array(ttype, np.uint32),
                    np.array(tpar, np.float64).reshape(-1, 4), np.array(trefs, np.uint32).reshape(-1, 2),
                    np.array(pvec, np.float64).reshape(-1, 256, 3), np.array(pperm, np.uint32).reshape(-1, 3, 256),
                    n_other, flags)


# ---------------------------------------------------------------- camera
class CameraBuilder:                          # camera.rs:28-112
    def __init__(self, raw: "_capi.rtw_camera_builder | None" = None):
        if raw is None:
            raw = _capi.rtw_camera_builder()
            _lib.rtw_camera_builder_default(C.byref(raw))
        self.raw = raw

    def _set3(self, name, v):
        getattr(self.raw, name)[:] = [float(x) for x in v]
        return self

    def with_aspect_ratio(self, v):
        self.raw.has_aspect_ratio, self.raw.aspect_ratio = 1, float(v)
        return self

    def with_image_width(self, v):
        self.raw.has_image_width, self.raw.image_width = 1, int(v)
        return self

    def with_image_height(self, v):
        self.raw.has_image_height, self.raw.image_height = 1, int(v)
        return self

    def with_samples_per_pixel(self, v):
        self.raw.samples_per_pixel = int(v)
        return self

    def with_max_depth(self, v):
        self.raw.max_depth = int(v)
        return self

    def with_background(self, c):
        return self._set3("background", c)

    def with_vfov(self, v):
        self.raw.vfov = float(v)
        return self

    def with_lookfrom(self, p):
        return self._set3("lookfrom", p)

    def with_lookat(self, p):
        return self._set3("lookat", p)

    def with_vup(self, v):
        return self._set3("vup", v)

    def with_defocus_angle(self, v):
        self.raw.defocus_angle = float(v)
        return self

    def with_focus_dist(self, v):
        self.raw.focus_dist = float(v)
        return self

    def build(self) -> "Camera":              # camera.rs:114-218
        cam = _capi.rtw_camera()
        rc = _lib.rtw_camera_build(C.byref(self.raw), C.byref(cam))
        if rc != 0:
            raise RenderError(rc, "CameraBuilder::build failed")
        return Camera(cam)

    def copy(self) -> "CameraBuilder":
        raw = _capi.rtw_camera_builder()
        C.pointer(raw)[0] = self.raw
        return CameraBuilder(raw)


class Camera:
    def __init__(self, raw: "_capi.rtw_camera"):
        self.raw = raw

    def __getattr__(self, name):
        raw = self.__dict__["raw"]
        v = getattr(raw, name)
        return tuple(v) if isinstance(v, C.Array) else v

    def render(self, world, lights, *, seed: int = 0x5EED0001, precision: int = RTW_F64,
               device: int = 0, devices=None, accel: int = RTW_ACCEL_AUTO) -> np.ndarray:
        """Camera::render (camera.rs:295-297) on the GPU: float64 sums [H, W, 3].
        The default is the parity mode (RTW_F64: the reference's f64 arithmetic,
        bit-identical to the oracle); precision=RTW_F32 opts into the faster
        speed mode, which agrees with the reference statistically.
        `devices` (a list of GPU indices) renders on all of them, one rank each
        (rtw_create_devices) -- the same image bit for bit."""
        with Renderer(device=device, precision=precision, devices=devices) as r:
            r.set_accel(accel)
            r.set_scene(flatten(world, lights))
            return r.render(self, seed)

    render_debug = render                     # camera.rs:299-312 (no sequential mode on a GPU)

    def render_progressive(self, world, lights, window: int, *, seed: int = 0x5EED0001,
                           precision: int = RTW_F64, device: int = 0, devices=None):
        """The render `window` samples at a time: a generator of (samples_done,
        sums) after each window, sums the float64 [H, W, 3] running sums (the
        same array each time: copy it to keep a stage).  The last yield is
        render()'s image bit for bit (at one sample per item, the default).  A
        stage saved with np.savez continues later with
        Renderer.render_window(cam, seed, samples_done, n, sums).  `devices` as
        render()'s: every listed GPU renders its tiles of each window."""
        if window < 1:
            raise RenderError(_capi.RTW_E_INVALID, "render_progressive: window must be >= 1")
        spp = self.raw.samples_per_pixel
        with Renderer(device=device, precision=precision, devices=devices) as r:
            r.set_scene(flatten(world, lights))
            sums = None
            for first in range(0, spp, window):
                n = min(window, spp - first)
                sums = r.render_window(self, seed, first, n, sums)
                yield first + n, sums

    def render_adaptive(self, world, lights, min_samples: int, max_samples: int, window: int, tolerance: float,
                        *, seed: int = 0x5EED0001, precision: int = RTW_F64, device: int = 0, devices=None,
                        accel: int = RTW_ACCEL_AUTO):
        """Adaptive sampling of the scene (Renderer.render_adaptive): (sums,
        counts), each tile stopped between min_samples and max_samples once its
        pixels are within `tolerance`.  `devices` as render()'s: the same sums
        and counts bit for bit from all the listed GPUs."""
        with Renderer(device=device, precision=precision, devices=devices) as r:
            r.set_accel(accel)
            r.set_scene(flatten(world, lights))
            return r.render_adaptive(self, seed, min_samples, max_samples, window, tolerance)

    def render_features(self, world, lights, first: int = 0, n: int | None = None, *, seed: int = 0x5EED0001,
                        counts=None, want_ids: bool = True, precision: int = RTW_F64, device: int = 0,
                        accel: int = RTW_ACCEL_AUTO):
        """The denoising guides of this camera's render of the scene
        (Renderer.render_features): (features [H, W, 8], ids [H, W, 2] | None),
        with the scene staged for this one call."""
        with Renderer(device=device, precision=precision) as r:
            r.set_accel(accel)
            r.set_scene(flatten(world, lights))
            return r.render_features(self, seed, first, n, counts=counts, want_ids=want_ids)

    def render_wavefront(self, world, lights, first_sample: int = 0, n_samples: int | None = None, on_bounce=None,
                         *, seed: int = 0x5EED0001, precision: int = RTW_F64, device: int = 0,
                         accel: int = RTW_ACCEL_AUTO) -> np.ndarray:
        """The render as a loop over the path queries (Renderer.render_wavefront),
        with the scene staged for this one call: float64 sums [H, W, 3], in
        RTW_F64 render()'s bit for bit; on_bounce is the per-round hook."""
        with Renderer(device=device, precision=precision) as r:
            r.set_accel(accel)
            r.set_scene(flatten(world, lights))
            return r.render_wavefront(self, seed, first_sample, n_samples, on_bounce)

    def render_wavefront_batched(self, world, lights, first_sample: int = 0, n_samples: int | None = None, *,
                                 batch: int = 0, on_bounce=None, seed: int = 0x5EED0001, precision: int = RTW_F64,
                                 device: int = 0, accel: int = RTW_ACCEL_AUTO) -> np.ndarray:
        """render_wavefront with its rounds on the device, `batch` samples at a
        time (Renderer.render_wavefront_batched), with the scene staged for this
        one call: float64 sums [H, W, 3], the same bits as render_wavefront."""
        with Renderer(device=device, precision=precision) as r:
            r.set_accel(accel)
            r.set_scene(flatten(world, lights))
            return r.render_wavefront_batched(self, seed, first_sample, n_samples, batch=batch, on_bounce=on_bounce)

    def render_denoised(self, world, lights, *, seed: int = 0x5EED0001, precision: int = RTW_F64, device: int = 0,
                        accel: int = RTW_ACCEL_AUTO, variance: bool = False, **params) -> np.ndarray:
        """The render, its feature pass and the denoiser on one context: the
        filtered per-sample means [H, W, 3] float64 of Renderer.render's sums
        and Renderer.render_features' guides of the same samples (display them
        with spp = 1).  **params as Renderer.denoise's.  variance=True: the
        variance-guided filter instead -- Renderer.render_window_moments of
        all the samples, the feature pass and Renderer.denoise_variance
        (**params as its)."""
        with Renderer(device=device, precision=precision) as r:
            r.set_accel(accel)
            r.set_scene(flatten(world, lights))
            if variance:
                spp = int(self.raw.samples_per_pixel)
                sums, moments = r.render_window_moments(self, seed, 0, spp)
                features, _ = r.render_features(self, seed, want_ids=False)
                return r.denoise_variance(sums, features, moments, spp, **params)
            sums = r.render(self, seed)
            features, _ = r.render_features(self, seed, want_ids=False)
            return r.denoise(sums, features, int(self.raw.samples_per_pixel), **params)


class Renderer:
    """An rtw_ctx: a device (or, with `devices`, one rank per listed GPU:
    rtw_create_devices), a precision, a resident scene and work buffers."""

    def __init__(self, device: int = 0, precision: int = RTW_F32, *, devices=None, virtual_ranks=None):
        self.ctx = None
        if virtual_ranks is not None:
            # test mode (rtw_create_virtual): `virtual_ranks` ranks on `device`,
            # the gather by device copies -- the n-rank path on one GPU
            out = C.c_void_p()
            rc = _lib.rtw_create_virtual(device, int(virtual_ranks), precision, C.byref(out))
            if rc != 0:
                raise RenderError(rc, f"rtw_create_virtual({device}, {virtual_ranks}) failed (code {rc})")
            self.ctx = out.value
        elif devices is not None:
            devs = [int(d) for d in devices]
            arr = (C.c_int * max(len(devs), 1))(*devs)
            out = C.c_void_p()
            rc = _lib.rtw_create_devices(arr, len(devs), precision, C.byref(out))
            if rc != 0:
                raise RenderError(rc, f"rtw_create_devices({devs}) failed (code {rc}): an empty, repeated "
                                  "or not visible device, or a HIP / RCCL failure")
            self.ctx = out.value
            device = devs[0]
        else:
            self.ctx = _lib.rtw_create(device, precision)
            if not self.ctx:
                raise RenderError(_capi.RTW_E_DEVICE, f"rtw_create(device={device}) failed: no gfx950 "
                                  "device visible (this library has no CPU path)")
        self.device = device
        self.precision = precision
        self.stats = _capi.rtw_stats()
        self._adaptive_size = None    # (W, H) of the last adaptive render: adaptive_moments
        self._listed = devices is not None or virtual_ranks is not None

    @property
    def n_devices(self) -> int:
        return int(_lib.rtw_device_count(self.ctx))

    @property
    def _whole_image(self) -> bool:
        """The context is a multi-device one (a list of one GPU included): its
        window and adaptive renders go through the *_image entry points."""
        return self.n_devices > 1 or getattr(self, "_listed", False)

    def rank_view(self, k: int) -> "_RankView":
        """Rank k's per-device context (stats / timings / last kernel)."""
        sub = _lib.rtw_device_ctx(self.ctx, k)
        if not sub:
            raise RenderError(_capi.RTW_E_INVALID, f"no rank {k}")
        return _RankView(self, k, sub, int(_lib.rtw_device_of(sub)), self.precision)

    def close(self):
        if self.ctx:
            _lib.rtw_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise RenderError(rc, f"{what}: {_lib.rtw_last_error(self.ctx).decode()}")

    def set_chunk(self, chunk: int):
        self._check(_lib.rtw_set_chunk(self.ctx, chunk), "rtw_set_chunk")

    def set_tuning(self, key: str, value: int):
        self._check(_lib.rtw_set_tuning(self.ctx, key.encode(), int(value)), "rtw_set_tuning")

    def set_accel(self, accel: int):
        self._check(_lib.rtw_set_accel(self.ctx, accel), "rtw_set_accel")

    def set_scene(self, scene: SceneSoA):
        s, keep = scene.as_c()
        self._check(_lib.rtw_set_scene(self.ctx, C.byref(s)), "rtw_set_scene")
        del keep

    def render(self, cam: Camera, seed: int) -> np.ndarray:
        H, W = cam.raw.image_height, cam.raw.image_width
        out = np.zeros((H, W, 3), np.float64)
        self._check(_lib.rtw_render(self.ctx, C.byref(cam.raw), None, C.c_uint64(seed),
                                    out.ctypes.data_as(_capi._f64p), C.byref(self.stats)),
                    "rtw_render")
        return out

    def render_device(self, cam: Camera, seed: int, out_ptr: int, out_bytes: int, *,
                      rank: int = 0, nranks: int = 1, stream: int | None = None):
        """Asynchronous render of this rank's 8x8 tiles (T = rank mod nranks),
        packed, into device memory (rtw_render_device).  `stream` defaults to
        torch's current stream, so that the render is ordered after the torch
        work that prepared `out_ptr` and before the work that reads it."""
        if stream is None:
            stream = _torch_stream(self.device)
        self._check(_lib.rtw_render_device(self.ctx, C.byref(cam.raw), C.c_uint64(seed), rank,
                                           nranks, C.c_void_p(out_ptr) if out_ptr else None, out_bytes,
                                           C.c_void_p(stream) if stream else None),
                    "rtw_render_device")

    def render_window(self, cam: Camera, seed: int, first: int, n: int, sums=None) -> np.ndarray:
        """Samples [first, first + n) of every pixel, continuing the running
        sums `sums` (float64 [H, W, 3] of samples [0, first); not needed when
        first == 0) in place (rtw_render_window).  Windows folded one after
        another are the one-shot render of as many samples, bit for bit.
        Returns the sums; cam.samples_per_pixel is not read.  On a multi-device
        Renderer every rank renders its tiles of the window
        (rtw_render_window_image): the same sums bit for bit."""
        H, W = cam.raw.image_height, cam.raw.image_width
        if sums is None:
            if first:
                raise RenderError(_capi.RTW_E_INVALID, "render_window: first > 0 continues `sums`")
            sums = np.zeros((H, W, 3), np.float64)
        if sums.dtype != np.float64 or sums.shape != (H, W, 3) or not sums.flags.c_contiguous:
            raise RenderError(_capi.RTW_E_INVALID, "sums must be a contiguous float64 array [H, W, 3]")
        fn, name = ((_lib.rtw_render_window_image, "rtw_render_window_image") if self._whole_image
                    else (_lib.rtw_render_window, "rtw_render_window"))
        self._check(fn(self.ctx, C.byref(cam.raw), C.c_uint64(seed), first, n, sums.ctypes.data_as(_capi._f64p),
                       C.byref(self.stats)), name)
        return sums

    def render_window_moments(self, cam: Camera, seed: int, first: int, n: int, sums=None, moments=None):
        """render_window that also keeps each pixel's luminance moments
        (rtw_render_window_moments): (sums float64 [H, W, 3], moments float64
        [H, W, 2] = {sum Y, sum Y*Y}) of samples [0, first + n), continuing
        `sums` and `moments` of samples [0, first) in place (neither is needed
        when first == 0).  One sample per item: the sums are render_window's at
        chunk 1 bit for bit, and windows compose bit for bit.  One-device
        Renderers only."""
        H, W = cam.raw.image_height, cam.raw.image_width
        if sums is None or moments is None:
            if first:
                raise RenderError(_capi.RTW_E_INVALID, "render_window_moments: first > 0 continues `sums` and `moments`")
            sums = np.zeros((H, W, 3), np.float64) if sums is None else sums
            moments = np.zeros((H, W, 2), np.float64) if moments is None else moments
        for a, k, what in ((sums, 3, "sums"), (moments, 2, "moments")):
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (H, W, k)
                    and a.flags.c_contiguous and a.flags.writeable):
                raise RenderError(_capi.RTW_E_INVALID, f"{what} must be a contiguous float64 array [H, W, {k}]")
        self._check(_lib.rtw_render_window_moments(self.ctx, C.byref(cam.raw), C.c_uint64(seed), first, n,
                                                   sums.ctypes.data_as(_capi._f64p),
                                                   moments.ctypes.data_as(_capi._f64p), C.byref(self.stats)),
                    "rtw_render_window_moments")
        return sums, moments

    def render_window_moments_device(self, cam: Camera, seed: int, first: int, n: int, sums_ptr: int,
                                     sums_bytes: int, moments_ptr: int, moments_bytes: int, *,
                                     stream: int | None = None):
        """render_window_moments on device memory (rtw_render_window_moments_device):
        image-order H*W*3 float64 sums and H*W*2 float64 moments, continued in
        place; on torch's current stream by default."""
        if stream is None:
            stream = _torch_stream(self.device)
        self._check(_lib.rtw_render_window_moments_device(
            self.ctx, C.byref(cam.raw), C.c_uint64(seed), first, n, C.c_void_p(sums_ptr) if sums_ptr else None,
            sums_bytes, C.c_void_p(moments_ptr) if moments_ptr else None, moments_bytes,
            C.c_void_p(stream) if stream else None), "rtw_render_window_moments_device")

    def adaptive_moments(self, width: int | None = None, height: int | None = None) -> np.ndarray:
        """The luminance moments float64 [H, W, 2] = {sum Y, sum Y*Y} of the
        last render_adaptive / render_adaptive_device on this one-device
        Renderer, over each pixel's first counts[pixel] samples
        (rtw_adaptive_moments).  The image size is that render's."""
        if width is None or height is None:
            if self._adaptive_size is None:
                raise RenderError(_capi.RTW_E_INVALID, "adaptive_moments: no adaptive render on this Renderer yet")
            width, height = self._adaptive_size
        moments = np.zeros((height, width, 2), np.float64)
        self._check(_lib.rtw_adaptive_moments(self.ctx, moments.ctypes.data_as(_capi._f64p)), "rtw_adaptive_moments")
        return moments

    def adaptive_moments_device(self, moments_ptr: int, moments_bytes: int, *, stream: int | None = None):
        """adaptive_moments into device memory (rtw_adaptive_moments_device):
        H*W*2 float64, on torch's current stream by default."""
        if stream is None:
            stream = _torch_stream(self.device)
        self._check(_lib.rtw_adaptive_moments_device(self.ctx, C.c_void_p(moments_ptr) if moments_ptr else None,
                                                     moments_bytes, C.c_void_p(stream) if stream else None),
                    "rtw_adaptive_moments_device")

    def render_window_device(self, cam: Camera, seed: int, first: int, n: int, accum_ptr: int,
                             accum_bytes: int, *, rank: int = 0, nranks: int = 1, stream: int | None = None):
        """Asynchronous window [first, first + n) of this rank's tiles folded
        onto a device accumulator of tiles_for_rank * 64 * 3 float64, packed
        like render_device's output (rtw_render_window_device); on torch's
        current stream by default."""
        if stream is None:
            stream = _torch_stream(self.device)
        self._check(_lib.rtw_render_window_device(self.ctx, C.byref(cam.raw), C.c_uint64(seed), rank, nranks,
                                                  first, n, C.c_void_p(accum_ptr) if accum_ptr else None,
                                                  accum_bytes, C.c_void_p(stream) if stream else None),
                    "rtw_render_window_device")

    def render_adaptive(self, cam: Camera, seed: int, min_samples: int, max_samples: int, window: int,
                        tolerance: float):
        """Adaptive sampling (rtw_render_adaptive): every 8x8 tile takes
        min_samples samples, then `window` more at a time up to max_samples,
        and stops once the standard error of each of its pixels' displayed
        value sqrt(mean) is at most `tolerance`.  Returns (sums, counts): the
        float64 [H, W, 3] sums and the uint32 [H, W] samples each pixel took --
        sums[j, i] is the window render of its first counts[j, i] samples bit
        for bit.  Stopping on the samples' own variance biases the estimate
        slightly; cam.samples_per_pixel is not read.  Display with
        encode_rgb8(sums, counts) / write_ppm(path, sums, counts).  On a
        multi-device Renderer every rank runs the passes on the tiles it owns
        (rtw_render_adaptive_image): the same sums and counts bit for bit."""
        H, W = cam.raw.image_height, cam.raw.image_width
        sums = np.zeros((H, W, 3), np.float64)
        counts = np.zeros((H, W), np.uint32)
        fn, name = ((_lib.rtw_render_adaptive_image, "rtw_render_adaptive_image") if self._whole_image
                    else (_lib.rtw_render_adaptive, "rtw_render_adaptive"))
        self._check(fn(self.ctx, C.byref(cam.raw), C.c_uint64(seed), min_samples, max_samples, window,
                       float(tolerance), sums.ctypes.data_as(_capi._f64p), counts.ctypes.data_as(_capi._u32p),
                       C.byref(self.stats)), name)
        self._adaptive_size = (W, H)
        return sums, counts

    def render_adaptive_device(self, cam: Camera, seed: int, min_samples: int, max_samples: int, window: int,
                               tolerance: float, sums_ptr: int, sums_bytes: int, counts_ptr: int,
                               counts_bytes: int, *, stream: int | None = None):
        """render_adaptive into device memory (rtw_render_adaptive_device):
        H*W*3 float64 sums and H*W uint32 counts in image order, on torch's
        current stream by default.  The call synchronises with the host once
        per pass (it reads back how many tiles go on).  On a multi-device
        Renderer (rtw_render_adaptive_image_device) the buffers and the stream
        are the first device's."""
        if stream is None:
            stream = _torch_stream(self.device)
        fn, name = ((_lib.rtw_render_adaptive_image_device, "rtw_render_adaptive_image_device")
                    if self._whole_image else (_lib.rtw_render_adaptive_device, "rtw_render_adaptive_device"))
        self._check(fn(self.ctx, C.byref(cam.raw), C.c_uint64(seed), min_samples, max_samples, window,
                       float(tolerance), C.c_void_p(sums_ptr) if sums_ptr else None, sums_bytes,
                       C.c_void_p(counts_ptr) if counts_ptr else None, counts_bytes,
                       C.c_void_p(stream) if stream else None), name)
        self._adaptive_size = (int(cam.raw.image_width), int(cam.raw.image_height))

    def render_image_device(self, cam: Camera, seed: int, image_ptr: int, image_bytes: int, *,
                            stream: int | None = None):
        """Asynchronous render of the whole image [H, W, 3] into device memory
        of the first device (rtw_render_image_device): every device of the
        context renders its share, one RCCL gather, the assembly on `stream`
        (torch's current stream of the first device by default)."""
        if stream is None:
            stream = _torch_stream(self.device)
        self._check(_lib.rtw_render_image_device(self.ctx, C.byref(cam.raw), C.c_uint64(seed),
                                                 C.c_void_p(image_ptr) if image_ptr else None, image_bytes,
                                                 C.c_void_p(stream) if stream else None),
                    "rtw_render_image_device")

    def assemble_tiles(self, ranks_ptr: int, rank_stride_bytes: int, nranks: int, width: int,
                       height: int, image_ptr: int, *, stream: int | None = None):
        """The ranks' gathered packed tiles -> the image [H, W, 3] on the device
        (rtw_assemble_tiles), on torch's current stream by default."""
        if stream is None:
            stream = _torch_stream(self.device)
        self._check(_lib.rtw_assemble_tiles(self.ctx, C.c_void_p(ranks_ptr), rank_stride_bytes, nranks,
                                            width, height, C.c_void_p(image_ptr),
                                            C.c_void_p(stream) if stream else None),
                    "rtw_assemble_tiles")

    def set_split(self, width: int, height: int, nranks: int, tile_rank=None, tile_cost=None):
        """Renders and assemblies of a width x height image over nranks ranks
        follow this tile -> rank split from now on (rtw_set_split, ABI 10);
        None restores the round robin.  tile_cost orders each rank's tasks."""
        n = n_tiles(width, height)

        def arr(a):
            if a is None:
                return None, None
            a = np.ascontiguousarray(np.asarray(a, np.uint32).reshape(-1))
            if a.size != n:
                raise RenderError(_capi.RTW_E_INVALID, f"split arrays need {n} entries, got {a.size}")
            return a, a.ctypes.data_as(_capi._u32p)
        r, rp = arr(tile_rank)
        c, cp = arr(tile_cost)
        self._check(_lib.rtw_set_split(self.ctx, width, height, nranks, rp, cp), "rtw_set_split")

    def get_split(self, width: int, height: int, nranks: int):
        """(kind, tile_rank) of the split renders of this size and rank count
        follow (rtw_get_split): kind 0 = the round robin (tile_rank None),
        1 = set by set_split, 2 = dealt by the context itself (balance)."""
        out = np.zeros(n_tiles(width, height), np.uint32)
        kind = _lib.rtw_get_split(self.ctx, width, height, nranks, out.ctypes.data_as(_capi._u32p))
        if kind < 0:
            self._check(kind, "rtw_get_split")
        return int(kind), (out if kind else None)

    def tile_costs(self, cam: Camera, rank: int = 0, nranks: int = 1, out=None) -> np.ndarray:
        """The tile costs this context counted in its first render of (cam,
        rank, nranks) (rtw_tile_costs): uint32 [n_tiles], the rank's tiles
        filled in (zeros elsewhere, or `out`'s entries kept).  Waits."""
        n = n_tiles(cam.image_width, cam.image_height)
        out = np.zeros(n, np.uint32) if out is None else out
        if out.dtype != np.uint32 or out.size != n or not out.flags.c_contiguous:
            raise RenderError(_capi.RTW_E_INVALID, "out must be a contiguous uint32 array of n_tiles")
        self._check(_lib.rtw_tile_costs(self.ctx, C.byref(cam.raw), rank, nranks, out.ctypes.data_as(_capi._u32p)),
                    "rtw_tile_costs")
        return out

    def culled_tiles(self) -> int:
        """Tiles of the last render that were provably empty and answered by
        the fold without tracing (rtw_culled_tiles; tuning "tile_cull")."""
        return int(_lib.rtw_culled_tiles(self.ctx))

    def get_timings(self, n: int = 64):
        """(render_ms, total_ms) lists for the last n renders (HIP events)."""
        a, b = (C.c_float * n)(), (C.c_float * n)()
        got = _lib.rtw_get_timings(self.ctx, a, b, n)
        if got < 0:
            self._check(got, "rtw_get_timings")
        return list(a[:got]), list(b[:got])

    def last_kernel(self):
        """(kernel, options) of the render kernel the last render launched
        (rtw_last_kernel), or None before any: render_kernel<R, kernel, options>."""
        v = _lib.rtw_last_kernel(self.ctx)
        if v < 0:
            self._check(v, "rtw_last_kernel")
        return None if v == 0 else (v >> 8, v & 0xff)

    def get_stats(self) -> "_capi.rtw_stats":
        self._check(_lib.rtw_get_stats(self.ctx, C.byref(self.stats)), "rtw_get_stats")
        return self.stats

    # ---- batched ray queries (rtw_hit_rays / rtw_light_pdf_rays)
    def _query_rays(self, rays, what):
        """(rays as [n, 6] of the context's precision, is_torch).  numpy input is
        converted; a torch tensor must be on this device, contiguous and of the
        context's precision already (no silent copy of device memory)."""
        np_dtype = np.float32 if self.precision == RTW_F32 else np.float64
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            want = torch.float32 if self.precision == RTW_F32 else torch.float64
            if rays.dtype != want:
                raise RenderError(_capi.RTW_E_INVALID, f"{what}: tensor dtype {rays.dtype}, the context's is {want}")
            if not rays.is_cuda or rays.device.index != self.device:
                raise RenderError(_capi.RTW_E_INVALID, f"{what}: the tensor is not on device {self.device}")
            if rays.dim() != 2 or rays.shape[1] != 6 or not rays.is_contiguous():
                raise RenderError(_capi.RTW_E_INVALID, f"{what}: rays must be a contiguous [n, 6] tensor")
            return rays, True
        a = np.ascontiguousarray(np.asarray(rays, np_dtype))
        if a.ndim != 2 or a.shape[1] != 6:
            raise RenderError(_capi.RTW_E_INVALID, f"{what}: rays must be [n, 6] {{origin, direction}}")
        return a, False

    def hit_rays(self, rays, t_min: float | None = None):
        """world.hit(&r, t_min..=INFINITY) of the staged scene for n rays
        [n, 6] {origin, direction}: (hits [n, 9] {t, p, normal (front-face
        adjusted), u, v}, ids [n, 4] int32 {object id or -1, material id, front
        face, RTW_PRIM_*}); a miss has object -1 and zeros.  t_min defaults to
        f64::EPSILON, the integrator's.  numpy in, numpy out (the host entry);
        a torch tensor on the GPU goes through the device entry on torch's
        current stream, without a host copy, and torch tensors come back."""
        t_min = 2.220446049250313e-16 if t_min is None else float(t_min)
        r, is_torch = self._query_rays(rays, "hit_rays")
        n = int(r.shape[0])
        if is_torch:
            import torch
            hits = torch.zeros((n, 9), dtype=r.dtype, device=r.device)
            ids = torch.zeros((n, 4), dtype=torch.int32, device=r.device)
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_hit_rays_device(self.ctx, C.c_void_p(r.data_ptr()), n, t_min,
                                                 C.c_void_p(hits.data_ptr()), hits.numel() * hits.element_size(),
                                                 C.c_void_p(ids.data_ptr()), ids.numel() * 4,
                                                 C.c_void_p(stream) if stream else None), "rtw_hit_rays_device")
            return hits, ids
        hits = np.zeros((n, 9), r.dtype)
        ids = np.zeros((n, 4), np.int32)
        self._check(_lib.rtw_hit_rays(self.ctx, r.ctypes.data_as(C.c_void_p), n, t_min,
                                      hits.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p)), "rtw_hit_rays")
        return hits, ids

    def light_pdf(self, rays):
        """lights.pdf_value(origin, direction) of the staged light list for n
        pairs [n, 6]: the pdfs [n] (NaN where the reference's is: an origin
        inside a light sphere, an empty list).  numpy / torch as hit_rays."""
        r, is_torch = self._query_rays(rays, "light_pdf")
        n = int(r.shape[0])
        if is_torch:
            import torch
            pdf = torch.zeros((n,), dtype=r.dtype, device=r.device)
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_light_pdf_rays_device(self.ctx, C.c_void_p(r.data_ptr()), n,
                                                       C.c_void_p(pdf.data_ptr()), pdf.numel() * pdf.element_size(),
                                                       C.c_void_p(stream) if stream else None),
                        "rtw_light_pdf_rays_device")
            return pdf
        pdf = np.zeros(n, r.dtype)
        self._check(_lib.rtw_light_pdf_rays(self.ctx, r.ctypes.data_as(C.c_void_p), n,
                                            pdf.ctypes.data_as(C.c_void_p)), "rtw_light_pdf_rays")
        return pdf

    # ---- any-hit occlusion and light sampling (rtw_occluded_rays / rtw_light_sample)
    def occluded(self, rays, t_max=None, t_min: float | None = None):
        """world.hit(&r, t_min..=t_max[i]).is_some() of the staged scene for n
        rays [n, 6]: uint8 [n], 1 where anything lies in the inclusive range.
        t_max: [n] of the context's precision, or None for +inf; an entry that
        is NaN or below t_min answers 0, as does a NaN ray.  t_min defaults to
        f64::EPSILON.  The traversal stops at the first accepted hit.  numpy /
        torch as hit_rays (a torch t_max must be a tensor like the rays)."""
        t_min = 2.220446049250313e-16 if t_min is None else float(t_min)
        r, is_torch = self._query_rays(rays, "occluded")
        n = int(r.shape[0])
        if is_torch:
            import torch
            if t_max is not None:
                if type(t_max).__module__.split(".")[0] != "torch" or t_max.dtype != r.dtype or \
                        t_max.device != r.device or t_max.dim() != 1 or t_max.shape[0] != n or \
                        not t_max.is_contiguous():
                    raise RenderError(_capi.RTW_E_INVALID, "occluded: t_max must be a contiguous [n] tensor of the "
                                                           "rays' dtype and device")
            occ = torch.zeros((n,), dtype=torch.uint8, device=r.device)
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_occluded_rays_device(
                self.ctx, C.c_void_p(r.data_ptr()), n, t_min,
                C.c_void_p(t_max.data_ptr()) if t_max is not None and n else None,
                t_max.numel() * t_max.element_size() if t_max is not None else 0,
                C.c_void_p(occ.data_ptr()), occ.numel(), C.c_void_p(stream) if stream else None),
                "rtw_occluded_rays_device")
            return occ
        tm = None
        if t_max is not None:
            tm = np.ascontiguousarray(np.asarray(t_max, r.dtype))
            if tm.shape != (n,):
                raise RenderError(_capi.RTW_E_INVALID, "occluded: t_max must be [n], one upper end per ray")
        occ = np.zeros(n, np.uint8)
        self._check(_lib.rtw_occluded_rays(self.ctx, r.ctypes.data_as(C.c_void_p), n, t_min,
                                           tm.ctypes.data_as(C.c_void_p) if tm is not None and n else None,
                                           occ.ctypes.data_as(C.c_void_p)), "rtw_occluded_rays")
        return occ

    def light_sample(self, origins, seed: int, first_stream: int = 0, sample: int = 0, pdf: bool = True):
        """lights.random(origin, rng) of the staged light list for n points
        [n, 3]: (directions [n, 3], pdf [n] or None, light [n] int32).  Point k
        draws from the stream a render gives to (seed, pixel first_stream + k,
        sample): one index draw, then the entry's random() -- so calls compose
        over first_stream.  Directions are the reference's, unnormalised (a
        quad's is p - origin; NaN for an origin inside a sphere light); pdf is
        light_pdf of {origin, direction} bit for bit, fused into the same
        kernel; light is the list index drawn.  An empty light list is
        refused.  numpy / torch as hit_rays."""
        np_dtype = np.float32 if self.precision == RTW_F32 else np.float64
        is_torch = type(origins).__module__.split(".")[0] == "torch"
        seed, first_stream, sample = int(seed), int(first_stream), int(sample)
        if is_torch:
            import torch
            want = torch.float32 if self.precision == RTW_F32 else torch.float64
            if origins.dtype != want:
                raise RenderError(_capi.RTW_E_INVALID, f"light_sample: tensor dtype {origins.dtype}, the context's is {want}")
            if not origins.is_cuda or origins.device.index != self.device:
                raise RenderError(_capi.RTW_E_INVALID, f"light_sample: the tensor is not on device {self.device}")
            if origins.dim() != 2 or origins.shape[1] != 3 or not origins.is_contiguous():
                raise RenderError(_capi.RTW_E_INVALID, "light_sample: origins must be a contiguous [n, 3] tensor")
            n = int(origins.shape[0])
            dirs = torch.zeros((n, 3), dtype=want, device=origins.device)
            p = torch.zeros((n,), dtype=want, device=origins.device) if pdf else None
            light = torch.zeros((n,), dtype=torch.int32, device=origins.device)
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_light_sample_device(
                self.ctx, C.c_void_p(origins.data_ptr()), n, seed, first_stream, sample,
                C.c_void_p(dirs.data_ptr()), dirs.numel() * dirs.element_size(),
                C.c_void_p(p.data_ptr()) if pdf and n else None, p.numel() * p.element_size() if pdf else 0,
                C.c_void_p(light.data_ptr()), light.numel() * 4, C.c_void_p(stream) if stream else None),
                "rtw_light_sample_device")
            return dirs, p, light
        o = np.ascontiguousarray(np.asarray(origins, np_dtype))
        if o.ndim != 2 or o.shape[1] != 3:
            raise RenderError(_capi.RTW_E_INVALID, "light_sample: origins must be [n, 3]")
        n = int(o.shape[0])
        dirs = np.zeros((n, 3), np_dtype)
        p = np.zeros(n, np_dtype) if pdf else None
        light = np.zeros(n, np.int32)
        self._check(_lib.rtw_light_sample(self.ctx, o.ctypes.data_as(C.c_void_p), n, seed, first_stream, sample,
                                          dirs.ctypes.data_as(C.c_void_p),
                                          p.ctypes.data_as(C.c_void_p) if pdf and n else None,
                                          light.ctypes.data_as(C.c_void_p)), "rtw_light_sample")
        return dirs, p, light

    # ---- direct lighting as one query (rtw_direct_light)
    def direct_light(self, points, seed: int, n_samples: int = 1, first_stream: int = 0, first_sample: int = 0,
                     t_min: float | None = None, direct=None, records: bool = False):
        """Direct lighting of n shading points [n, 6] {p, normal} (fields 1..6
        of a hit_rays record) with n_samples light samples each: the f64 sums
        [n, 3] of emitted * scattering_pdf / pdf over the samples s =
        first_sample .. first_sample + n_samples - 1.  Per sample: the
        direction, list index and pdf of light_sample (stream: seed,
        first_stream + k, s), the closest hit of hit_rays along it, the
        emission shade_rays gives that hit, and Lambertian's scattering pdf
        max(dot(normal, unit(d)) / pi, 0); a term is added only for a hit with
        pdf > 0 and scattering pdf > 0.  The light list's lobe alone, not the
        reference's mixture; the caller multiplies by the albedo and divides by
        the samples.  A point with normal (0, 0, 0) -- a miss row of hit_rays
        -- is skipped: its sums stay as they are.  direct: sums to continue
        ([n, 3] f64; updated in place when it is a contiguous f64 array or
        tensor), or None to start from zero.  records=True also returns
        (samples [n * n_samples, 12] {d, pdf, t, spdf, Le, term}, sample_ids
        [n * n_samples, 4] int32 {light index, object id or -1, material id,
        added}).  t_min defaults to f64::EPSILON.  numpy in, numpy out (the
        host entry); torch GPU tensors go through the device entry on torch's
        current stream."""
        t_min = 2.220446049250313e-16 if t_min is None else float(t_min)
        seed, n_samples, first_stream, first_sample = int(seed), int(n_samples), int(first_stream), int(first_sample)
        np_dtype = np.float32 if self.precision == RTW_F32 else np.float64
        accumulate = 0 if direct is None else 1
        if type(points).__module__.split(".")[0] == "torch":
            import torch
            want = torch.float32 if self.precision == RTW_F32 else torch.float64
            if points.dtype != want:
                raise RenderError(_capi.RTW_E_INVALID, f"direct_light: tensor dtype {points.dtype}, the context's is {want}")
            if not points.is_cuda or points.device.index != self.device:
                raise RenderError(_capi.RTW_E_INVALID, f"direct_light: the tensor is not on device {self.device}")
            if points.dim() != 2 or points.shape[1] != 6 or not points.is_contiguous():
                raise RenderError(_capi.RTW_E_INVALID, "direct_light: points must be a contiguous [n, 6] tensor")
            n = int(points.shape[0])
            if direct is None:
                direct = torch.zeros((n, 3), dtype=torch.float64, device=points.device)
            elif type(direct).__module__.split(".")[0] != "torch" or direct.dtype != torch.float64 or \
                    direct.device != points.device or tuple(direct.shape) != (n, 3) or not direct.is_contiguous():
                raise RenderError(_capi.RTW_E_INVALID, "direct_light: direct must be a contiguous [n, 3] float64 "
                                                       "tensor on the points' device")
            rows = n * max(n_samples, 0)
            samples = torch.zeros((rows, 12), dtype=want, device=points.device) if records else None
            ids = torch.zeros((rows, 4), dtype=torch.int32, device=points.device) if records else None
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_direct_light_device(
                self.ctx, C.c_void_p(points.data_ptr()) if n else None, points.numel() * points.element_size(), n,
                seed, first_stream, first_sample, n_samples, t_min, accumulate,
                C.c_void_p(direct.data_ptr()) if n else None, direct.numel() * 8,
                C.c_void_p(samples.data_ptr()) if records and rows else None,
                samples.numel() * samples.element_size() if records else 0,
                C.c_void_p(ids.data_ptr()) if records and rows else None, ids.numel() * 4 if records else 0,
                C.c_void_p(stream) if stream else None), "rtw_direct_light_device")
            return (direct, samples, ids) if records else direct
        pts = np.ascontiguousarray(np.asarray(points, np_dtype))
        if pts.ndim != 2 or pts.shape[1] != 6:
            raise RenderError(_capi.RTW_E_INVALID, "direct_light: points must be [n, 6] {p, normal}")
        n = int(pts.shape[0])
        if direct is None:
            direct = np.zeros((n, 3), np.float64)
        else:
            if not (isinstance(direct, np.ndarray) and direct.dtype == np.float64 and direct.flags.c_contiguous):
                direct = np.ascontiguousarray(np.asarray(direct, np.float64))
            if direct.shape != (n, 3):
                raise RenderError(_capi.RTW_E_INVALID, "direct_light: direct must be [n, 3], one sum per point")
        rows = n * max(n_samples, 0)
        samples = np.zeros((rows, 12), np_dtype) if records else None
        ids = np.zeros((rows, 4), np.int32) if records else None
        self._check(_lib.rtw_direct_light(
            self.ctx, pts.ctypes.data_as(C.c_void_p) if n else None, n, seed, first_stream, first_sample, n_samples,
            t_min, accumulate, direct.ctypes.data_as(C.c_void_p) if n else None,
            samples.ctypes.data_as(C.c_void_p) if records and rows else None,
            ids.ctypes.data_as(C.c_void_p) if records and rows else None), "rtw_direct_light")
        return (direct, samples, ids) if records else direct

    def render_direct(self, cam: Camera, seed: int, light_samples: int = 1, first_sample: int = 0,
                      n_samples: int | None = None, sums=None):
        """One direct-light bounce of every pixel: [H, W, 3] f64 sums of
        direct_light at the first hits of the camera samples first_sample ..
        first_sample + n_samples - 1 (n_samples defaults to the camera's
        samples_per_pixel), light_samples light samples at each.  Per camera
        sample s: camera_rays, hit_rays, then direct_light on the records' {p,
        normal} -- miss rows are skipped by the zero-normal rule -- with
        first_stream 0 (the pixel index), first_sample s * light_samples, and
        the seed seed ^ 0x9E3779B97F4A7C15, so the light draws do not reuse
        the camera jitter's stream.  sums: [H, W, 3] f64 to continue (a
        window's), or None.  The caller multiplies by the feature pass's albedo
        and divides by the samples."""
        W, H = int(cam.raw.image_width), int(cam.raw.image_height)
        n_samples = int(cam.samples_per_pixel) if n_samples is None else int(n_samples)
        light_samples, first_sample = int(light_samples), int(first_sample)
        lseed = (int(seed) ^ 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        if sums is None:
            direct = None
        else:
            direct = np.ascontiguousarray(np.asarray(sums, np.float64)).reshape(-1, 3)
            if direct.shape[0] != W * H:
                raise RenderError(_capi.RTW_E_INVALID, "render_direct: sums must be [H, W, 3]")
        for s in range(first_sample, first_sample + n_samples):
            rays, _ = self.camera_rays(cam, seed, s)
            hits, _ = self.hit_rays(rays)
            direct = self.direct_light(np.ascontiguousarray(hits[:, 1:7]), lseed, light_samples, 0,
                                       s * light_samples, direct=direct)
        if direct is None:
            direct = np.zeros((W * H, 3), np.float64)
        return direct.reshape(H, W, 3)

    # ---- ambient occlusion as one query (rtw_ambient_occlusion)
    def ambient_occlusion(self, points, seed: int, n_samples: int = 1, t_max: float | None = None,
                          t_min: float | None = None, first_stream: int = 0, first_sample: int = 0, open=None,
                          records: bool = False):
        """How much of the cosine-weighted hemisphere above n shading points
        [n, 6] {p, normal} (fields 1..6 of a hit_rays record) is open: uint32
        [n], the number of the samples s = first_sample .. first_sample +
        n_samples - 1 whose direction -- CosinePdf::generate in the normal's
        frame, the first two draws of the stream (seed, first_stream + k, s) --
        meets nothing over t_min..=t_max, as occluded answers that ray.  t_max:
        one upper end for the call, None for +inf (the sky); NaN or below t_min
        is an empty range, every sample open.  A point with normal (0, 0, 0) --
        a miss row of hit_rays -- is skipped: its count stays as it is.  open:
        counts to continue ([n] uint32; updated in place when it is a
        contiguous uint32 array, or an int32 tensor holding those bits), or
        None to start from zero, so sample windows compose exactly.
        records=True also returns (directions [n * n_samples, 3], occluded
        [n * n_samples] uint8), row k * n_samples + (s - first_sample).  t_min
        defaults to f64::EPSILON.  numpy in, numpy out (the host entry); torch
        GPU tensors go through the device entry on torch's current stream and
        give the counts as an int32 tensor."""
        t_min = 2.220446049250313e-16 if t_min is None else float(t_min)
        t_max = float("inf") if t_max is None else float(t_max)
        seed, n_samples, first_stream, first_sample = int(seed), int(n_samples), int(first_stream), int(first_sample)
        np_dtype = np.float32 if self.precision == RTW_F32 else np.float64
        accumulate = 0 if open is None else 1
        if type(points).__module__.split(".")[0] == "torch":
            import torch
            want = torch.float32 if self.precision == RTW_F32 else torch.float64
            if points.dtype != want:
                raise RenderError(_capi.RTW_E_INVALID,
                                  f"ambient_occlusion: tensor dtype {points.dtype}, the context's is {want}")
            if not points.is_cuda or points.device.index != self.device:
                raise RenderError(_capi.RTW_E_INVALID, f"ambient_occlusion: the tensor is not on device {self.device}")
            if points.dim() != 2 or points.shape[1] != 6 or not points.is_contiguous():
                raise RenderError(_capi.RTW_E_INVALID, "ambient_occlusion: points must be a contiguous [n, 6] tensor")
            n = int(points.shape[0])
            if open is None:
                open = torch.zeros((n,), dtype=torch.int32, device=points.device)
            elif type(open).__module__.split(".")[0] != "torch" or open.dtype != torch.int32 or \
                    open.device != points.device or tuple(open.shape) != (n,) or not open.is_contiguous():
                raise RenderError(_capi.RTW_E_INVALID, "ambient_occlusion: open must be a contiguous [n] int32 "
                                                       "tensor on the points' device")
            rows = n * max(n_samples, 0)
            dirs = torch.zeros((rows, 3), dtype=want, device=points.device) if records else None
            occ = torch.zeros((rows,), dtype=torch.uint8, device=points.device) if records else None
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_ambient_occlusion_device(
                self.ctx, C.c_void_p(points.data_ptr()) if n else None, points.numel() * points.element_size(), n,
                seed, first_stream, first_sample, n_samples, t_min, t_max, accumulate,
                C.c_void_p(open.data_ptr()) if n else None, open.numel() * 4,
                C.c_void_p(dirs.data_ptr()) if records and rows else None,
                dirs.numel() * dirs.element_size() if records else 0,
                C.c_void_p(occ.data_ptr()) if records and rows else None, occ.numel() if records else 0,
                C.c_void_p(stream) if stream else None), "rtw_ambient_occlusion_device")
            return (open, dirs, occ) if records else open
        pts = np.ascontiguousarray(np.asarray(points, np_dtype))
        if pts.ndim != 2 or pts.shape[1] != 6:
            raise RenderError(_capi.RTW_E_INVALID, "ambient_occlusion: points must be [n, 6] {p, normal}")
        n = int(pts.shape[0])
        if open is None:
            open = np.zeros(n, np.uint32)
        else:
            if not (isinstance(open, np.ndarray) and open.dtype == np.uint32 and open.flags.c_contiguous):
                open = np.ascontiguousarray(np.asarray(open, np.uint32))
            if open.shape != (n,):
                raise RenderError(_capi.RTW_E_INVALID, "ambient_occlusion: open must be [n], one count per point")
        rows = n * max(n_samples, 0)
        dirs = np.zeros((rows, 3), np_dtype) if records else None
        occ = np.zeros(rows, np.uint8) if records else None
        self._check(_lib.rtw_ambient_occlusion(
            self.ctx, pts.ctypes.data_as(C.c_void_p) if n else None, n, seed, first_stream, first_sample, n_samples,
            t_min, t_max, accumulate, open.ctypes.data_as(C.c_void_p) if n else None,
            dirs.ctypes.data_as(C.c_void_p) if records and rows else None,
            occ.ctypes.data_as(C.c_void_p) if records and rows else None), "rtw_ambient_occlusion")
        return (open, dirs, occ) if records else open

    def render_ao(self, cam: Camera, seed: int, ao_samples: int = 1, t_max: float | None = None):
        """An ambient-occlusion pass of every pixel: ([H, W] uint32 open, [H, W]
        uint32 taken).  Per camera sample s of the camera's samples_per_pixel:
        camera_rays, hit_rays, then ambient_occlusion on the records' {p,
        normal} with first_stream 0 (the pixel index), first_sample s *
        ao_samples, and the seed seed ^ 0x9E3779B97F4A7C15 (render_direct's),
        so the draws do not reuse the camera jitter's stream.  A miss row takes
        nothing: its zero normal is skipped, and `taken` counts ao_samples for
        every first hit.  open / taken is the pixel's open share; with t_max
        None it is the sky's."""
        W, H = int(cam.raw.image_width), int(cam.raw.image_height)
        ao_samples = int(ao_samples)
        aseed = (int(seed) ^ 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        open_ = np.zeros(W * H, np.uint32)
        taken = np.zeros(W * H, np.uint32)
        for s in range(int(cam.samples_per_pixel)):
            rays, _ = self.camera_rays(cam, seed, s)
            hits, _ = self.hit_rays(rays)
            pts = np.ascontiguousarray(hits[:, 1:7])
            open_ = self.ambient_occlusion(pts, aseed, ao_samples, t_max, None, 0, s * ao_samples, open=open_)
            taken += np.where((pts[:, 3:6] != 0).any(-1), ao_samples, 0).astype(np.uint32)
        return open_.reshape(H, W), taken.reshape(H, W)

    # ---- radiance along arbitrary rays as one query (rtw_radiance_rays)
    def radiance(self, rays, seed: int, n_samples: int = 1, max_depth: int = 50, background=(0.0, 0.0, 0.0),
                 first_stream: int = 0, first_sample: int = 0, rng=None, radiance=None, records: bool = False):
        """Incoming radiance along n rays [n, 6] {origin, direction}: the f64
        sums [n, 3] of the sample colours s = first_sample .. first_sample +
        n_samples - 1, each Camera::ray_colour_tail_call run to the end of its
        path -- up to max_depth rounds of hit_rays(t_min = f64::EPSILON),
        shade_rays and path_advance's fold, in one kernel.  MISS ends a path
        with mult * background + res, ABSORBED with mult * emitted + res, a
        path alive after max_depth rounds with 0 + res.  Sample s of ray k
        draws from the stream (seed, first_stream + k, s), light_sample's
        keying; with rng ([n, 4] start states, numpy uint64 or a torch int64
        tensor carrying those bits; n_samples must be 1) from the caller's
        state, which is UPDATED IN PLACE -- camera_rays followed by
        radiance(rng=rng) is one sample of a render.  radiance: sums to
        continue ([n, 3] f64; updated in place when it is a contiguous f64
        array or tensor), or None to start from zero, so sample windows
        compose exactly.  NaN is not scrubbed.  records=True also returns
        (colours [n * n_samples, 3] of the context's precision, segments [n *
        n_samples] -- the world.hit calls of the pair; uint32, int32 as a
        tensor), row k * n_samples + (s - first_sample).  numpy in, numpy out
        (the host entry); torch GPU tensors go through the device entry on
        torch's current stream."""
        seed, n_samples, max_depth = int(seed), int(n_samples), int(max_depth)
        first_stream, first_sample = int(first_stream), int(first_sample)
        bg = (C.c_double * 3)(*[float(v) for v in background])
        accumulate = 0 if radiance is None else 1
        r, is_torch = self._query_rays(rays, "radiance")
        n = int(r.shape[0])
        rows = n * max(n_samples, 0)
        if is_torch:
            import torch
            if radiance is None:
                radiance = torch.zeros((n, 3), dtype=torch.float64, device=r.device)
            elif type(radiance).__module__.split(".")[0] != "torch" or radiance.dtype != torch.float64 or \
                    radiance.device != r.device or tuple(radiance.shape) != (n, 3) or not radiance.is_contiguous():
                raise RenderError(_capi.RTW_E_INVALID, "radiance: radiance must be a contiguous [n, 3] float64 "
                                                       "tensor on the rays' device")
            if rng is not None and (type(rng).__module__.split(".")[0] != "torch" or rng.dtype != torch.int64 or
                                    rng.device != r.device or tuple(rng.shape) != (n, 4) or not rng.is_contiguous()):
                raise RenderError(_capi.RTW_E_INVALID, "radiance: rng must be a contiguous [n, 4] int64 tensor on "
                                                       "the rays' device")
            colours = torch.zeros((rows, 3), dtype=r.dtype, device=r.device) if records else None
            segs = torch.zeros((rows,), dtype=torch.int32, device=r.device) if records else None
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_radiance_rays_device(
                self.ctx, C.c_void_p(r.data_ptr()) if n else None, r.numel() * r.element_size(), n, seed,
                first_stream, first_sample, n_samples, max_depth, bg,
                C.c_void_p(rng.data_ptr()) if rng is not None and n else None, rng.numel() * 8 if rng is not None else 0,
                accumulate, C.c_void_p(radiance.data_ptr()) if n else None, radiance.numel() * 8,
                C.c_void_p(colours.data_ptr()) if records and rows else None,
                colours.numel() * colours.element_size() if records else 0,
                C.c_void_p(segs.data_ptr()) if records and rows else None, segs.numel() * 4 if records else 0,
                C.c_void_p(stream) if stream else None), "rtw_radiance_rays_device")
            return (radiance, colours, segs) if records else radiance
        if radiance is None:
            radiance = np.zeros((n, 3), np.float64)
        else:
            if not (isinstance(radiance, np.ndarray) and radiance.dtype == np.float64 and radiance.flags.c_contiguous):
                radiance = np.ascontiguousarray(np.asarray(radiance, np.float64))
            if radiance.shape != (n, 3):
                raise RenderError(_capi.RTW_E_INVALID, "radiance: radiance must be [n, 3], one sum per ray")
        if rng is not None and (not isinstance(rng, np.ndarray) or rng.dtype != np.uint64 or rng.shape != (n, 4) or
                                not rng.flags.c_contiguous or not rng.flags.writeable):
            raise RenderError(_capi.RTW_E_INVALID, "radiance: rng must be a writeable C-contiguous [n, 4] uint64 array "
                                                   "(it is updated in place)")
        colours = np.zeros((rows, 3), r.dtype) if records else None
        segs = np.zeros(rows, np.uint32) if records else None
        self._check(_lib.rtw_radiance_rays(
            self.ctx, r.ctypes.data_as(C.c_void_p) if n else None, n, seed, first_stream, first_sample, n_samples,
            max_depth, bg, rng.ctypes.data_as(C.c_void_p) if rng is not None and n else None, accumulate,
            radiance.ctypes.data_as(C.c_void_p) if n else None,
            colours.ctypes.data_as(C.c_void_p) if records and rows else None,
            segs.ctypes.data_as(C.c_void_p) if records and rows else None), "rtw_radiance_rays")
        return (radiance, colours, segs) if records else radiance

    def render_radiance(self, cam: Camera, seed: int, first_sample: int = 0, n_samples: int | None = None, sums=None):
        """The camera's image through the radiance query: [H, W, 3] f64 sums of
        the samples first_sample .. first_sample + n_samples - 1 of every pixel
        (n_samples defaults to the camera's samples from first_sample on).  Per
        camera sample s: camera_rays, then radiance(rng=rng) with the camera's
        max_depth and background, folded in sample order -- in RTW_F64 the sums
        are render()'s at chunk 1 bit for bit.  sums: [H, W, 3] f64 to continue
        (a window's), or None."""
        W, H = int(cam.raw.image_width), int(cam.raw.image_height)
        first_sample = int(first_sample)
        n_samples = max(int(cam.raw.samples_per_pixel) - first_sample, 0) if n_samples is None else int(n_samples)
        if sums is None:
            acc = np.zeros((W * H, 3), np.float64)
        else:
            acc = np.array(sums, np.float64).reshape(-1, 3)
            if acc.shape[0] != W * H:
                raise RenderError(_capi.RTW_E_INVALID, "render_radiance: sums must be [H, W, 3]")
        for s in range(first_sample, first_sample + n_samples):
            rays, rng = self.camera_rays(cam, seed, s)
            acc = self.radiance(rays, seed, 1, int(cam.raw.max_depth), cam.background, rng=rng, radiance=acc)
        return acc.reshape(H, W, 3)

    # ---- path queries: camera rays and the material bounce (rtw_camera_rays / rtw_shade_rays)
    @staticmethod
    def _pixel_list(pixels):
        """a host list of pixel indices as contiguous uint32 (refused when one is not a uint32)"""
        p64 = np.asarray(pixels, np.int64).reshape(-1)
        if ((p64 < 0) | (p64 > 0xFFFFFFFF)).any():
            raise RenderError(_capi.RTW_E_INVALID, "camera_rays: a pixel index is not a uint32")
        return np.ascontiguousarray(p64.astype(np.uint32))

    def camera_rays(self, cam: Camera, seed: int, sample: int, pixels=None, first_pixel: int = 0, n: int | None = None,
                    *, as_torch: bool = False):
        """Camera::get_ray for n pixels and one sample index: (rays [n, 6]
        {origin, direction} of the context's precision, rng [n, 4] -- the
        xoshiro256++ words of each stream after get_ray's draws).  Ray k is
        pixel index pixels[k] (j * W + i, the render's stream key), or
        first_pixel + k without a list; n defaults to the list's length, or to
        the pixels from first_pixel to the image's end.  The stream is the one a
        render gives to (seed, pixel, sample).  numpy out: rng is uint64 (the
        host entry, which refuses an index >= W * H).  A torch tensor of pixels
        (int32, on this device) or as_torch=True goes through the device entry on
        torch's current stream: torch tensors come back, rng as int64 carrying
        the same bits; there an out-of-range index is the caller's error (it is
        clamped to the last pixel)."""
        W, H = int(cam.raw.image_width), int(cam.raw.image_height)
        seed, sample, first_pixel = int(seed), int(sample), int(first_pixel)
        pix_torch = pixels is not None and type(pixels).__module__.split(".")[0] == "torch"
        if pix_torch or as_torch:
            import torch
            dev = torch.device("cuda", self.device)
            if pixels is not None:
                if not pix_torch:
                    pixels = torch.as_tensor(self._pixel_list(pixels).view(np.int32), device=dev)
                if pixels.dtype != torch.int32 or not pixels.is_cuda or pixels.device.index != self.device or \
                        pixels.dim() != 1 or not pixels.is_contiguous():
                    raise RenderError(_capi.RTW_E_INVALID, "camera_rays: pixels must be a contiguous [n] int32 tensor "
                                                           "on this device")
                n = int(pixels.shape[0]) if n is None else int(n)
                if n > int(pixels.shape[0]):
                    raise RenderError(_capi.RTW_E_INVALID, "camera_rays: n is beyond the pixel list")
            elif n is None:
                n = max(W * H - first_pixel, 0)
            want = torch.float32 if self.precision == RTW_F32 else torch.float64
            rays = torch.zeros((n, 6), dtype=want, device=dev)
            rng = torch.zeros((n, 4), dtype=torch.int64, device=dev)
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_camera_rays_device(
                self.ctx, C.byref(cam.raw), seed, sample,
                C.c_void_p(pixels.data_ptr()) if pixels is not None and n else None,
                pixels.numel() * 4 if pixels is not None else 0, first_pixel, n,
                C.c_void_p(rays.data_ptr()), rays.numel() * rays.element_size(),
                C.c_void_p(rng.data_ptr()), rng.numel() * 8, C.c_void_p(stream) if stream else None),
                "rtw_camera_rays_device")
            return rays, rng
        pix = None
        if pixels is not None:
            pix = self._pixel_list(pixels)
            n = len(pix) if n is None else int(n)
            if n > len(pix):
                raise RenderError(_capi.RTW_E_INVALID, "camera_rays: n is beyond the pixel list")
        elif n is None:
            n = max(W * H - first_pixel, 0)
        rays = np.zeros((n, 6), np.float32 if self.precision == RTW_F32 else np.float64)
        rng = np.zeros((n, 4), np.uint64)
        self._check(_lib.rtw_camera_rays(self.ctx, C.byref(cam.raw), seed, sample,
                                         pix.ctypes.data_as(C.c_void_p) if pix is not None and n else None,
                                         first_pixel, n, rays.ctypes.data_as(C.c_void_p),
                                         rng.ctypes.data_as(C.c_void_p)), "rtw_camera_rays")
        return rays, rng

    def shade_rays(self, rays, hits, ids, rng, pdfs: bool = False):
        """One iteration of ray_colour_tail_call after world.hit for n rays:
        (next [n, 6] {p, direction}, weight [n, 3], emitted [n, 3], event [n]
        int32 RTW_EVENT_*[, pdfs [n, 3] {mixture, light list, scattering}]).
        rays are the incoming rays, hits and ids what hit_rays returned for
        them; rng [n, 4] is each path's xoshiro256++ state, advanced by exactly
        the draws of the reference's branch and UPDATED IN PLACE (MISS rows are
        left as they are).  MISS: the path ends with mult * background + res;
        ABSORBED: with mult * emitted + res; REFLECT: mult *= weight; SCATTER:
        res += mult * emitted, then mult *= weight.  numpy arrays go through the
        host entry (rng uint64, C-contiguous); torch tensors on the GPU through
        the device entry on torch's current stream (rng int64, the same bits)."""
        r, is_torch = self._query_rays(rays, "shade_rays")
        n = int(r.shape[0])
        if is_torch:
            import torch
            for name, t, dt, cols in (("hits", hits, r.dtype, 9), ("ids", ids, torch.int32, 4),
                                      ("rng", rng, torch.int64, 4)):
                if type(t).__module__.split(".")[0] != "torch" or t.dtype != dt or t.device != r.device or \
                        tuple(t.shape) != (n, cols) or not t.is_contiguous():
                    raise RenderError(_capi.RTW_E_INVALID, f"shade_rays: {name} must be a contiguous [n, {cols}] "
                                                           f"{dt} tensor on the rays' device")
            nxt = torch.zeros((n, 6), dtype=r.dtype, device=r.device)
            weight = torch.zeros((n, 3), dtype=r.dtype, device=r.device)
            emitted = torch.zeros((n, 3), dtype=r.dtype, device=r.device)
            event = torch.zeros((n,), dtype=torch.int32, device=r.device)
            pd = torch.zeros((n, 3), dtype=r.dtype, device=r.device) if pdfs else None
            stream = _torch_stream(self.device)
            nb = lambda t: t.numel() * t.element_size()   # noqa: E731
            vp = lambda t: C.c_void_p(t.data_ptr()) if n else None   # noqa: E731
            self._check(_lib.rtw_shade_rays_device(
                self.ctx, vp(r), nb(r), vp(hits), nb(hits), vp(ids), nb(ids), n, vp(rng), nb(rng), vp(nxt), nb(nxt),
                vp(weight), nb(weight), vp(emitted), nb(emitted), vp(event), nb(event),
                vp(pd) if pdfs else None, nb(pd) if pdfs else 0, C.c_void_p(stream) if stream else None),
                "rtw_shade_rays_device")
            return (nxt, weight, emitted, event, pd) if pdfs else (nxt, weight, emitted, event)
        h = np.ascontiguousarray(np.asarray(hits, r.dtype))
        i4 = np.ascontiguousarray(np.asarray(ids, np.int32))
        if h.shape != (n, 9) or i4.shape != (n, 4):
            raise RenderError(_capi.RTW_E_INVALID, "shade_rays: hits must be [n, 9] and ids [n, 4], as hit_rays returns them")
        if not isinstance(rng, np.ndarray) or rng.dtype != np.uint64 or rng.shape != (n, 4) or \
                not rng.flags.c_contiguous or not rng.flags.writeable:
            raise RenderError(_capi.RTW_E_INVALID, "shade_rays: rng must be a writeable C-contiguous [n, 4] uint64 array "
                                                   "(it is updated in place)")
        nxt = np.zeros((n, 6), r.dtype)
        weight = np.zeros((n, 3), r.dtype)
        emitted = np.zeros((n, 3), r.dtype)
        event = np.zeros(n, np.int32)
        pd = np.zeros((n, 3), r.dtype) if pdfs else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if n else None   # noqa: E731
        self._check(_lib.rtw_shade_rays(self.ctx, vp(r), vp(h), vp(i4), n, vp(rng), vp(nxt), vp(weight), vp(emitted),
                                        vp(event), vp(pd) if pdfs else None), "rtw_shade_rays")
        return (nxt, weight, emitted, event, pd) if pdfs else (nxt, weight, emitted, event)

    def render_wavefront(self, cam: Camera, seed: int, first_sample: int = 0, n_samples: int | None = None,
                         on_bounce=None, *, sums=None, as_torch: bool = False):
        """The reference's integrator as a loop over the queries -- a wavefront
        path tracer: the sums [H, W, 3] (float64) of the samples [first_sample,
        first_sample + n_samples) of every pixel (n_samples defaults to the
        camera's samples from first_sample on).  Per sample: camera_rays, then up
        to max_depth rounds of hit_rays(t_min = f64::EPSILON) and shade_rays on
        the paths still alive (compacted each round); a MISS ends a path with
        mult * background + res, ABSORBED with mult * emitted + res, a path alive
        after max_depth rounds with 0 + res (camera.rs:470-521).  Samples are added
        in sample order onto `sums` ([H, W, 3] float64 of an earlier window; None:
        zeros), so windows compose bit for bit, and in RTW_F64 the image is
        render()'s bit for bit.  It is the tool for AOVs, light-path expressions
        and integrators written outside the library, not a faster render:
        measured 20-30x slower than render() at 1200 x 800 x 4 samples and
        40-60x at 256 x 160 -- about 0.5 ms of host work a round (two query calls
        and some twenty small array operations), whatever the image.
        on_bounce(depth, paths, rays, hits, ids, event, weight, emitted), when
        given, is called each round before the paths are compacted (depth counts
        rounds from 0, paths are the pixel indices j * W + i of the live paths,
        the arrays are that round's, row for row): the hook for AOVs and
        light-path expressions.  It runs once per round of every sample, in
        sample order.  as_torch keeps every array on the GPU (torch tensors on
        torch's current stream; the sums come back as a float64 tensor)."""
        W, H = int(cam.raw.image_width), int(cam.raw.image_height)
        first_sample = int(first_sample)
        n_samples = max(int(cam.raw.samples_per_pixel) - first_sample, 0) if n_samples is None else int(n_samples)
        depth_max = int(cam.raw.max_depth)
        np_dtype = np.float32 if self.precision == RTW_F32 else np.float64
        if as_torch:
            import torch
            dev = torch.device("cuda", self.device)
            t_dtype = torch.float32 if self.precision == RTW_F32 else torch.float64
            bg = torch.tensor([float(v) for v in cam.background], dtype=t_dtype, device=dev)
            sums = torch.zeros((H * W, 3), dtype=torch.float64, device=dev) if sums is None else \
                torch.as_tensor(sums, dtype=torch.float64, device=dev).reshape(H * W, 3)
            new = lambda n, v: torch.full((n, 3), v, dtype=t_dtype, device=dev)   # noqa: E731
            where = lambda m: torch.nonzero(m).reshape(-1)                        # noqa: E731
            f64 = lambda a: a.to(torch.float64)                                   # noqa: E731
            contig = lambda a: a.contiguous()                                     # noqa: E731
        else:
            bg = np.asarray(cam.background, np_dtype)
            sums = np.zeros((H * W, 3), np.float64) if sums is None else \
                np.array(sums, np.float64).reshape(H * W, 3)
            new = lambda n, v: np.full((n, 3), v, np_dtype)   # noqa: E731
            where = lambda m: np.nonzero(m)[0]                 # noqa: E731
            f64 = lambda a: a.astype(np.float64)               # noqa: E731
            contig = np.ascontiguousarray
        for s in range(first_sample, first_sample + n_samples):
            rays, rng = self.camera_rays(cam, seed, s, as_torch=as_torch)
            n = int(rays.shape[0])
            if as_torch:
                paths = torch.arange(n, device=rays.device)
            else:
                paths = np.arange(n)
            mult, res, colour = new(n, 1.0), new(n, 0.0), new(n, 0.0)
            for depth in range(depth_max):
                if int(paths.shape[0]) == 0:
                    break
                hits, ids = self.hit_rays(rays)
                nxt, weight, emitted, event = self.shade_rays(rays, hits, ids, rng)
                if on_bounce is not None:
                    on_bounce(depth, paths, rays, hits, ids, event, weight, emitted)
                miss, gone = where(event == _capi.RTW_EVENT_MISS), where(event == _capi.RTW_EVENT_ABSORBED)
                colour[paths[miss]] = mult[miss] * bg + res[miss]                  # camera.rs:473-475
                colour[paths[gone]] = mult[gone] * emitted[gone] + res[gone]       # camera.rs:484-486
                scat = where(event == _capi.RTW_EVENT_SCATTER)
                res[scat] = res[scat] + mult[scat] * emitted[scat]                 # camera.rs:519
                keep = where(event >= _capi.RTW_EVENT_REFLECT)
                mult = mult[keep] * weight[keep]                                   # camera.rs:496, 518
                res, paths = res[keep], paths[keep]
                rays, rng = contig(nxt[keep]), contig(rng[keep])
            if int(paths.shape[0]):
                colour[paths] = 0.0 + res                                          # camera.rs:470-472
            sums = sums + f64(colour)
        return sums.reshape(H, W, 3)

    # ---- wavefront path rounds on the device (rtw_path_begin_device / rtw_path_advance / rtw_render_wavefront)
    def path_begin(self, n: int, first_slot: int = 0):
        """The state n paths start from, as torch tensors on this device
        (rtw_path_begin_device on torch's current stream): (mult [n, 3] of ones,
        res [n, 3] of zeros, slot [n] int32 carrying the uint32 first_slot + k)."""
        import torch
        n, first_slot = int(n), int(first_slot)
        if n < 0 or first_slot < 0 or first_slot + n > 1 << 32:
            raise RenderError(_capi.RTW_E_INVALID, "path_begin: first_slot + n is beyond 2^32 slots")
        dev = torch.device("cuda", self.device)
        dt = torch.float32 if self.precision == RTW_F32 else torch.float64
        mult = torch.empty((n, 3), dtype=dt, device=dev)
        res = torch.empty((n, 3), dtype=dt, device=dev)
        slot = torch.empty((n,), dtype=torch.int32, device=dev)
        stream = _torch_stream(self.device)
        nb = lambda t: t.numel() * t.element_size()                  # noqa: E731
        vp = lambda t: C.c_void_p(t.data_ptr()) if n else None       # noqa: E731
        self._check(_lib.rtw_path_begin_device(self.ctx, n, first_slot, vp(mult), nb(mult), vp(res), nb(res), vp(slot),
                                               nb(slot), C.c_void_p(stream) if stream else None),
                    "rtw_path_begin_device")
        return mult, res, slot

    def path_advance(self, mult, res, slot, event, weight, emitted, nxt, rng, colour, background, last: bool = False,
                     *, out=None):
        """One round's bookkeeping on the device (rtw_path_advance, include/rtw.h):
        from the state (mult, res, slot) the round started with and what
        shade_rays returned for its rays (event, weight, emitted, nxt, and the
        rng it advanced), a path that ends writes colour[slot] (MISS: mult *
        background + res; ABSORBED: mult * emitted + res; with `last` a survivor:
        0 + res'), and the survivors' state (rays, rng, mult, res, slot) comes
        back, cut to the survivor count -- the one readback of the round.  Rows:
        the survivors of each 256 input paths stay together and in order, the
        blocks in any order; slot names the path.  colour [slots, 3] is UPDATED
        IN PLACE.  numpy arrays (rng uint64, slot uint32, event int32) go through
        the host entry, which refuses a slot beyond colour; torch tensors on the
        GPU (rng int64, slot int32, the same bits) through the device entry on
        torch's current stream, where such a path's colour is skipped.  out: five
        arrays / tensors of at least n rows to write the survivors into (rows
        beyond the count are left as they are); none may overlap an input."""
        bg = (C.c_double * 3)(*[float(v) for v in background])
        if type(mult).__module__.split(".")[0] == "torch":
            import torch
            dt = torch.float32 if self.precision == RTW_F32 else torch.float64
            n = int(mult.shape[0])
            dev = mult.device
            spec = (("mult", mult, dt, (n, 3)), ("res", res, dt, (n, 3)), ("slot", slot, torch.int32, (n,)),
                    ("event", event, torch.int32, (n,)), ("weight", weight, dt, (n, 3)),
                    ("emitted", emitted, dt, (n, 3)), ("nxt", nxt, dt, (n, 6)), ("rng", rng, torch.int64, (n, 4)))
            for name, t, d, shape in spec:
                if type(t).__module__.split(".")[0] != "torch" or t.dtype != d or not t.is_cuda or \
                        t.device.index != self.device or tuple(t.shape) != shape or not t.is_contiguous():
                    raise RenderError(_capi.RTW_E_INVALID, f"path_advance: {name} must be a contiguous {list(shape)} "
                                                           f"{d} tensor on device {self.device}")
            if type(colour).__module__.split(".")[0] != "torch" or colour.dtype != dt or colour.device != dev or \
                    colour.dim() != 2 or colour.shape[1] != 3 or not colour.is_contiguous():
                raise RenderError(_capi.RTW_E_INVALID, "path_advance: colour must be a contiguous [slots, 3] tensor of "
                                                       "the context's precision on the state's device")
            if out is None:
                out = (torch.empty((n, 6), dtype=dt, device=dev), torch.empty((n, 4), dtype=torch.int64, device=dev),
                       torch.empty((n, 3), dtype=dt, device=dev), torch.empty((n, 3), dtype=dt, device=dev),
                       torch.empty((n,), dtype=torch.int32, device=dev))
            o_spec = (("rays", dt, 6), ("rng", torch.int64, 4), ("mult", dt, 3), ("res", dt, 3), ("slot", torch.int32, 0))
            for (name, d, cols), t in zip(o_spec, out):
                if t.dtype != d or t.device != dev or not t.is_contiguous() or t.dim() != (2 if cols else 1) or \
                        (cols and t.shape[1] != cols):
                    raise RenderError(_capi.RTW_E_INVALID, f"path_advance: out {name} has the wrong dtype, shape or device")
            count = torch.zeros((1,), dtype=torch.int64, device=dev)
            stream = _torch_stream(self.device)
            nb = lambda t: t.numel() * t.element_size()                  # noqa: E731
            vp = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None   # noqa: E731
            args = []
            for t in (mult, res, slot, event, weight, emitted, nxt, rng, *out, colour):
                args += [vp(t), nb(t)]
            self._check(_lib.rtw_path_advance_device(self.ctx, n, *args, int(colour.shape[0]), bg, 1 if last else 0,
                                                     C.c_void_p(count.data_ptr()),
                                                     C.c_void_p(stream) if stream else None), "rtw_path_advance_device")
            m = int(count.item())
            return tuple(t[:m] for t in out)
        dt = np.float32 if self.precision == RTW_F32 else np.float64
        as_c = lambda a, d: np.ascontiguousarray(np.asarray(a, d))   # noqa: E731
        mult, res, weight, emitted, nxt = (as_c(a, dt) for a in (mult, res, weight, emitted, nxt))
        slot, event, rng = as_c(slot, np.uint32), as_c(event, np.int32), as_c(rng, np.uint64)
        n = int(mult.shape[0])
        for name, a, shape in (("mult", mult, (n, 3)), ("res", res, (n, 3)), ("slot", slot, (n,)), ("event", event, (n,)),
                               ("weight", weight, (n, 3)), ("emitted", emitted, (n, 3)), ("nxt", nxt, (n, 6)),
                               ("rng", rng, (n, 4))):
            if a.shape != shape:
                raise RenderError(_capi.RTW_E_INVALID, f"path_advance: {name} must be {list(shape)}")
        if not isinstance(colour, np.ndarray) or colour.dtype != dt or colour.ndim != 2 or colour.shape[1] != 3 or \
                not colour.flags.c_contiguous or not colour.flags.writeable:
            raise RenderError(_capi.RTW_E_INVALID, "path_advance: colour must be a writeable C-contiguous [slots, 3] array "
                                                   "of the context's precision (it is updated in place)")
        if out is None:
            out = (np.zeros((n, 6), dt), np.zeros((n, 4), np.uint64), np.zeros((n, 3), dt), np.zeros((n, 3), dt),
                   np.zeros(n, np.uint32))
        o_spec = (("rays", dt, (6,)), ("rng", np.uint64, (4,)), ("mult", dt, (3,)), ("res", dt, (3,)), ("slot", np.uint32, ()))
        for (name, d, tail), a in zip(o_spec, out):
            if not isinstance(a, np.ndarray) or a.dtype != d or a.shape[1:] != tail or a.shape[0] < n or \
                    not a.flags.c_contiguous or not a.flags.writeable:
                raise RenderError(_capi.RTW_E_INVALID, f"path_advance: out {name} must be a writeable C-contiguous "
                                                       f"array of at least n rows")
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None   # noqa: E731
        m = C.c_uint64(0)
        self._check(_lib.rtw_path_advance(self.ctx, n, *[vp(a) for a in (mult, res, slot, event, weight, emitted, nxt,
                                                                         rng, *out, colour)],
                                          int(colour.shape[0]), bg, 1 if last else 0, C.byref(m)), "rtw_path_advance")
        return tuple(a[:m.value] for a in out)

    def render_wavefront_batched(self, cam: Camera, seed: int, first_sample: int = 0, n_samples: int | None = None, *,
                                 batch: int = 0, sums=None, on_bounce=None, as_torch: bool = False):
        """render_wavefront with its rounds kept on the device
        (rtw_render_wavefront): the sums [H, W, 3] float64 of the samples
        [first_sample, first_sample + n_samples), added in sample order onto
        `sums` -- the same bits as render_wavefront, in RTW_F64 render()'s at
        chunk 1.  The samples run `batch` at a time through the same rounds (0:
        as many as keep a round at 2^22 paths), so there are max_depth rounds a
        batch, not a sample, and one 8-byte readback a round.  Without a hook
        this is the C driver (as_torch: on torch's current stream, device sums in
        and out).  With on_bounce the same batched loop runs here over
        camera_rays / hit_rays / shade_rays / path_advance on torch tensors, and
        the hook is called each round with render_wavefront's signature; paths
        are the slots b * W * H + pixel of the live paths (b: the sample's place
        in its batch), an int64 tensor, and the arrays are tensors on the GPU."""
        W, H = int(cam.raw.image_width), int(cam.raw.image_height)
        first_sample, batch = int(first_sample), int(batch)
        n_samples = max(int(cam.raw.samples_per_pixel) - first_sample, 0) if n_samples is None else int(n_samples)
        if batch < 0 or n_samples < 0 or first_sample < 0:
            raise RenderError(_capi.RTW_E_INVALID, "render_wavefront_batched: a negative sample window or batch")
        if on_bounce is None and not as_torch:
            out = np.zeros((H, W, 3), np.float64) if sums is None else \
                np.array(sums, np.float64).reshape(H, W, 3)
            self._check(_lib.rtw_render_wavefront(self.ctx, C.byref(cam.raw), int(seed), first_sample, n_samples, batch,
                                                  out.ctypes.data_as(C.POINTER(C.c_double))), "rtw_render_wavefront")
            return out
        import torch
        dev = torch.device("cuda", self.device)
        acc = torch.zeros((H, W, 3), dtype=torch.float64, device=dev) if sums is None else \
            torch.as_tensor(sums, dtype=torch.float64, device=dev).reshape(H, W, 3).clone()
        if on_bounce is None:
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_render_wavefront_device(self.ctx, C.byref(cam.raw), int(seed), first_sample, n_samples,
                                                         batch, C.c_void_p(acc.data_ptr()), acc.numel() * 8,
                                                         C.c_void_p(stream) if stream else None),
                        "rtw_render_wavefront_device")
            return acc
        px, depth_max = W * H, int(cam.raw.max_depth)
        dt = torch.float32 if self.precision == RTW_F32 else torch.float64
        B = min(batch if batch else max((1 << 22) // max(px, 1), 1), n_samples)
        flat = acc.reshape(px, 3)
        done = 0
        while done < n_samples:
            nb = min(B, n_samples - done)
            pairs = [self.camera_rays(cam, seed, first_sample + done + b, as_torch=True) for b in range(nb)]
            rays = torch.cat([p[0] for p in pairs]) if nb > 1 else pairs[0][0]
            rng = torch.cat([p[1] for p in pairs]) if nb > 1 else pairs[0][1]
            mult, res, slot = self.path_begin(nb * px)
            colour = torch.zeros((nb * px, 3), dtype=dt, device=dev)
            for depth in range(depth_max):
                if int(rays.shape[0]) == 0:
                    break
                hits, ids = self.hit_rays(rays)
                nxt, weight, emitted, event = self.shade_rays(rays, hits, ids, rng)
                on_bounce(depth, slot.to(torch.int64) & 0xFFFFFFFF, rays, hits, ids, event, weight, emitted)
                rays, rng, mult, res, slot = self.path_advance(mult, res, slot, event, weight, emitted, nxt, rng, colour,
                                                               cam.background, last=depth == depth_max - 1)
            for b in range(nb):
                flat += colour[b * px:(b + 1) * px].to(torch.float64)
            done += nb
        return acc if as_torch else acc.cpu().numpy()

    # ---- feature buffers for denoisers (rtw_render_features)
    def render_features(self, cam: Camera, seed: int, first: int = 0, n: int | None = None, *, counts=None,
                        features=None, want_ids: bool = True):
        """First-hit guides of the render's own primary rays: (features
        [H, W, 8] float64 sums {albedo rgb, normal xyz, distance, hits}, ids
        [H, W, 2] int32 {object id or -1, material id} of each pixel's sample 0,
        or None).  Pixel p folds the samples [first, min(first + n,
        counts[p])) in order onto `features` (zeros when None; n defaults to
        cam.samples_per_pixel - first), so windows and counts compose bit for
        bit with a one-shot pass, and render_adaptive's counts with n =
        max_samples give the guides of exactly the samples each colour was
        made of.  The ids are written by a call with first == 0 only (None
        when first > 0 or want_ids is false).  Sums, not means: see
        feature_means.  numpy arrays (or None) go through the host entry; with
        a torch GPU tensor as `features` or `counts` the call goes through the
        device entry on torch's current stream, without a host copy, `features`
        is updated in place and torch tensors come back.  rtw_get_query_stats
        then holds the pass's counters."""
        H, W = cam.raw.image_height, cam.raw.image_width
        first = int(first)
        n = max(int(cam.raw.samples_per_pixel) - first, 0) if n is None else int(n)
        with_ids = bool(want_ids) and first == 0
        is_torch = [type(a).__module__.split(".")[0] == "torch" for a in (features, counts)]
        if any(is_torch):
            import torch
            dev = torch.device("cuda", self.device)
            for a, t, dt, shape, what in ((features, is_torch[0], torch.float64, (H, W, 8), "features"),
                                          (counts, is_torch[1], torch.int32, (H, W), "counts")):
                if a is None:
                    continue
                ok_dt = t and (a.dtype == dt or (what == "counts" and a.dtype == getattr(torch, "uint32", dt)))
                if not (ok_dt and a.is_cuda and a.device.index == self.device and a.is_contiguous()
                        and tuple(a.shape) == shape):
                    raise RenderError(_capi.RTW_E_INVALID, f"render_features: {what} must be a contiguous "
                                      f"{list(shape)} {dt} tensor on device {self.device}")
            if features is None:
                features = torch.zeros((H, W, 8), dtype=torch.float64, device=dev)
            ids = torch.zeros((H, W, 2), dtype=torch.int32, device=dev) if with_ids else None
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_render_features_device(
                self.ctx, C.byref(cam.raw), C.c_uint64(seed), first, n,
                C.c_void_p(counts.data_ptr()) if counts is not None else None,
                counts.numel() * 4 if counts is not None else 0,
                C.c_void_p(features.data_ptr()), features.numel() * 8,
                C.c_void_p(ids.data_ptr()) if ids is not None else None, ids.numel() * 4 if ids is not None else 0,
                C.c_void_p(stream) if stream else None), "rtw_render_features_device")
            return features, ids
        if features is None:
            features = np.zeros((H, W, 8), np.float64)
        elif not (isinstance(features, np.ndarray) and features.dtype == np.float64 and features.shape == (H, W, 8)
                  and features.flags.c_contiguous and features.flags.writeable):
            raise RenderError(_capi.RTW_E_INVALID, f"render_features: features must be a C-contiguous float64 "
                              f"array of shape {(H, W, 8)}")
        cnt = None
        if counts is not None:
            cnt = np.ascontiguousarray(np.asarray(counts, np.uint32))
            if cnt.shape != (H, W):
                raise RenderError(_capi.RTW_E_INVALID, f"render_features: counts must have shape {(H, W)}")
        ids = np.zeros((H, W, 2), np.int32) if with_ids else None
        self._check(_lib.rtw_render_features(
            self.ctx, C.byref(cam.raw), C.c_uint64(seed), first, n,
            cnt.ctypes.data_as(C.c_void_p) if cnt is not None else None, features.ctypes.data_as(C.c_void_p),
            ids.ctypes.data_as(C.c_void_p) if ids is not None else None), "rtw_render_features")
        return features, ids

    # ---- the denoiser (rtw_denoise)
    def denoise(self, sums, features, n, **params):
        """The edge-avoiding a-trous filter of include/rtw.h over a render's
        colour sums [H, W, 3], the feature sums [H, W, 8] of render_features
        for the same samples and n, the sample count or the [H, W] counts of an
        adaptive render: the filtered per-sample MEANS [H, W, 3] float64
        (display them with spp = 1).  Keyword parameters as DenoiseParams
        (iterations, normal_power_log2, sigma_colour, sigma_depth, demodulate,
        fill_nonfinite); those left out take the library's defaults.  numpy
        arrays go through the host entry (float32 sums are widened exactly
        first); torch GPU tensors -- float32 or float64 sums, float64 features,
        int32 / uint32 counts -- go through the device entry on torch's current
        stream, without a host copy, and a torch tensor comes back.  No scene
        is needed; on a multi-device Renderer the filter runs on the first
        device."""
        p = DenoiseParams(**params).raw
        if type(sums).__module__.split(".")[0] == "torch":
            import torch
            H, W = int(sums.shape[0]), int(sums.shape[1])
            per_pixel = type(n).__module__.split(".")[0] == "torch"
            checks = [(sums, (torch.float32, torch.float64), (H, W, 3), "sums"),
                      (features, (torch.float64,), (H, W, 8), "features")]
            if per_pixel:
                checks.append((n, (torch.int32, getattr(torch, "uint32", torch.int32)), (H, W), "counts"))
            for a, dts, shape, what in checks:
                if not (type(a).__module__.split(".")[0] == "torch" and a.dtype in dts and a.is_cuda
                        and a.device.index == self.device and a.is_contiguous() and tuple(a.shape) == shape):
                    raise RenderError(_capi.RTW_E_INVALID, f"denoise: {what} must be a contiguous {list(shape)} "
                                      f"tensor of {dts} on device {self.device}")
            out = torch.empty((H, W, 3), dtype=torch.float64, device=sums.device)
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_denoise_device(
                self.ctx, C.c_void_p(sums.data_ptr()), RTW_F32 if sums.dtype == torch.float32 else RTW_F64,
                sums.numel() * sums.element_size(), C.c_void_p(features.data_ptr()), features.numel() * 8,
                C.c_void_p(n.data_ptr()) if per_pixel else None, n.numel() * 4 if per_pixel else 0,
                0 if per_pixel else int(n), W, H, C.byref(p), C.c_void_p(out.data_ptr()), out.numel() * 8,
                C.c_void_p(stream) if stream else None), "rtw_denoise_device")
            return out
        s = np.ascontiguousarray(np.asarray(sums), np.float64)
        if s.ndim != 3 or s.shape[2] != 3:
            raise RenderError(_capi.RTW_E_INVALID, f"denoise: sums must be [H, W, 3], got {list(s.shape)}")
        H, W = s.shape[:2]
        f = np.ascontiguousarray(np.asarray(features), np.float64)
        if f.shape != (H, W, 8):
            raise RenderError(_capi.RTW_E_INVALID, f"denoise: features must be {[H, W, 8]}, got {list(f.shape)}")
        cnt = _counts(n, H, W)
        out = np.zeros((H, W, 3), np.float64)
        self._check(_lib.rtw_denoise(self.ctx, s.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p),
                                     cnt.ctypes.data_as(C.c_void_p) if cnt is not None else None,
                                     0 if cnt is not None else int(n), W, H, C.byref(p),
                                     out.ctypes.data_as(C.c_void_p)), "rtw_denoise")
        return out

    # ---- the variance-guided denoiser (rtw_denoise_variance)
    def denoise_variance(self, sums, features, moments, n, **params):
        """The variance-guided a-trous filter of include/rtw.h: denoise's
        inputs plus the luminance moments [H, W, 2] float64 of the same samples
        (render_window_moments, adaptive_moments), whose per-pixel standard
        error scales the colour stop.  Returns the filtered per-sample MEANS
        [H, W, 3] float64.  Keyword parameters as DenoiseVarianceParams
        (iterations, normal_power_log2, sigma_var, sigma_depth, demodulate,
        fill_nonfinite).  numpy arrays go through the host entry; torch GPU
        tensors -- float32 or float64 sums, float64 features and moments, int32
        / uint32 counts -- through the device entry on torch's current stream,
        and a torch tensor comes back."""
        p = DenoiseVarianceParams(**params).raw
        if type(sums).__module__.split(".")[0] == "torch":
            import torch
            H, W = int(sums.shape[0]), int(sums.shape[1])
            per_pixel = type(n).__module__.split(".")[0] == "torch"
            checks = [(sums, (torch.float32, torch.float64), (H, W, 3), "sums"),
                      (features, (torch.float64,), (H, W, 8), "features"),
                      (moments, (torch.float64,), (H, W, 2), "moments")]
            if per_pixel:
                checks.append((n, (torch.int32, getattr(torch, "uint32", torch.int32)), (H, W), "counts"))
            for a, dts, shape, what in checks:
                if not (type(a).__module__.split(".")[0] == "torch" and a.dtype in dts and a.is_cuda
                        and a.device.index == self.device and a.is_contiguous() and tuple(a.shape) == shape):
                    raise RenderError(_capi.RTW_E_INVALID, f"denoise_variance: {what} must be a contiguous "
                                      f"{list(shape)} tensor of {dts} on device {self.device}")
            out = torch.empty((H, W, 3), dtype=torch.float64, device=sums.device)
            stream = _torch_stream(self.device)
            self._check(_lib.rtw_denoise_variance_device(
                self.ctx, C.c_void_p(sums.data_ptr()), RTW_F32 if sums.dtype == torch.float32 else RTW_F64,
                sums.numel() * sums.element_size(), C.c_void_p(features.data_ptr()), features.numel() * 8,
                C.c_void_p(moments.data_ptr()), moments.numel() * 8,
                C.c_void_p(n.data_ptr()) if per_pixel else None, n.numel() * 4 if per_pixel else 0,
                0 if per_pixel else int(n), W, H, C.byref(p), C.c_void_p(out.data_ptr()), out.numel() * 8,
                C.c_void_p(stream) if stream else None), "rtw_denoise_variance_device")
            return out
        s = np.ascontiguousarray(np.asarray(sums), np.float64)
        if s.ndim != 3 or s.shape[2] != 3:
            raise RenderError(_capi.RTW_E_INVALID, f"denoise_variance: sums must be [H, W, 3], got {list(s.shape)}")
        H, W = s.shape[:2]
        f = np.ascontiguousarray(np.asarray(features), np.float64)
        if f.shape != (H, W, 8):
            raise RenderError(_capi.RTW_E_INVALID,
                              f"denoise_variance: features must be {[H, W, 8]}, got {list(f.shape)}")
        m = np.ascontiguousarray(np.asarray(moments), np.float64)
        if m.shape != (H, W, 2):
            raise RenderError(_capi.RTW_E_INVALID,
                              f"denoise_variance: moments must be {[H, W, 2]}, got {list(m.shape)}")
        cnt = _counts(n, H, W)
        out = np.zeros((H, W, 3), np.float64)
        self._check(_lib.rtw_denoise_variance(
            self.ctx, s.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p),
            cnt.ctypes.data_as(C.c_void_p) if cnt is not None else None, 0 if cnt is not None else int(n), W, H,
            C.byref(p), out.ctypes.data_as(C.c_void_p)), "rtw_denoise_variance")
        return out

    def denoise_stats(self) -> "_capi.rtw_denoise_stats":
        """Counters of the last denoise (rtw_get_denoise_stats; waits for it):
        iterations, lds_iterations, filled, left_nonfinite, kernel_ms."""
        st = _capi.rtw_denoise_stats()
        self._check(_lib.rtw_get_denoise_stats(self.ctx, C.byref(st)), "rtw_get_denoise_stats")
        return st

    def get_query_stats(self) -> "_capi.rtw_query_stats":
        """Counters of the last query (rtw_get_query_stats): rays, hits, node
        visits, sphere tests, light tests, the world / light path that ran."""
        st = _capi.rtw_query_stats()
        self._check(_lib.rtw_get_query_stats(self.ctx, C.byref(st)), "rtw_get_query_stats")
        return st


class _RankView(Renderer):
    """One rank of a multi-device Renderer (not owned: close() is a no-op).
    It keeps its parent alive and refuses to run once the parent is closed
    (the rank's context is freed with it)."""

    def __init__(self, parent, k, ctx, device, precision):   # noqa: D107  (no rtw_create)
        self._parent = parent
        self._k = k
        self._sub = ctx
        self.device = device
        self.precision = precision
        self.stats = _capi.rtw_stats()

    @property
    def ctx(self):
        if self._parent is None or not self._parent.ctx:
            raise RenderError(_capi.RTW_E_INVALID, "rank view of a closed Renderer")
        return self._sub

    def get_stats(self) -> "_capi.rtw_stats":
        """This rank's own counters (rtw_get_stats_rank; rank 0 too)."""
        self.ctx
        self._check(_lib.rtw_get_stats_rank(self._parent.ctx, self._k, C.byref(self.stats)), "rtw_get_stats_rank")
        return self.stats

    def close(self):
        self._parent = None

    __del__ = close


def tiles_for_rank(width: int, height: int, rank: int, nranks: int) -> int:
    """8x8 tiles rank `rank` of `nranks` renders (rtw_tiles_for_rank)."""
    return int(_lib.rtw_tiles_for_rank(width, height, rank, nranks))


def tile_size() -> int:
    return int(_lib.rtw_tile_size())


def n_tiles(width: int, height: int) -> int:
    t = tile_size()
    return ((width + t - 1) // t) * ((height + t - 1) // t)


def split_deal(tile_cost, width: int, height: int, nranks: int) -> np.ndarray:
    """The tiles dealt to nranks ranks by cost (rtw_split_deal): uint32
    tile -> rank, each rank keeping its round-robin tile count."""
    n = n_tiles(width, height)
    cost = np.ascontiguousarray(np.asarray(tile_cost, np.uint32).reshape(-1))
    if cost.size != n:
        raise RenderError(_capi.RTW_E_INVALID, f"tile_cost needs {n} entries, got {cost.size}")
    out = np.zeros(n, np.uint32)
    rc = _lib.rtw_split_deal(cost.ctypes.data_as(_capi._u32p), width, height, nranks, out.ctypes.data_as(_capi._u32p))
    if rc != 0:
        raise RenderError(rc, "rtw_split_deal failed")
    return out


RTW_STREAM_NULL = 1   # include/rtw.h: the device's null (legacy default) stream


def torch_stream(device: int) -> int:
    """The rtw stream argument for torch's current stream on `device` (the
    Renderer's device, whatever torch's current device is): its hipStream_t,
    or RTW_STREAM_NULL when that is torch's default stream (handle 0, the
    device's null stream -- passing 0 would mean the context's own,
    unordered stream); 0 -- the context's own stream -- when torch has no GPU."""
    try:
        import torch
        if torch.cuda.is_available():
            h = int(torch.cuda.current_stream(device).cuda_stream)
            return h if h else RTW_STREAM_NULL
    except ImportError:
        pass
    return 0


_torch_stream = torch_stream


# ---------------------------------------------------------------- scenes
class scenes:                                 # scenes/src/lib.rs
    @staticmethod
    def simple_soa(seed: int = 0x5EED0001, n: int = 11):
        """(SceneSoA, CameraBuilder) straight from the C++ generator."""
        w = _lib.rtw_scene_simple(C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), n)
        if not w:
            raise RenderError(_capi.RTW_E_INVALID, "rtw_scene_simple failed")
        try:
            soa = SceneSoA.from_c(_lib.rtw_world_scene(w).contents)
            b = _capi.rtw_camera_builder()
            _lib.rtw_world_camera_builder(w, C.byref(b))
        finally:
            _lib.rtw_world_free(w)
        return soa, CameraBuilder(b)

    NAMES = ("cornell_box", "debug", "checkered_spheres", "perlin_spheres", "plane", "simple",
             "simple_light", "simple_transform")      # bin/src/main.rs:29-38

    @staticmethod
    def named_soa(name: str, seed: int = 0x5EED0001):
        """(SceneSoA, CameraBuilder) of a reference scene by its main.rs name
        (scenes.NAMES); `seed` drives simple's generator and the Perlin tables."""
        w = _lib.rtw_scene_named(name.encode(), C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF))
        if not w:
            raise RenderError(_capi.RTW_E_UNSUPPORTED, f"scene {name!r} is not in this build")
        try:
            soa = SceneSoA.from_c(_lib.rtw_world_scene(w).contents)
            b = _capi.rtw_camera_builder()
            _lib.rtw_world_camera_builder(w, C.byref(b))
        finally:
            _lib.rtw_world_free(w)
        return soa, CameraBuilder(b)

    @staticmethod
    def cornell_box_soa():
        return scenes.named_soa("cornell_box")

    @staticmethod
    def simple(seed: int = 0x5EED0001, n: int = 11):
        """scenes::simple -> (world, lights, CameraBuilder) as object lists."""
        soa, builder = scenes.simple_soa(seed, n)
        world, lights = HittableList(), HittableList()
        for pl, m in zip(soa.planes, soa.plane_mat):
            world.add(Plane(tuple(pl[:3]), tuple(pl[3:]), _mat(soa, m)))
        for sp, m in zip(soa.spheres, soa.sphere_mat):
            world.add(Sphere(tuple(sp[:3]), float(sp[3]), _mat(soa, m)))
        for li in soa.lights:
            lights.add(Sphere(tuple(li[:3]), float(li[3]), INVISIBLE))
        return world, lights, builder


def _mat(soa, m):
    p = soa.mat_params[m]
    return Material(int(soa.mat_type[m]), (float(p[0]), float(p[1]), float(p[2])), float(p[3]),
                    float(p[4]))


# ---------------------------------------------------------------- output
def _sums(sums: np.ndarray):
    """(contiguous array, ctypes pointer, f32?) of float32 or float64 sums."""
    if np.asarray(sums).dtype == np.float32:
        s = np.ascontiguousarray(sums, np.float32)
        return s, s.ctypes.data_as(_capi._f32p), True
    s = np.ascontiguousarray(sums, np.float64)
    return s, s.ctypes.data_as(_capi._f64p), False


def _counts(spp, H, W):
    """None for a sample count; for an array of per-pixel counts (an adaptive
    render's) the contiguous uint32 [H, W] array."""
    if np.ndim(spp) == 0:
        return None
    c = np.ascontiguousarray(spp, np.uint32)
    if c.shape != (H, W):
        raise RenderError(_capi.RTW_E_INVALID, f"counts must be [H, W] = [{H}, {W}], got {list(c.shape)}")
    return c


def encode_rgb8(sums: np.ndarray, spp) -> np.ndarray:
    """SampledColour Display (colour.rs:14-36), rows flipped top-first: uint8 [H, W, 3].
    float32 sums (a speed-mode render) are widened to f64 exactly first.  spp:
    the sample count, or the [H, W] counts of an adaptive render (each pixel
    then divides by its own)."""
    s, ptr, f32 = _sums(sums)
    H, W = s.shape[:2]
    out = np.zeros((H, W, 3), np.uint8)
    c = _counts(spp, H, W)
    if c is not None:
        s = np.ascontiguousarray(s, np.float64)
        _lib.rtw_encode_rgb8_counts(s.ctypes.data_as(_capi._f64p), c.ctypes.data_as(_capi._u32p), W, H,
                                    out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out
    fn = _lib.rtw_encode_rgb8_f32 if f32 else _lib.rtw_encode_rgb8
    fn(ptr, W, H, spp, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def write_ppm(path: str, sums: np.ndarray, spp) -> int:
    """The reference's P3 image.ppm (bin/src/main.rs:89-104); spp as encode_rgb8's."""
    s, ptr, f32 = _sums(sums)
    H, W = s.shape[:2]
    c = _counts(spp, H, W)
    if c is not None:
        s = np.ascontiguousarray(s, np.float64)
        n = _lib.rtw_write_ppm_counts(path.encode(), s.ctypes.data_as(_capi._f64p), c.ctypes.data_as(_capi._u32p),
                                      W, H)
    else:
        n = (_lib.rtw_write_ppm_f32 if f32 else _lib.rtw_write_ppm)(path.encode(), ptr, W, H, spp)
    if n < 0:
        raise RenderError(n, f"cannot write {path}")
    return n


class DenoiseParams:
    """rtw_denoise_params: the library's defaults (rtw_denoise_params_default)
    with the given fields replaced -- iterations (1..16), normal_power_log2
    (0..10), sigma_colour (>= 0; 0: no colour weight), sigma_depth (> 0),
    demodulate, fill_nonfinite (0 / 1).  The library checks the ranges."""
    FIELDS = tuple(f for f, _ in _capi.rtw_denoise_params._fields_)

    def __init__(self, **fields):
        self.raw = _capi.rtw_denoise_params()
        _lib.rtw_denoise_params_default(C.byref(self.raw))
        for k, v in fields.items():
            if k not in self.FIELDS:
                raise RenderError(_capi.RTW_E_INVALID, f"DenoiseParams has no field {k!r} (it has {self.FIELDS})")
            setattr(self.raw, k, float(v) if k.startswith("sigma") else int(v))

    def __getattr__(self, name):
        return getattr(self.__dict__["raw"], name)

    def as_dict(self):
        return {f: getattr(self.raw, f) for f in self.FIELDS}


class DenoiseVarianceParams:
    """rtw_denoise_variance_params: the library's defaults
    (rtw_denoise_variance_params_default) with the given fields replaced --
    iterations (1..16), normal_power_log2 (0..10), sigma_var (>= 0: the colour
    stop's width in standard errors of the centre pixel), sigma_depth (> 0),
    demodulate, fill_nonfinite (0 / 1).  The library checks the ranges."""
    FIELDS = tuple(f for f, _ in _capi.rtw_denoise_variance_params._fields_)

    def __init__(self, **fields):
        self.raw = _capi.rtw_denoise_variance_params()
        _lib.rtw_denoise_variance_params_default(C.byref(self.raw))
        for k, v in fields.items():
            if k not in self.FIELDS:
                raise RenderError(_capi.RTW_E_INVALID,
                                  f"DenoiseVarianceParams has no field {k!r} (it has {self.FIELDS})")
            setattr(self.raw, k, float(v) if k.startswith("sigma") else int(v))

    def __getattr__(self, name):
        return getattr(self.__dict__["raw"], name)

    def as_dict(self):
        return {f: getattr(self.raw, f) for f in self.FIELDS}


def feature_means(features, n):
    """The guides a denoiser reads from render_features' sums [H, W, 8], for
    the sample count n (a number, or the [H, W] counts the pass was given):
    (albedo [H, W, 3] = sums / n, normal [H, W, 3] = the normal sum normalised
    (0 where no sample hit), distance [H, W] = sum / hits (inf where no sample
    hit), coverage [H, W] = hits / n).  A pixel with n = 0 has albedo and
    coverage 0.  Pure numpy."""
    f = np.asarray(features, np.float64)
    if f.ndim != 3 or f.shape[2] != 8:
        raise RenderError(_capi.RTW_E_INVALID, f"features must be [H, W, 8], got {list(f.shape)}")
    cnt = np.broadcast_to(np.asarray(n, np.float64), f.shape[:2])
    hits = f[..., 7]
    with np.errstate(divide="ignore", invalid="ignore"):
        sampled = cnt > 0
        albedo = np.where(sampled[..., None], f[..., 0:3] / cnt[..., None], 0.0)
        coverage = np.where(sampled, hits / cnt, 0.0)
        length = np.sqrt((f[..., 3:6] ** 2).sum(-1))
        normal = np.where((length > 0)[..., None], f[..., 3:6] / length[..., None], 0.0)
        distance = np.where(hits > 0, f[..., 6] / hits, np.inf)
    return albedo, normal, distance, coverage
