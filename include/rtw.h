/*
 * rtw.h -- C-ABI of the MI355X (gfx950) path tracer: the drop-in boundary for
 * the reference's per-pixel / per-sample ray_colour loop.
 *
 * Reference interfaces replaced (paths relative to N9199/ray_tracing_weekend):
 *   Camera::render(&self, world: &dyn Hittable, lights: &dyn Hittable)
 *       -> Vec<Vec<SampledColour>>            shared/src/camera.rs:295-297
 *   Camera::render_debug(...)                 shared/src/camera.rs:299-312
 *   (both through render_internal            shared/src/camera.rs:315-388)
 *   CameraBuilder::build(self) -> Camera      shared/src/camera.rs:114-218
 *   scenes::simple() (the input producer)     scenes/src/lib.rs:155-233
 *   SampledColour Display / PPM writer        shared/src/colour.rs:14-36,136-148;
 *                                             bin/src/main.rs:89-104
 *
 * Plain C types only (no torch, no HIP types): pointers, sizes, POD structs.
 * Every entry point returns 0 on success and a negative RTW_E* code on error
 * (the reference panics instead; this library never aborts the caller).
 * The rtw_ctx is reentrant across contexts; one context is single-threaded.
 * The GPU work runs on gfx950 only; there is no CPU fallback in this library.
 *
 * Output convention (mirrors render_internal's Vec<Vec<Colour>> before it is
 * wrapped in SampledColour): out[(j * W + i) * 3 + c] is the SUM of the
 * samples of pixel (i, j) -- not the mean -- and j = 0 is the BOTTOM row
 * (camera.rs:179-188: viewport_v = +v * h).  NaN samples are not scrubbed
 * (the live integrator never calls fix_nan, camera.rs:459-522).
 */
#ifndef RTW_H
#define RTW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_ABI_VERSION 10

/* error codes */
#define RTW_OK 0
#define RTW_E_INVALID (-1)       /* bad argument / inconsistent scene */
#define RTW_E_DEVICE (-2)        /* HIP runtime error (message in rtw_last_error) */
#define RTW_E_NO_LIGHTS (-3)     /* a Lambertian bounce drew a light sample from an empty
                                    light list: hittable_list.rs:417 panics there */
#define RTW_E_NO_SCENE (-4)      /* render before a scene was set */
#define RTW_E_UNSUPPORTED (-5)   /* scene/feature outside this build's scope */
#define RTW_E_PANIC (-6)         /* the render reached a point where the reference panics:
                                    a non-finite plane UV (plane.rs:66-69) */

/* precision of the device arithmetic */
#define RTW_F32 0                /* speed mode: f32 + FMA + native sqrt/rcp/sin/cos */
#define RTW_F64 1                /* parity mode: f64, no FMA contraction, same op order
                                    as the reference (bit-comparable with the oracle) */
/* Supported range of the parity mode.  Its kernels cull candidates with f32
 * filters (a widened slab test, pre-passes before the f64 sphere and light
 * tests, an f32 walk of the light grid) that must never drop what the f64 test
 * accepts.  What is tested, with zero exceptions allowed:
 *   - whole renders, the light grid's walk included: scenes and cameras scaled
 *     by 2^-40 .. 2^40, translated by up to 2^22, focus_dist 2^-30 .. 2^30,
 *     light queries from 10^4 away.  This is the supported range;
 *   - the pre-passes and the slab tests alone, primitive by primitive: sizes
 *     2^-130 .. 2^130 with |d| = 2^-30 .. 2^30 -- where a coordinate or its
 *     square leaves f32's range they keep every candidate.  The light grid's
 *     f32 walk does NOT fail open there (beyond f32 its box test is NaN and
 *     the ray "misses the grid"), so whole renders beyond 2^+-40 are not
 *     promised;
 *   - a ray direction must keep d . d, its reciprocal and d . (o - c) normal
 *     f32 numbers: |d|_1 within 2^-60 .. 2^46 (the reference never normalises
 *     directions: a camera's primary rays have the length of focus_dist,
 *     scattered rays about 1).  A camera scaled by 2^-70 (|d| = 2^-67) renders
 *     wrong pixels: the leaf pre-pass drops spheres the reference hits;
 *   - direction components that are exactly +-0 are fine in the parity mode.
 *     The speed mode (RTW_F32) can lose boxes for a ray with a component
 *     exactly 0 beside a non-zero origin component. */

/* material kinds (shared/src/material.rs) */
#define RTW_LAMBERTIAN 0         /* material.rs:327-376 (SolidColour texture) */
#define RTW_METAL 1              /* material.rs:378-421 */
#define RTW_DIELECTRIC 2         /* material.rs:423-488 ("Dialectric") */
#define RTW_INVISIBLE 3          /* material.rs:321-325 */
#define RTW_DIFFUSE_LIGHT 4      /* material.rs:490-514: emits albedo, scatter() None */

/* texture kinds (shared/src/texture.rs) */
#define RTW_TEX_SOLID 0          /* SolidColour, texture.rs:15-22 */
#define RTW_TEX_CHECKER 1        /* CheckerTexture, texture.rs:24-55 */
#define RTW_TEX_NOISE 2          /* NoiseTexture over a Perlin table, texture.rs:57-102, perlin.rs */

/* light-list entry kinds (rtw_scene.light_kinds) */
#define RTW_LIGHT_SPHERE 0       /* Sphere::pdf_value / random, sphere.rs:101-127 */
#define RTW_LIGHT_QUAD 1         /* Quad::pdf_value / random, quadrilateral.rs:100-118 */
#define RTW_LIGHT_DEFAULT 2      /* a hittable without its own pdf (Plane, Transformed<Cuboid>):
                                    the trait defaults pdf_value = 0, random = (1, 0, 0),
                                    hittable.rs:175-181 */
/* rtw_scene.light_flags */
#define RTW_LIGHTS_BVH_LEAF 1    /* the light list is a BoundedVolumeHierarchy of <= 5 entries
                                    (a leaf): pdf_value = (sum / n * n) / n, bvh.rs:67-76,191-194 */

/* Stream arguments (hipStream_t as void*): NULL = the context's own stream
 * (non-blocking); RTW_STREAM_NULL = the device's null (legacy default)
 * stream, which orders with every blocking stream -- e.g. PyTorch's default
 * stream, whose handle is 0; anything else is a hipStream_t of that device. */
#define RTW_STREAM_NULL ((void *)1)

/* World acceleration used by the render kernel */
#define RTW_ACCEL_AUTO 0         /* pick per scene */
#define RTW_ACCEL_BRUTE 1        /* every ray tests every sphere, sphere list in LDS */
#define RTW_ACCEL_BVH 2          /* device BVH (closest-hit semantics unchanged) */

/* CameraBuilder (camera.rs:29-42).  has_* == 0 encodes Option::None. */
typedef struct rtw_camera_builder {
    int32_t has_aspect_ratio, has_image_width, has_image_height;
    double aspect_ratio;
    uint32_t image_width, image_height;
    uint32_t samples_per_pixel;  /* u16 in the reference */
    uint32_t max_depth;
    double background[3];
    double vfov;
    double lookfrom[3], lookat[3], vup[3];
    double defocus_angle, focus_dist;
} rtw_camera_builder;

/* The derived Camera fields the render loop reads (camera.rs:228-261). */
typedef struct rtw_camera {
    uint32_t image_width, image_height;
    uint32_t samples_per_pixel, max_depth;
    double background[3];
    double defocus_angle;
    double center[3], pixel00_loc[3], pixel_delta_u[3], pixel_delta_v[3];
    double defocus_disk_u[3], defocus_disk_v[3];
} rtw_camera;

/* Flattened world + lights, struct-of-arrays, caller-owned host memory.
 * world  = planes + spheres + quads + transformed cuboids (closest hit over
 *          all of them, bvh.rs:164-188), materials and their textures
 * lights = the light list in order: spheres, quads and entries with the
 *          Hittable defaults (HittableList::pdf_value / random,
 *          hittable_list.rs:408-419) */
typedef struct rtw_scene {
    uint32_t n_spheres;
    const double *spheres;        /* n_spheres x {cx, cy, cz, radius} */
    const uint32_t *sphere_mat;   /* n_spheres material ids */
    uint32_t n_planes;
    const double *planes;         /* n_planes x {px, py, pz, nx, ny, nz}, unit normal */
    const uint32_t *plane_mat;
    uint32_t n_materials;
    const uint32_t *mat_type;     /* RTW_LAMBERTIAN ... RTW_DIFFUSE_LIGHT */
    const double *mat_params;     /* n_materials x {albedo r, g, b, fuzz, ior} */
    uint32_t n_lights;
    const double *lights;         /* n_lights x {cx, cy, cz, radius}: the light list's spheres */
    /* Quads (quadrilateral.rs:21-56): Quad::new(Q, u, v, mat) */
    uint32_t n_quads;
    const double *quads;          /* n_quads x {Qx, Qy, Qz, ux, uy, uz, vx, vy, vz} */
    const uint32_t *quad_mat;
    uint32_t n_light_quads;
    const double *light_quads;    /* the light list's quads, n x 9 as quads */
    /* light-list order (HittableList insertion order, hittable_list.rs:408-419):
     * n_lights + n_light_quads + n_light_other RTW_LIGHT_* kinds, each taking
     * the next entry of its array (RTW_LIGHT_DEFAULT has no data);
     * NULL = all spheres, then all quads */
    const uint32_t *light_kinds;
    /* Transformed<Cuboid> (cuboid.rs:26-71, entities/transformations.rs:10-30):
     * Cuboid::new(p, q, mat) under the composed Transformation (rotation R,
     * translation T; Transformation::then order, geometry transformations.rs) */
    uint32_t n_boxes;
    const double *boxes;          /* n_boxes x {p xyz, q xyz, R[3][3] row-major, T xyz} = 18 */
    const uint32_t *box_mat;
    /* Textures (texture.rs, perlin.rs).  mat_tex == NULL: every material's
     * colour is the SolidColour albedo in mat_params.  Otherwise mat_tex[m] is
     * the texture of material m (Lambertian attenuation, DiffuseLight emission),
     * evaluated at the hit's (u, v, p) (sphere.rs:49-54, plane.rs:40-54,
     * quadrilateral.rs:58-63):
     *   RTW_TEX_SOLID    tex_params {r, g, b, -}
     *   RTW_TEX_CHECKER  tex_params {-, -, -, inv_scale = 1 / scale}, tex_refs {even, odd} texture ids
     *   RTW_TEX_NOISE    tex_params {-, -, -, scale}, tex_refs {Perlin table id, -} */
    const uint32_t *mat_tex;
    uint32_t n_textures;
    const uint32_t *tex_type;
    const double *tex_params;     /* n_textures x 4 */
    const uint32_t *tex_refs;     /* n_textures x 2 */
    uint32_t n_perlin;
    const double *perlin_vec;     /* n_perlin x 256 x 3: Perlin::rand_vec */
    const uint32_t *perlin_perm;  /* n_perlin x 3 x 256: perm_x, perm_y, perm_z (0..255) */
    /* light-list entries of kind RTW_LIGHT_DEFAULT (light_kinds == 2) */
    uint32_t n_light_other;
    uint32_t light_flags;         /* RTW_LIGHTS_BVH_LEAF */
} rtw_scene;

typedef struct rtw_stats {
    uint64_t samples;             /* W*H*spp of the rendered tiles */
    uint64_t segments;            /* world.hit calls */
    uint64_t lambertian;          /* Scatter-branch bounces (light pdf loop) */
    double kernel_ms;             /* device time of the last render (HIP events) */
    uint32_t accel;               /* RTW_ACCEL_* actually used */
    uint32_t chunk;               /* samples per work item */
    uint64_t node_visits;         /* BVH inner nodes entered (RTW_ACCEL_BVH) */
    uint64_t sphere_tests;        /* ray-sphere discriminant evaluations */
    uint32_t bvh_width;           /* child boxes tested per node visit (4, 2; 0 = no BVH) */
    uint32_t kernel;              /* render-kernel variant: 0 brute/L2, 1 brute/LDS, 2 BVH one
                                     loop, 3 BVH while-while, 4 BVH 4-wide, 5 BVH while-while
                                     with the tree in LDS */
    /* samples that reached a reference panic (the render then returns an
     * error): a non-finite plane UV (plane.rs:66-69) -> RTW_E_PANIC;
     * HittableList::random on an empty light list (hittable_list.rs:417)
     * -> RTW_E_NO_LIGHTS */
    uint64_t panic_plane_uv, panic_no_lights;
    /* light-pdf work (ABI 9): light tests = (bounce, light) pairs tested by the
     * light pdf -- every Lambertian bounce x every light for the linear list
     * loop (hittable_list.rs:408-412), the lights of the big list, the visited
     * grid cells or light-BVH leaves for the light grid / BVH (counted by the
     * kernel); grid_cells = light-grid cells those walks visited.  For the
     * light grid these are WALK-WORK counters, not properties of the samples:
     * the cooperative walks visit a piece boundary's cell twice, size pieces
     * by the wave's pending cells and count a re-walk again, so they depend
     * on how rays are grouped into waves (the image does not). */
    uint64_t light_tests, grid_cells;
} rtw_stats;

typedef struct rtw_ctx rtw_ctx;

/* ---- context ---------------------------------------------------------- */
int rtw_abi_version(void);
/* A context on one GPU (HIP device index `device`). */
rtw_ctx *rtw_create(int device, int precision);
/* A context over several GPUs of this node: SURVEY.md §8(b)(1)'s
 * rtw_create(device_mask, precision), the drop-in for render_internal's use of
 * every host core (camera.rs:340-353: one rayon task per pixel over the
 * global pool) -- here one rank per GPU, all in the calling process.
 * devices[k] is rank k's HIP device; rank k renders the 8x8 tiles
 * T = k (mod n_devices) (rtw_tiles_for_rank), and ONE RCCL gather
 * (ncclGather, rccl.h:745-746, a single-process clique from ncclCommInitAll)
 * brings the ranks' packed tiles to rank 0's device, which un-interleaves them
 * (rtw_assemble_tiles).  Every knob (rtw_set_tuning / rtw_set_chunk /
 * rtw_set_accel) and the scene (rtw_set_scene, staged once) apply to all
 * ranks; rtw_render and rtw_render_image_device render on all of them, and
 * the image is bit-identical to a one-GPU render of the same seed.
 * RTW_E_INVALID: NULL / empty list, a negative, repeated or not visible
 * device (checked before any HIP call for the first two); RTW_E_DEVICE: a HIP
 * or RCCL failure (RCCL is loaded at run time: librccl.so.1). */
int rtw_create_devices(const int *devices, uint32_t n_devices, int precision, rtw_ctx **out);
/* The same over the devices whose bits are set (bit k = HIP device k, in
 * increasing order); NULL on error (an empty mask included). */
rtw_ctx *rtw_create_mask(uint64_t device_mask, int precision);
/* rtw_create_mask with its error code (ABI 9): RTW_E_INVALID for an empty mask
 * or a device that is not visible (compare rtw_visible_devices), RTW_E_DEVICE
 * for a HIP / RCCL failure -- which a caller must not answer by dropping GPUs. */
int rtw_create_mask_ex(uint64_t device_mask, int precision, rtw_ctx **out);
/* HIP devices visible to this process (RTW_E_DEVICE if HIP fails). */
int rtw_visible_devices(void);
/* TEST MODE (ABI 9): a multi-device context of n_ranks ranks that all live on
 * one device, with every product code path of rtw_create_devices -- per-rank
 * contexts, streams, work buffers and scene copies, rank 0 rendering into its
 * gather slot, the equal-size slots, the assembly, the summed stats -- except
 * the transport: the gather is n_ranks - 1 device copies on rank 0's stream,
 * each after its rank's render, instead of ncclGather.  It lets a one-GPU box
 * execute and check the n-rank path; RCCL stays the only product transport. */
int rtw_create_virtual(int device, uint32_t n_ranks, int precision, rtw_ctx **out);
/* Ranks of a context (1 for rtw_create), and rank k's per-device context
 * (k = 0: ctx itself) for rtw_get_stats / rtw_get_timings / rtw_last_kernel
 * of that rank; owned by ctx (do not destroy).  rtw_device_of: its HIP device. */
uint32_t rtw_device_count(const rtw_ctx *ctx);
rtw_ctx *rtw_device_ctx(rtw_ctx *ctx, uint32_t k);
int rtw_device_of(const rtw_ctx *ctx);
void rtw_destroy(rtw_ctx *ctx);
const char *rtw_last_error(const rtw_ctx *ctx);
int rtw_precision(const rtw_ctx *ctx);
/* knobs: samples per work item (0 = auto), acceleration (RTW_ACCEL_*) */
int rtw_set_chunk(rtw_ctx *ctx, uint32_t chunk);
int rtw_set_accel(rtw_ctx *ctx, int accel);
/* scheduling knobs (benchmarking): "chunk" (samples per item, 0 = auto),
 * "auto_chunk", "group" (chunks per wave task, 0 = auto: 4..32), "target_tasks"
 * (auto group: about this many tasks; 0 = 2^17),
 * "persist" (workgroups of persistent waves that take tasks from a global counter;
 * 1 = as many as are resident at once, the default; 0 = one task per wave),
 * "query_grid" (testing: the ray queries, the feature pass and the wavefront rounds --
 * rtw_hit_rays, rtw_light_pdf_rays, rtw_occluded_rays, rtw_light_sample, rtw_camera_rays,
 * rtw_shade_rays, rtw_path_begin_device, rtw_path_advance, rtw_render_wavefront and
 * rtw_render_features, their device forms included -- launch at most this many workgroups,
 * each walking its blocks of 256 rays (or taking its tiles) one after another; 0 = as many
 * as are resident at once, the default; clamped to 2^20.  Every answer is the same at any
 * value, only the order of rtw_path_advance's blocks in the out-state follows the grid; no
 * render kernel reads it),
 * "lds" (1 = stage the sphere list in LDS when it fits, 0 = read it from HBM),
 * "robust" (f32 ray-sphere tests in closest-approach form: 1 on, 0 off,
 * 2 = by the scene's distance-to-radius ratio, the default),
 * "item_order" (wave item pool: 1 = sample-major, the default; 0 = pixel-major),
 * "lpt" (longest tiles first: the segments of each pixel's first 2 samples,
 * summed per tile, order the tasks, cached until the scene, camera or rank split
 * changes; 1 = for worlds held in LDS or of at most 4 MiB (an XCD's L2), the
 * default, 2 = for every world, 0 = tiles in index order),
 * "lpt_inline" (1 = the default: the first render of a scene / camera / split
 * runs in tile index order and counts those segments itself, the next render
 * reads them back (waiting for it once) and takes the ordered tasks; 0 = a
 * blocking 2-spp pilot render before the first render),
 * "lpt_pilot_spp" (samples per pixel counted, default 2), "lpt_pilot_depth" (the
 * separate pilot's max depth, 0 = the camera's),
 * "lpt_min_spp" (renders of fewer samples per pixel keep the index order, default 32),
 * "bvh_leaf" (spheres per BVH leaf, 1..15; 0 = auto, the default: 4, 8 for
 * scenes of >= 100k spheres, 2 for f64 contexts on scenes of 4096..100k; takes effect at the
 * next rtw_set_scene), "light_bvh_min" (light lists this long or longer take the light grid
 * or light BVH in the BVH kernels, default 64), "light_grid" (light-grid resolution in
 * 1/16 cells per light, default 8; 0 = the light BVH instead; next rtw_set_scene),
 * "max_group" (longest-first task list: at most this many chunks per task, default 32),
 * "grid_piece" (f32 light-grid walks: cells per piece of the wave's cooperative walk,
 * default by grid size: its widest side / 14, 4..16; 0 = every lane walks its own ray),
 * "light_leaf" (light spheres per light-BVH leaf, 1..15; 0 = 4), "partial_max" (bytes of chunk sums an auto chunk may use, default 128 GiB, at most half the device's memory; an auto chunk doubles if the allocation fails),
 * "bvh_kind" (3 = binary while-while on the tree staged in LDS, the
 * default, 1 = binary while-while from L1/L2, 2 = 4-wide octant BVH, 0 =
 * binary single loop), "bvh_lds_max" (LDS bytes per workgroup bvh_kind 3 may
 * use; 0 = by precision: 36 KiB f32, 52 KiB f64), "bvh_ww" (legacy: 1 -> bvh_kind 1, 0 -> 0), "auto_accel",
 * "window" (sample windows, the one key that takes a negative value: 0 = off, the
 * default; N > 0 = every render of more than N samples per pixel runs N samples at a
 * time -- N rounded up to a multiple of an explicit chunk -- onto an f64 accumulator of
 * the context, so the chunk sums hold one window instead of the whole render; -1 = the
 * largest window whose chunk sums fit "partial_max", the auto chunk then stays 1 at any
 * spp.  Same image as the one-shot render at the same chunk, bit for bit; stats cover the
 * whole render; rtw_get_timings then lists the windows) */
int rtw_set_tuning(rtw_ctx *ctx, const char *key, int64_t value);

/* ---- CameraBuilder::build (camera.rs:114-218) ------------------------- */
int rtw_camera_build(const rtw_camera_builder *builder, rtw_camera *out);
/* CameraBuilder::new() defaults (camera.rs:45-60) */
void rtw_camera_builder_default(rtw_camera_builder *out);

/* ---- scene ------------------------------------------------------------ */
/* Validate, convert to the device layout and upload (copied; the caller may
 * free its arrays afterwards). */
int rtw_set_scene(rtw_ctx *ctx, const rtw_scene *scene);

/* ---- Camera::render (camera.rs:295-297) ------------------------------- */
/* Synchronous drop-in: uploads `scene` (if non-NULL), renders every pixel and
 * writes H*W*3 doubles (sums, j = 0 bottom row) to host `out_sum`.  On a
 * multi-device context every GPU renders its share (rtw_create_devices);
 * `stats` then sums the ranks' counters (kernel_ms: the slowest rank). */
int rtw_render(rtw_ctx *ctx, const rtw_camera *cam, const rtw_scene *scene,
               uint64_t seed, double *out_sum, rtw_stats *stats);

/* The whole image into device memory of the context's first device: d_image
 * holds H*W*3 elements of the context's precision (sums, j = 0 bottom row).
 * Asynchronous on `stream` (a hipStream_t of that device; NULL = the
 * context's own): rank 0 renders on it, the other ranks on their own
 * streams; the RCCL gather and the assembly are ordered on `stream` after
 * every rank's render, so work queued on `stream` afterwards sees the image. */
int rtw_render_image_device(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed, void *d_image,
                            size_t image_bytes, void *stream);

/* Device-resident form for benchmarking and multi-GPU sharding.
 * The image is cut into 8x8 tiles T = ty * tiles_x + tx (tiles_x = ceil(W/8),
 * row j = 0 at the bottom); rank `rank` of `nranks` renders the tiles
 * T = rank, rank + nranks, ... (a fine interleave: every rank samples the
 * whole image, so the ranks' costs match).  d_out receives them packed: a
 * device buffer of rtw_tiles_for_rank(W, H, rank, nranks) * 64 * 3 elements of
 * the context's precision (float or double), the rank's k-th tile at
 * d_out[(k * 64 + ly * 8 + lx) * 3 + c] (pixels outside the image: 0).
 * d_out may be NULL when the rank has no tiles.  Asynchronous on `stream`
 * (a hipStream_t; NULL = the context's own stream).  No host synchronisation
 * inside, except once per (scene, camera, rank split) when tuning "lpt" is on
 * and spp >= "lpt_min_spp": the second render of the key waits for the first,
 * whose tile costs order its tasks, and reads them back (then cached; with
 * "lpt_inline" 0 the first render runs and reads back a 2-spp pilot instead).
 * On a multi-device context it renders on the first device only (each rank's
 * context: rtw_device_ctx). */
int rtw_render_device(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed,
                      uint32_t rank, uint32_t nranks, void *d_out, size_t out_bytes,
                      void *stream);

/* ---- sample windows: progressive and resumable renders -----------------
 * Every (pixel, sample) has its own RNG stream, so a render can be taken a
 * window of samples at a time and its running per-pixel sums continued later:
 * windows [0, a), [a, b), ... folded one after another give the one-shot
 * render of b samples at the same chunk bit for bit, in both precisions (the
 * running sums are f64 whatever the context's precision: the f32 one-shot
 * fold also accumulates in f64 and rounds once). */
/* Samples [first_sample, first_sample + n_samples) of this rank's tiles, folded
 * in sample order onto d_accum: tiles_for_rank * 64 * 3 doubles (always f64),
 * packed like rtw_render_device's d_out, the sums of samples [0, first_sample)
 * on entry (ignored when first_sample == 0) and of [0, first_sample + n_samples)
 * afterwards.  cam->samples_per_pixel is not read.  Asynchronous on `stream`.
 * n_samples == 0 does nothing.  RTW_E_INVALID when first_sample + n_samples
 * overflows, first_sample is not a multiple of the chunk (rtw_set_chunk; the
 * auto chunk is 1), d_accum is NULL or accum_bytes too small; RTW_E_UNSUPPORTED
 * on a multi-device context (rtw_render_window_image and tuning "window" serve
 * those).  Stats are the window's. */
int rtw_render_window_device(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed,
                             uint32_t rank, uint32_t nranks,
                             uint32_t first_sample, uint32_t n_samples,
                             double *d_accum, size_t accum_bytes, void *stream);
/* Host form, one-device contexts: sums is H*W*3 doubles (j = 0 bottom row),
 * read when first_sample > 0, written with the continued sums. Synchronous. */
int rtw_render_window(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed,
                      uint32_t first_sample, uint32_t n_samples,
                      double *sums, rtw_stats *stats);

/* ---- adaptive sampling: converged tiles stop between sample passes -------
 * Opt-in; no other entry point changes.  Pass 0 renders samples [0,
 * min_samples) of every 8x8 tile; pass k the next `window` samples (up to
 * max_samples) of the tiles still active, one sample per item.  The fold keeps,
 * per pixel and in f64, the three colour sums (the additions of a window
 * render, in sample order) and S1 = sum Y, S2 = sum Y*Y of the samples'
 * luminance Y = ((0.2126 r) + (0.7152 g)) + (0.0722 b).  After a pass that
 * ends at n samples a pixel is settled when S1 or S2 is not finite, or when
 *     m = S1 / n,  q = S2 / n,  var = fmax(q - m*m, 0),  v = var / (n - 1),
 *     v <= ((4 * tolerance) * tolerance) * fmax(m, 2^-16)
 * (every operation a separately rounded f64 operation): the standard error of
 * the displayed value sqrt(mean) is at most `tolerance`, the mean floored at
 * one 8-bit level squared.  A tile stops when all its pixels inside the image
 * are settled, or at max_samples, and never resumes; all pixels of a tile
 * share its count.  So sums[pixel] is the sequential f64 fold of the pixel's
 * first counts[pixel] samples: rtw_render_window(first 0, n = counts) at
 * chunk 1, bit for bit.  Stopping on the samples' own variance biases the
 * estimate slightly (pixels whose first samples happen to agree stop early).
 * sums: H*W*3 doubles, j = 0 the bottom row; counts: H*W.  cam->
 * samples_per_pixel and the tuning key "window" are not read.  RTW_E_INVALID
 * (nothing launched): a NULL pointer, min_samples < 2, max_samples <
 * min_samples, window == 0, a negative or non-finite tolerance, an explicit
 * rtw_set_chunk above 1; RTW_E_UNSUPPORTED on a multi-device context
 * (rtw_render_adaptive_image serves those); RTW_E_NO_SCENE.  An image without pixels renders nothing (stats of no
 * samples).  Stats cover the whole render: samples = the sum of counts,
 * the counters summed over the passes, chunk = 1.  Synchronous. */
int rtw_render_adaptive(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed,
                        uint32_t min_samples, uint32_t max_samples, uint32_t window,
                        double tolerance, double *sums, uint32_t *counts, rtw_stats *stats);
/* Device form: the image-order sums and counts into device memory of the
 * context's device (RTW_E_INVALID when a buffer is NULL or too small).  The
 * work runs on `stream`, but the call synchronises with the host once per
 * pass: it reads back how many tiles go on.  The buffers are complete in
 * stream order when it returns. */
int rtw_render_adaptive_device(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed,
                               uint32_t min_samples, uint32_t max_samples, uint32_t window,
                               double tolerance, double *d_sums, size_t sums_bytes,
                               uint32_t *d_counts, size_t counts_bytes, void *stream);
/* ---- windows and adaptive sampling over every device of the context -------
 * rtw_render_device is the rank form and rtw_render_image_device the whole
 * image over all ranks; these are the whole-image forms of the window and
 * adaptive entry points above.  Semantics, argument checks and error codes are
 * those of the one-device forms, which keep refusing a multi-device context;
 * on a one-device context each delegates to its one-device form.  What they
 * add: on a multi-device context (rtw_create_devices) every rank takes part,
 * on the tiles the context's split for (W, H, n) gives it (rtw_set_split, a
 * dealt split, or the round robin: the tiles a fixed render renders there).
 * Sums, counts and NaN mask equal the one-device entry point's on the same
 * arguments bit for bit, in both precisions, for any rank count and split
 * (every (pixel, sample) has its own RNG stream).  Stats are summed over the
 * ranks as rtw_get_stats sums them: kernel_ms the slowest rank's, samples the
 * sum of counts (adaptive) or the window's; a rank without a tile contributes
 * none. */
/* rtw_render_adaptive over all ranks.  Ownership is static for the render:
 * each rank runs the passes on its own tiles and compacts its own list, the
 * ranks take each pass in lockstep (every rank's launch, then every rank's
 * wait) with no traffic between them; at the end ONE gather brings a record
 * per tile (its sums and count) to rank 0, which writes the image-order
 * arrays.  The split is read, never dealt, counted or cleared. */
int rtw_render_adaptive_image(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed,
                              uint32_t min_samples, uint32_t max_samples, uint32_t window,
                              double tolerance, double *sums, uint32_t *counts, rtw_stats *stats);
/* rtw_render_adaptive_device over all ranks: d_sums and d_counts are device
 * memory of the context's first device, complete in `stream`'s order (a stream
 * of that device: rank 0 renders on it, the gather and the assembly run on it)
 * when the call returns.  The call synchronises with the host once per pass
 * and rank. */
int rtw_render_adaptive_image_device(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed,
                                     uint32_t min_samples, uint32_t max_samples, uint32_t window,
                                     double tolerance, double *d_sums, size_t sums_bytes,
                                     uint32_t *d_counts, size_t counts_bytes, void *stream);
/* rtw_render_window over all ranks: each rank continues its tiles of `sums` on
 * a packed f64 accumulator of its own (f64 whatever the precision), ONE gather,
 * the f64 assembly on the first device, the download into `sums`.
 * first_sample must be a multiple of every rank's chunk.  Synchronous.  (No
 * device-resident form: it would need a scatter of the sums to the ranks.) */
int rtw_render_window_image(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed,
                            uint32_t first_sample, uint32_t n_samples,
                            double *sums, rtw_stats *stats);
/* ---- per-pixel luminance moments: the variance guide of a denoiser ---------
 * moments is always f64 [H, W, 2] = {S1, S2} in image order, j = 0 the bottom
 * row: with Y = ((0.2126 r) + (0.7152 g)) + (0.0722 b) of each sample's colour
 * (widened exactly when the context is f32), S1 = sum Y and S2 = sum Y * Y in
 * sample order, every operation a separately rounded f64 operation -- the
 * statistic of the adaptive fold above. */
/* rtw_render_window that also keeps the moments: samples [first_sample,
 * first_sample + n_samples) of every pixel, one sample per item, folded in
 * sample order onto sums (H*W*3 doubles, image order; rtw_render_window's
 * additions at chunk 1, bit for bit) and onto moments (H*W*2 doubles).  Both
 * are read when first_sample > 0 and ignored when it is 0, so windows [0, a),
 * [a, b), ... give the call of [0, b) bit for bit, in both precisions.  A
 * window larger than the chunk-sum budget runs in sub-windows internally; the
 * result does not depend on where they fall, nor on tuning tile_cull (a moments
 * window does not cull).  cam->samples_per_pixel and the tuning key "window"
 * are not read.  n_samples == 0 and an image without pixels do nothing.
 * RTW_E_INVALID (nothing launched): a NULL context, camera, sums or moments,
 * first_sample + n_samples beyond 2^32 - 1, an explicit rtw_set_chunk above 1,
 * (device form) a buffer that is too small; RTW_E_UNSUPPORTED on a multi-device
 * or virtual-rank context and for a width or height of 2^16 or more;
 * RTW_E_NO_SCENE.  Stats are the window's, chunk = 1.  The host form is
 * synchronous; the device form takes device memory of the context's device,
 * runs on `stream` and waits for the device only where rtw_render_window_device
 * does. */
int rtw_render_window_moments(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed,
                              uint32_t first_sample, uint32_t n_samples,
                              double *sums, double *moments, rtw_stats *stats);
int rtw_render_window_moments_device(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed,
                                     uint32_t first_sample, uint32_t n_samples,
                                     double *d_sums, size_t sums_bytes,
                                     double *d_moments, size_t moments_bytes, void *stream);
/* The {S1, S2} of the last rtw_render_adaptive / rtw_render_adaptive_device of
 * this one-device context, at that render's image size: per pixel the sums over
 * its first counts[pixel] samples.  RTW_E_INVALID before any adaptive render on
 * the context, after rtw_set_scene, for NULL or (device form) too-small
 * moments; RTW_E_UNSUPPORTED on a multi-device or virtual-rank context.  The
 * host form is synchronous; the device form enqueues one copy kernel on
 * `stream` and never waits (the caller orders it after the adaptive render). */
int rtw_adaptive_moments(rtw_ctx *ctx, double *moments);
int rtw_adaptive_moments_device(rtw_ctx *ctx, double *d_moments, size_t bytes, void *stream);
uint32_t rtw_tile_size(void);                        /* tile edge in pixels (8) */
uint32_t rtw_tiles_for_rank(uint32_t image_width, uint32_t image_height, uint32_t rank,
                            uint32_t nranks);
/* The gathered packed tiles of all ranks -> the image [H][W][3] (sums, j = 0
 * bottom row), on the device: d_ranks holds nranks rank buffers, each
 * rank_stride_bytes apart (>= rank 0's packed size; equal-size buffers as an
 * RCCL gather delivers them).  Follows the context's split for (W, H,
 * nranks) (rtw_set_split; the round robin without one).  Asynchronous on
 * `stream`. */
int rtw_assemble_tiles(rtw_ctx *ctx, const void *d_ranks, size_t rank_stride_bytes, uint32_t nranks,
                       uint32_t image_width, uint32_t image_height, void *d_image, void *stream);

/* ---- cost-balanced rank split (ABI 10) ---------------------------------
 * The round robin (T mod nranks) gives every rank the same NUMBER of tiles
 * but not the same work: a rank's share of glass and mirror tiles varies.
 * The reference balances dynamically -- one rayon task per pixel,
 * work-stealing over every host core (camera.rs:340-353); across GPUs the
 * tiles are dealt once by their costs instead.  A split keeps the round
 * robin's per-rank tile counts (rtw_tiles_for_rank), so packed buffers and the
 * gather stay the same size, and the image does not depend on the split. */
#define RTW_MAX_RANKS 256
/* Deal the tiles of a W x H image (n_tiles = ceil(W/8) * ceil(H/8) entries of
 * tile_cost, any cost unit) to nranks ranks: costliest first (ties: lower
 * tile index), each to the rank of least dealt cost (ties: lower rank) that
 * still has room below its round-robin count.  Writes tile_rank[n_tiles].
 * Deterministic: every process dealing the same costs gets the same split. */
int rtw_split_deal(const uint32_t *tile_cost, uint32_t image_width, uint32_t image_height,
                   uint32_t nranks, uint32_t *tile_rank);
/* Renders (rtw_render_device with this nranks, and the multi-device paths)
 * and rtw_assemble_tiles of a W x H image over nranks ranks follow this split
 * from now on: rank r renders the tiles T with tile_rank[T] == r, packed in
 * increasing T.  tile_rank == NULL restores the round robin.  tile_cost
 * (optional, n_tiles) orders each rank's tasks longest first without a
 * counting render.  RTW_E_INVALID unless every rank r gets exactly
 * rtw_tiles_for_rank(W, H, r, nranks) tiles.  A multi-device context sets it
 * on every rank. */
int rtw_set_split(rtw_ctx *ctx, uint32_t image_width, uint32_t image_height, uint32_t nranks,
                  const uint32_t *tile_rank, const uint32_t *tile_cost);
/* The split renders of (W, H, nranks) follow: 0 = the round robin (tile_rank
 * untouched), 1 = set by rtw_set_split, 2 = dealt by the context itself
 * (tuning "balance"); for 1 and 2 tile_rank (may be NULL) receives it. */
int rtw_get_split(rtw_ctx *ctx, uint32_t image_width, uint32_t image_height, uint32_t nranks,
                  uint32_t *tile_rank);
/* The tile costs the context counted in its first render of (cam, rank,
 * nranks) under its current split (tuning "lpt", spp >= "lpt_min_spp": BVH
 * node visits + sphere tests + 12 per segment of each pixel's first
 * "lpt_pilot_spp" samples, summed per tile), written to tile_cost[T] for the
 * rank's tiles T (other entries untouched: the ranks' arrays summed give the
 * whole image's).  Waits for that render.  RTW_E_INVALID when there is no
 * such count.  With tuning "balance" (1, the default) a multi-device
 * context deals its split from these costs by itself: the first
 * rtw_render_image_device of a camera counts, the second deals and renders
 * balanced (re-dealt when the scene or camera changes).  A provably empty
 * tile (rtw_culled_tiles) is never traced and gets no task: it is reported
 * with the smallest cost, 1 (the fold answers it; 0 stays "not counted"),
 * which rtw_split_deal deals like any other cost. */
int rtw_tile_costs(rtw_ctx *ctx, const rtw_camera *cam, uint32_t rank, uint32_t nranks, uint32_t *tile_cost);
/* Provably empty tiles (RTW_F64, scenes of spheres and planes only; tuning
 * "tile_cull", default 1, 0 = off): a tile whose every camera ray -- every
 * lens point, every pixel offset -- misses every primitive by a margin that
 * dominates the rounding of the reference's tests is not traced.  Every
 * sample of it is the background, and the fold adds that constant in the
 * reference's order, so the image is the same bit for bit; stats.samples and
 * stats.segments count its samples (one segment each).  Nothing is culled in
 * RTW_F32, in adaptive renders, for scenes with quads, cuboids, textures or
 * emitters, or when a scene or camera value is not finite or beyond 2^130.
 * Returns the number of such tiles in the last render (summed over the ranks
 * of a multi-device render); 0 for a NULL context. */
uint32_t rtw_culled_tiles(rtw_ctx *ctx);
/* Counters of the last render (waits for it to finish).  Returns
 * RTW_E_NO_LIGHTS / RTW_E_PANIC (stats still filled) when a sample reached a
 * reference panic, RTW_E_INVALID before the first render.  A multi-device
 * context sums the ranks that took part in its last render (all of them after
 * rtw_render / rtw_render_image_device; rank 0 after rtw_render_device). */
int rtw_get_stats(rtw_ctx *ctx, rtw_stats *stats);
/* Rank k's own counters of its last render (k = 0 included: rtw_get_stats on
 * rtw_device_ctx(ctx, 0) == ctx sums the ranks), ABI 9. */
int rtw_get_stats_rank(rtw_ctx *ctx, uint32_t k, rtw_stats *stats);
/* Device times (HIP events) of the last min(max, 64) renders, oldest first:
 * render_ms = the render kernel alone, total_ms = render + chunk reduction.
 * Waits for them; returns how many were written. */
int rtw_get_timings(rtw_ctx *ctx, float *render_ms, float *total_ms, int max);
/* The render-kernel variant of the last render: (kernel << 8) | options, with
 * kernel as rtw_stats.kernel and options the compile-time option bits of the
 * launched instantiation (1 closest-approach f32 tests, 2 light BVH / grid,
 * 4 textures, 8 quads / cuboids / mixed light lists, 16 f64 hit points);
 * 0 when no render kernel has run.  Measurement tooling uses it to name the
 * exact machine code that ran (render_kernel<R, kernel, options>). */
int rtw_last_kernel(const rtw_ctx *ctx);

/* ---- batched ray queries: Hittable::hit and the light list's pdf_value ---
 * The reference's other public surface, the Hittable trait (shared/src/
 * hittable.rs:172-182), against the scene staged by rtw_set_scene:
 *   closest hit   world.hit(&r, t_min..=INFINITY) of the HittableList /
 *                 BoundedVolumeHierarchy (hittable_collections/bvh.rs:164-188)
 *                 for n rays, each answered with a HitRecord::new
 *                 (hittable.rs:100-129);
 *   light pdf     HittableList::pdf_value(origin, direction) of the light list
 *                 (hittable_list.rs:408-412), the RTW_LIGHTS_BVH_LEAF form
 *                 included, NaN where the reference gives NaN (an origin
 *                 inside a light sphere; an empty list's 0 / 0).
 * A query runs the traversal a render of the scene would run under the same
 * tuning keys (accel, bvh_kind, lds, bvh_lds_max, robust, light_grid,
 * light_bvh_min), through the same device code.  RTW_F64: bit-identical to
 * the reference's f64 arithmetic.  RTW_F32: the plain f32 arithmetic of the
 * speed mode -- the render's f64 hit-point refinement (tuning hit64) is not
 * part of a query.  Queries keep their own buffers and counters: a render
 * before and after one is unchanged.
 *
 *   rays: n x 6 {ox, oy, oz, dx, dy, dz} in the context's precision (float
 *         or double); the direction need not be normalised
 *   hits: n x 9 {t, p xyz, normal xyz (against the ray: front-face adjusted),
 *         u, v}, same precision
 *   ids : n x 4 int32 {object id, material id, front face 0 / 1, RTW_PRIM_*}.
 *         Object ids count planes, then quads, cuboids, spheres, each in scene
 *         order (the ids of rtw_stats and the oracle).
 *   A miss: object id -1, every other field of both rows 0.
 * Equal t goes to the lowest object id.  A cuboid hit reports what the render
 * uses (entities/transformations.rs:14-29): the world-space point with the
 * object-space normal, front face and UV.
 * t_min: one scalar per call, finite and >= 0 (the reference passes
 * f64::EPSILON from the integrator, 0 from pdf_value); the upper end of the
 * closest-hit query is always +inf, the only one the reference's integrator
 * passes -- a ranged any-hit is rtw_occluded_rays below.
 *
 * Errors: RTW_E_INVALID for a NULL context, a NULL array with n > 0, a buffer
 * that is too small, a negative / NaN / infinite t_min; RTW_E_NO_SCENE before
 * rtw_set_scene; RTW_E_UNSUPPORTED on a multi-device or virtual-rank context
 * (a query has no tiles to split).  n = 0 is RTW_OK and launches nothing.
 * The host forms are synchronous; the device forms enqueue on the caller's
 * stream as rtw_render_device does (NULL: the context's own). */
#define RTW_PRIM_PLANE 0
#define RTW_PRIM_QUAD 1
#define RTW_PRIM_CUBOID 2
#define RTW_PRIM_SPHERE 3
int rtw_hit_rays(rtw_ctx *ctx, const void *rays, uint64_t n, double t_min, void *hits, int32_t *ids);
int rtw_hit_rays_device(rtw_ctx *ctx, const void *d_rays, uint64_t n, double t_min, void *d_hits,
                        size_t hits_bytes, int32_t *d_ids, size_t ids_bytes, void *stream);
/* pdf: n values of the context's precision */
int rtw_light_pdf_rays(rtw_ctx *ctx, const void *rays, uint64_t n, void *pdf);
int rtw_light_pdf_rays_device(rtw_ctx *ctx, const void *d_rays, uint64_t n, void *d_pdf, size_t pdf_bytes,
                              void *stream);
typedef struct rtw_query_stats {
    uint64_t rays;                /* rays of the last query */
    uint64_t hits;                /* ... that hit something (closest hit) */
    uint64_t node_visits;         /* BVH inner nodes entered */
    uint64_t sphere_tests;        /* ray-sphere tests (the brute-force sweep: rays x spheres) */
    uint64_t light_tests;         /* (ray, light) pairs the light pdf tested */
    uint32_t kernel;              /* closest hit: the world that ran, as rtw_stats.kernel;
                                     light pdf: 0 linear list, 1 light BVH, 2 light grid,
                                     3 mixed list (quads / default entries) */
    uint32_t is_light_pdf;        /* the last query: 0 closest hit (or a feature pass), 1 light
                                     pdf, 2 any hit (rtw_occluded_rays: `hits` counts the
                                     occluded rays, `kernel` is the world), 3 light sample
                                     (rtw_light_sample: `kernel` is the light path,
                                     light_tests those of the fused pdf), 4 camera rays
                                     (rtw_camera_rays), 5 the bounce (rtw_shade_rays: `hits`
                                     counts the rays that continue, `kernel` is the light path),
                                     6 one path advance (rtw_path_advance: rays = n, `hits`
                                     counts the survivors), 7 the wavefront driver
                                     (rtw_render_wavefront: rays = the sum of the rounds' n --
                                     a render's `segments` --, `hits` = the SCATTER events -- its
                                     `lambertian` --, kernel_ms = the device time of the whole
                                     call); `kernel` is 0 for both; 8 direct lighting
                                     (rtw_direct_light: rays = the (point, sample) pairs traced,
                                     `hits` = the pairs that added a term, light_tests those
                                     of the fused pdf, `kernel` is the world), 9 ambient occlusion
                                     (rtw_ambient_occlusion: rays = the (point, sample) pairs
                                     traced, `hits` = the occluded pairs, `kernel` is the
                                     world), 10 radiance (rtw_radiance_rays: rays = the
                                     segments traced, `hits` = the SCATTER events, light_tests
                                     those of the bounces' pdfs, `kernel` is the world) */
    double kernel_ms;             /* device time of the query kernel (HIP events) */
} rtw_query_stats;
/* Counters of the last query (waits for it); RTW_E_INVALID before the first. */
int rtw_get_query_stats(rtw_ctx *ctx, rtw_query_stats *stats);

/* ---- any-hit occlusion and light sampling: what an outside integrator needs -
 * With the light pdf above these answer the Hittable trait completely (hit
 * with a range, pdf_value, random): per shading point a direction towards a
 * light, its pdf, and a shadow ray.  Both run on the plan of the queries above
 * (the same world, test form, stack, LDS and light path under the same tuning
 * keys), through the same device functions, on the queries' own buffers.
 *
 * rtw_occluded_rays: world.hit(&r, t_min..=t_max[i]).is_some() for n rays
 * (hittable_list.rs:395-406, bvh.rs:164-188) -- the reference's semantics, not
 * a closest hit with a smaller bound:
 *   - a candidate is accepted when t_min <= t && t <= t_max, inclusive at both
 *     ends (RangeInclusive); per primitive, t is the closest-hit query's t bit
 *     for bit in each precision;
 *   - a sphere whose near root is outside the range is tried at its far root
 *     (sphere.rs:72-80);
 *   - the range is not shrunk from object to object (hittable_list.rs:399-405);
 *   - the AABB gates of planes, quads and cuboids (bounded_hit, hittable.rs:
 *     39-86) test max(t_min, tn) <= min(t_max, tf): a finite t_max is part of
 *     the gate.  Spheres are tested without a gate of their own: as in the
 *     closest-hit query, neither the sweep nor the BVH leaves model a sphere's
 *     unpadded box (the sphere's own root test decides).
 * The traversal stops at the first accepted hit: a ray blocked by a plane, quad
 * or cuboid never enters the sphere traversal, and an accepted sphere culls
 * every box still on the ray's stack.
 *   rays    : n x 6, as rtw_hit_rays
 *   t_max   : n values of the context's precision, or NULL for +inf.  +inf is
 *             allowed; t_max[i] NaN or < t_min answers 0.  A NaN ray answers 0.
 *   occluded: n bytes, 0 or 1
 * t_min and the errors are rtw_hit_rays'.  Query stats: is_light_pdf = 2, hits =
 * the occluded rays, kernel = the world that ran.
 *
 * rtw_light_sample: lights.random(origin, rng) (hittable_list.rs:414-419) for n
 * points and, when pdf is not NULL, lights.pdf_value(origin, direction drawn).
 * The stream convention for points that belong to no pixel: point k draws from
 * the stream a render gives to (seed, pixel index first_stream + k, sample
 * index `sample`) -- the keying of the render's RNG (splitmix64 over seed,
 * pixel + 1, sample + 1 into xoshiro256++), with a 64-bit pixel index -- and
 * makes from its start exactly the draws the render's Lambertian branch makes
 * for lights.random: one gen_range(0..len) for the entry, then the entry's
 * random() (Sphere::random sphere.rs:114-127, Quad::random quadrilateral.rs:
 * 114-118, the (1, 0, 0) default of hittable.rs).  Calls compose: (first_stream
 * = a, n) followed by (a + n, m) equals one call of n + m points.
 *   origins   : n x 3 in the context's precision
 *   directions: n x 3 as the reference returns them: unnormalised; for a quad
 *               p - origin, so a shadow ray along one has t_max just under 1;
 *               an origin inside a sphere light gives the reference's NaN
 *   pdf       : n values or NULL; rtw_light_pdf_rays of {origin, direction} bit
 *               for bit (the same light path: linear, light BVH, grid, mixed;
 *               the RTW_LIGHTS_BVH_LEAF form included)
 *   light     : n list indices (the entry drawn), or NULL
 * An empty light list is RTW_E_INVALID (the reference panics, hittable_list.rs:
 * 417); the other errors are the queries'.  Query stats: is_light_pdf = 3,
 * kernel = the light path, light_tests those of the fused pdf. */
int rtw_occluded_rays(rtw_ctx *ctx, const void *rays, uint64_t n, double t_min, const void *t_max,
                      uint8_t *occluded);
int rtw_occluded_rays_device(rtw_ctx *ctx, const void *d_rays, uint64_t n, double t_min, const void *d_t_max,
                             size_t t_max_bytes, uint8_t *d_occluded, size_t occluded_bytes, void *stream);
int rtw_light_sample(rtw_ctx *ctx, const void *origins, uint64_t n, uint64_t seed, uint64_t first_stream,
                     uint32_t sample, void *directions, void *pdf, int32_t *light);
int rtw_light_sample_device(rtw_ctx *ctx, const void *d_origins, uint64_t n, uint64_t seed, uint64_t first_stream,
                            uint32_t sample, void *d_directions, size_t directions_bytes, void *d_pdf,
                            size_t pdf_bytes, int32_t *d_light, size_t light_bytes, void *stream);

/* ---- direct lighting as one query ------------------------------------------
 * rtw_direct_light: for n shading points {p, normal} and S = n_samples light
 * samples each, the light half of the reference's Lambertian bounce followed by
 * the next segment's emission (camera.rs:480-521), folded per point.  It fuses
 * what the queries above answer one by one -- rtw_light_sample, rtw_hit_rays,
 * the `emitted` of rtw_shade_rays -- through the same device functions, on the
 * same plan (world, test form, stacks, LDS, light path), so every field below
 * is those queries' bit for bit in each precision.
 *
 * The estimator is the light list's lobe alone: direction and pdf are
 * lights.random / lights.pdf_value, not the reference's MixturePdf with the
 * cosine lobe.  An emitter that is not in the light list counts only where a
 * listed light's direction passes it.  The caller multiplies the sums by the
 * surface's albedo (the feature pass's) and divides by the samples taken.
 *
 * The law, per point k, over s = first_sample .. first_sample + S - 1 in that
 * order:
 *   1. the stream Rng(seed, first_stream + k, s) -- rtw_light_sample's keying,
 *      with `sample` = s; from its start, d and the list index are exactly
 *      rtw_light_sample's (hittable_list.rs:414-419);
 *   2. pdf = lights.pdf_value(p, d): rtw_light_pdf_rays of {p, d} bit for bit,
 *      through whichever light path the plan picks (linear, light BVH, grid,
 *      mixed; the RTW_LIGHTS_BVH_LEAF form included);
 *   3. the closest hit of {p, d} over t_min..=inf: rtw_hit_rays' record (t, object
 *      id, material id, u, v, the hit point);
 *   4. Le = Material::emitted(u, v, hit point) of that material: rtw_shade_rays'
 *      `emitted` -- DiffuseLight's texture, black for every other material and
 *      for a miss;
 *   5. spdf = max(dot(normal, normalize(d)) / PI, 0) (material.rs:372-375);
 *   6. a term is added only when there is a hit, pdf > 0 and spdf > 0 (the
 *      comparisons are false for NaN);
 *   7. term_c = (Le_c * spdf) / pdf, in the context's precision;
 *   8. direct[k][c] += (double)term_c: one f64 add, never contracted;
 *   9. when no term is added, no add is made and the record's term is 0.
 * A point whose normal is exactly (0, 0, 0) -- a miss row of rtw_hit_rays -- is
 * skipped entirely: no draws, no traversal, its sums untouched, its records 0
 * with object id -1.
 *   points    : n x 6 {p xyz, normal xyz} in the context's precision: fields 1..6
 *               of a rtw_hit_rays record
 *   direct    : n x 3 f64 sums in both precisions (as the feature pass folds);
 *               overwritten, or continued from its content when accumulate != 0,
 *               so windows over first_sample compose bit for bit
 *   samples   : optional (NULL), n * S x 12 in the context's precision, row
 *               k * S + (s - first_sample): {d xyz, pdf, t (0 for a miss), spdf,
 *               Le rgb, term rgb}
 *   sample_ids: optional (NULL), n * S x 4 int32: {light-list index drawn, object
 *               id hit or -1, material id, 1 if the sample added a term}
 * Calls compose over first_stream as rtw_light_sample's do.  Device form: each
 * d_ pointer is followed by its size in bytes; d_points must be 16-byte aligned
 * in f64 and 8-byte in f32, d_direct 8-byte, d_samples and d_sample_ids 16-byte.
 * Errors: RTW_E_INVALID for a NULL context, NULL points or direct with n > 0,
 * short or misaligned device buffers, a t_min that is not finite and >= 0,
 * n_samples == 0, an empty light list (the reference panics, hittable_list.rs:
 * 417), or n * S over 2^32 when records are asked for; RTW_E_NO_SCENE before
 * rtw_set_scene; RTW_E_UNSUPPORTED on multi-device and virtual contexts.  n = 0
 * launches nothing.  Query stats: is_light_pdf = 8, rays = the (point, sample)
 * pairs traced, hits = the pairs that added a term, light_tests those of the
 * fused pdf, kernel = the world that ran, node_visits and sphere_tests as in
 * the closest hit. */
int rtw_direct_light(rtw_ctx *ctx, const void *points, uint64_t n, uint64_t seed, uint64_t first_stream,
                     uint32_t first_sample, uint32_t n_samples, double t_min, int accumulate, double *direct,
                     void *samples, int32_t *sample_ids);
int rtw_direct_light_device(rtw_ctx *ctx, const void *d_points, size_t points_bytes, uint64_t n, uint64_t seed,
                            uint64_t first_stream, uint32_t first_sample, uint32_t n_samples, double t_min,
                            int accumulate, double *d_direct, size_t direct_bytes, void *d_samples,
                            size_t samples_bytes, int32_t *d_sample_ids, size_t sample_ids_bytes, void *stream);

/* ---- ambient occlusion as one query ----------------------------------------
 * rtw_ambient_occlusion: for n shading points {p, normal} and S = n_samples
 * samples each, how much of the cosine-weighted hemisphere above the point is
 * open: the number of samples whose direction meets nothing.  With the
 * reference's CosinePdf a sky sample's term is background * spdf / pdf =
 * background, so the sky's share of a point's direct light is background *
 * open / S -- the lobe rtw_direct_light (the light list's lobe alone) leaves
 * out.  It fuses CosinePdf::generate and rtw_occluded_rays through the same
 * device functions, on the same plan (world, test form, stack, LDS).  The
 * answer is an integer count: exact in both precisions, and independent of the
 * order the samples are taken in.
 *
 * The law, per point k, over s = first_sample .. first_sample + S - 1:
 *   1. the stream Rng(seed, first_stream + k, s) -- rtw_light_sample's keying,
 *      with `sample` = s; from its start, exactly the two draws of
 *      CosinePdf::new(normal).generate(rng) (pdf.rs:38-52, onb.rs:8-35,
 *      utils.rs:146-161): r1, r2 = two Standard f64 (in f32: their f32 form);
 *   2. x = (cos(2 PI r1) sqrt(r2), sin(2 PI r1) sqrt(r2), sqrt(1 - r2));
 *      Onb(normal): w = normalize(normal), a = |w.x| > 0.9 ? (0, 1, 0) : (1, 0, 0),
 *      v = normalize(cross(w, a)), u = cross(w, v);
 *      d = ((0 + u * x.x) + v * x.y) + w * x.z, the fold from zero of
 *      Onb::transform.  In f64 this is the reference bit for bit; in f32 it is
 *      the render's f32 form of the same operations.  d is not renormalised, so
 *      t counts in units of |d|, which is 1 within rounding;
 *   3. occ = world.hit(&{p, d}, t_min..=t_max).is_some(): rtw_occluded_rays of
 *      {p, d} with that t_max bit for bit -- inclusive at both ends, a sphere's
 *      far root when its near root is below t_min, the AABB gates of planes,
 *      quads and cuboids over the range.  A NaN ray (a NaN normal or point)
 *      answers 0.  t_max is one double for the call, rounded to the context's
 *      precision; +inf is allowed; a t_max that is NaN or < t_min answers 0 for
 *      every sample;
 *   4. open[k] += !occ.
 * A point whose normal is exactly (0, 0, 0) -- a miss row of rtw_hit_rays -- is
 * skipped entirely: no draws, no traversal, its count 0 (untouched when
 * accumulate != 0), its record rows 0.
 *   points    : n x 6 {p xyz, normal xyz} in the context's precision: fields 1..6
 *               of a rtw_hit_rays record
 *   open      : n x uint32; overwritten, or continued from its content when
 *               accumulate != 0, so windows over first_sample compose exactly
 *   directions: optional (NULL), n * S x 3 in the context's precision, row
 *               k * S + (s - first_sample): d
 *   occluded  : optional (NULL), n * S bytes, the same rows: occ
 * Calls compose over first_stream as rtw_light_sample's do.  Device form: each
 * d_ pointer is followed by its size in bytes; d_points must be 16-byte aligned
 * in f64 and 8-byte in f32, d_open 4-byte, d_directions 8-byte in f64 and 4-byte
 * in f32; d_open is zeroed (unless accumulate) and added to on `stream`.
 * Errors, checked in this order: RTW_E_INVALID for a NULL context;
 * RTW_E_UNSUPPORTED on multi-device and virtual contexts; RTW_E_NO_SCENE before
 * rtw_set_scene; RTW_E_INVALID for NULL points or open with n > 0, a t_min that
 * is not finite and >= 0, n_samples == 0, n over 2^40, n * S over 2^62, n * S
 * over 2^32 when a record is asked for, short or misaligned device buffers.  An
 * empty light list is fine.  n = 0 launches nothing.  Query stats: is_light_pdf
 * = 9, rays = the (point, sample) pairs traced, hits = the occluded pairs,
 * kernel = the world that ran, node_visits and sphere_tests as in the any hit. */
int rtw_ambient_occlusion(rtw_ctx *ctx, const void *points, uint64_t n, uint64_t seed, uint64_t first_stream,
                          uint32_t first_sample, uint32_t n_samples, double t_min, double t_max, int accumulate,
                          uint32_t *open, void *directions, uint8_t *occluded);
int rtw_ambient_occlusion_device(rtw_ctx *ctx, const void *d_points, size_t points_bytes, uint64_t n, uint64_t seed,
                                 uint64_t first_stream, uint32_t first_sample, uint32_t n_samples, double t_min,
                                 double t_max, int accumulate, uint32_t *d_open, size_t open_bytes,
                                 void *d_directions, size_t directions_bytes, uint8_t *d_occluded,
                                 size_t occluded_bytes, void *stream);

/* ---- radiance along arbitrary rays as one query -----------------------------
 * rtw_radiance_rays: for n rays {origin, direction} and S = n_samples samples
 * each, the full incoming radiance: Camera::ray_colour_tail_call
 * (camera.rs:460-522) run to the end of every path, the sample colours summed
 * in f64.  It fuses the loop of rtw_hit_rays, rtw_shade_rays and
 * rtw_path_advance into one kernel through the same device functions, on the
 * same plan (world, test form, stacks, LDS, light path, tuning keys): no record
 * of a round leaves the registers.  With rtw_direct_light (the light list's
 * lobe) and rtw_ambient_occlusion (the sky's) this is the third fused
 * estimator: everything.
 *
 * The law, per ray k, over s = first_sample .. first_sample + S - 1 in that
 * order:
 *   1. the stream.  rng == NULL: Rng(seed, first_stream + k, s) from its start
 *      -- rtw_light_sample's keying, with `sample` = s.  rng != NULL: n x 4
 *      uint64 start states and n_samples must be 1; rng[k] is read (four zero
 *      words are no xoshiro256++ state: as in rtw_shade_rays the stream of (0,
 *      0, 0) stands in from the path's first hit on, and a path that never hits
 *      leaves them as they are) and written back after the path.  So
 *      rtw_camera_rays followed by rtw_radiance_rays(rng) is one sample of
 *      Camera::render;
 *   2. the path.  mult = (1, 1, 1), res = 0, r = rays[k]; up to max_depth
 *      rounds of: the record of rtw_hit_rays(r, t_min = f64::EPSILON); next,
 *      weight, emitted and event of rtw_shade_rays on that record, the stream
 *      advanced by exactly its draws; then rtw_path_advance's bookkeeping, every
 *      product rounded before its add:
 *        MISS      colour = mult * background + res, the path ends
 *        ABSORBED  colour = mult * emitted + res, the path ends
 *        SCATTER   res += mult * emitted; mult *= weight; r = next
 *        REFLECT   mult *= weight; r = next
 *      a path alive after max_depth rounds ends with colour = 0 + res; with
 *      max_depth == 0 every colour is 0 + 0 and nothing is traced.  background
 *      is three doubles, rounded to the context's precision.  Every field is
 *      those queries' bit for bit in each precision (f32: the plain f32
 *      arithmetic of the f32 queries);
 *   3. the fold.  radiance[k][c] += (double)colour_c: one f64 add per sample, in
 *      sample order, never contracted.  NaN is not scrubbed (the tail-call form
 *      never calls fix_nan).
 *   rays     : n x 6 {origin xyz, direction xyz} in the context's precision, as
 *              for rtw_hit_rays
 *   radiance : n x 3 f64 in both precisions; overwritten, or continued from its
 *              content when accumulate != 0, so windows over first_sample compose
 *              exactly
 *   colours  : optional (NULL), n * S x 3 in the context's precision, row
 *              k * S + (s - first_sample): the sample's colour
 *   segments : optional (NULL), n * S uint32, the same rows: the world.hit calls
 *              of the pair
 * Calls compose over first_stream as rtw_light_sample's do.  Device form: each
 * d_ pointer is followed by its size in bytes; d_rays must be 16-byte aligned in
 * f64 and 8-byte in f32, d_radiance 8-byte, d_rng 16-byte, d_colours 8-byte in
 * f64 and 4-byte in f32, d_segments 4-byte; `stream` as for
 * rtw_direct_light_device.
 * Errors, checked in this order before any device call: RTW_E_INVALID for a NULL
 * context; RTW_E_UNSUPPORTED on multi-device and virtual contexts;
 * RTW_E_NO_SCENE before rtw_set_scene; RTW_E_NO_LIGHTS where rtw_shade_rays
 * gives it (an empty light list and a Lambertian material); RTW_E_INVALID for
 * NULL rays, radiance or background with n > 0, n_samples == 0, rng with
 * n_samples != 1, first_sample + n_samples over 2^32, n over 2^40, n * S over
 * 2^62, n * S over 2^32 when a record is asked for, short or misaligned device
 * buffers.  n = 0 launches nothing.  Query stats: is_light_pdf = 10, rays = the
 * segments traced, hits = the SCATTER events, kernel = the world that ran,
 * light_tests, node_visits and sphere_tests as in the closest hit and the
 * bounce. */
int rtw_radiance_rays(rtw_ctx *ctx, const void *rays, uint64_t n, uint64_t seed, uint64_t first_stream,
                      uint32_t first_sample, uint32_t n_samples, uint32_t max_depth, const double background[3],
                      uint64_t *rng, int accumulate, double *radiance, void *colours, uint32_t *segments);
int rtw_radiance_rays_device(rtw_ctx *ctx, const void *d_rays, size_t rays_bytes, uint64_t n, uint64_t seed,
                             uint64_t first_stream, uint32_t first_sample, uint32_t n_samples, uint32_t max_depth,
                             const double background[3], uint64_t *d_rng, size_t rng_bytes, int accumulate,
                             double *d_radiance, size_t radiance_bytes, void *d_colours, size_t colours_bytes,
                             uint32_t *d_segments, size_t segments_bytes, void *stream);

/* ---- path queries: camera rays and the material bounce ---------------------
 * The Material trait (shared/src/material.rs:32-49) and Camera::get_ray as
 * batched queries, linked by the RNG state they return.  With rtw_hit_rays
 * between them a caller's loop is a wavefront path tracer:
 *     rays, rng = camera_rays(sample s)        mult = 1, res = 0
 *     repeat max_depth times:  hits, ids = hit_rays(rays, t_min = f64::EPSILON)
 *                              next, weight, emitted, event = shade_rays(...)
 *     MISS     colour = mult * background + res                (camera.rs:473-475)
 *     ABSORBED colour = mult * emitted + res                   (camera.rs:484-486)
 *     REFLECT  mult *= weight                                  (camera.rs:488-500)
 *     SCATTER  res += mult * emitted, then mult *= weight      (camera.rs:504-521)
 *     paths still alive after max_depth rounds: colour = 0 + res (camera.rs:470-472)
 * In RTW_F64 the image of that loop is bit for bit Camera::render's.
 *
 * rtw_camera_rays: Camera::get_ray (camera.rs:274-293) for n pixels and one
 * sample index.  Ray k belongs to pixel index pixels[k], or first_pixel + k
 * when pixels is NULL; the index is j * image_width + i, the render's stream
 * key (j = 0 is the bottom row).  The stream is the one a render gives to
 * (seed, that pixel, sample): splitmix64 over seed, pixel + 1, sample + 1 into
 * xoshiro256++.  From its start the call makes exactly get_ray's draws:
 *   1. Uniform::new_inclusive(-0.5, 0.5) for the x offset (camera.rs:275-276),
 *   2. Uniform::new_inclusive(-0.5, 0.5) for the y offset (camera.rs:276),
 *   3. only when defocus_angle > f64::EPSILON: the UnitDisk rejection loop
 *      (utils.rs:124-144), two Standard draws per try (camera.rs:285-290).
 *   rays: n x 6 {origin, direction = pixel sample - origin} in the context's
 *         precision, the direction unnormalised
 *   rng : n x 4 uint64, the xoshiro256++ words s0..s3 after those draws
 * cam->samples_per_pixel and max_depth are not read.  No scene needs to be
 * staged.  An index >= image_width * image_height is RTW_E_INVALID: the host
 * form checks every index; for the device form an out-of-range entry of
 * d_pixels is the caller's error -- it is clamped to the last pixel, so nothing
 * is read or written out of bounds.  Query stats: is_light_pdf = 4.
 *
 * rtw_shade_rays: one iteration of ray_colour_tail_call after world.hit
 * (camera.rs:480-521) for n rays.  rays are the incoming rays, hits and ids
 * exactly what rtw_hit_rays wrote for them.  The kernel reads no world
 * geometry: the record, the material and texture tables and the light list.
 *   event  : n int32
 *     RTW_EVENT_MISS      object id < 0.  Every output row is 0 and the ray's
 *                         rng is left untouched.
 *     RTW_EVENT_ABSORBED  scatter() is None: DiffuseLight (material.rs:490-514),
 *                         Invisible (material.rs:321-325), a Metal direction with
 *                         !(dot(direction, normal) > 0) (material.rs:416).
 *                         next, weight and pdfs are 0.
 *     RTW_EVENT_REFLECT   Metal or Dialectric (ScatterRecord::Reflect).
 *     RTW_EVENT_SCATTER   Lambertian (ScatterRecord::Scatter).
 *   emitted: n x 3, Material::emitted(u, v, p) with the texture evaluated at
 *            the record's (u, v, p) (material.rs:508-514; black otherwise,
 *            material.rs:42-44)
 *   weight : n x 3: Metal's albedo; (1, 1, 1) for Dialectric; for Lambertian
 *            (attenuation * scattering_pdf) / pdf_value in that association
 *            (camera.rs:518)
 *   next   : n x 6 {p, direction}, the direction as the reference returns it,
 *            unnormalised
 *   pdfs   : n x 3 or NULL: {MixturePdf value (pdf.rs:90-92), the light list's
 *            pdf_value (hittable_list.rs:408-412; the RTW_LIGHTS_BVH_LEAF form
 *            bvh.rs:67-76), scattering_pdf (material.rs:372-375)}; 0 unless the
 *            event is SCATTER.  The light list's value is rtw_light_pdf_rays of
 *            {p, direction} bit for bit: the same light path (linear, light BVH,
 *            grid, mixed) under the same tuning keys, through the same code.
 *   rng    : n x 4 uint64, required; read, advanced by exactly the draws of
 *            the reference's branch and written back:
 *     Metal       the UnitSphere rejection loop (utils.rs:99-122), three
 *                 Standard draws per try (material.rs:415); RTW_F32 draws three
 *                 words in all (the speed mode's direct sampler)
 *     Dialectric  one Open01, only when refraction is possible
 *                 (material.rs:474-476: not drawn on total internal reflection)
 *     Lambertian  one Standard for the lobe (pdf.rs:95); below 0.5
 *                 gen_range(0..len) and the entry's random()
 *                 (hittable_list.rs:414-419: Sphere two Standard, Quad two
 *                 Open01, the Hittable default none), else the cosine
 *                 hemisphere's two Standard (utils.rs:146-161)
 *     DiffuseLight, Invisible   nothing
 *            Four zero words are no xoshiro256++ state (no seeding produces them;
 *            every draw would be 0 and a rejection loop would never end): such a
 *            row draws from the stream of (seed 0, pixel 0, sample 0) instead.
 * A row whose material id is not one of the scene's is answered as a MISS.
 * RTW_F64: every output bit is the reference's.  RTW_F32: the plain f32
 * arithmetic of the speed mode; a loop of plain-f32 queries is not the hit64
 * render (whose hit points are refined in f64) and is outside the f32
 * tolerance of the renders.
 * Errors are the queries': RTW_E_INVALID for a NULL context, a NULL array with
 * n > 0 (pdfs excepted) or a buffer that is too small or, in the device forms,
 * not aligned for its records -- the largest power of two that divides the
 * record's size, 16 at the most: rays and next 16 bytes in RTW_F64 and 8 in
 * RTW_F32, hits / weight / emitted / pdfs 8 and 4, ids and rng 16, event 4 (so
 * a row slice of any of them is as good as the whole array); RTW_E_NO_SCENE before rtw_set_scene (rtw_shade_rays);
 * RTW_E_UNSUPPORTED on a multi-device or virtual-rank context; n = 0 launches
 * nothing.  The one difference from the render: an empty light list in a scene
 * that holds a Lambertian material is refused with RTW_E_NO_LIGHTS before the
 * launch (the reference panics, hittable_list.rs:417; the render carries a NaN
 * on).  Query stats: is_light_pdf = 5, hits = the rays that continue (REFLECT +
 * SCATTER), light_tests those of the fused light pdf, kernel = the light path. */
#define RTW_EVENT_MISS 0
#define RTW_EVENT_ABSORBED 1
#define RTW_EVENT_REFLECT 2
#define RTW_EVENT_SCATTER 3
int rtw_camera_rays(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed, uint32_t sample, const uint32_t *pixels,
                    uint64_t first_pixel, uint64_t n, void *rays, uint64_t *rng);
int rtw_camera_rays_device(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed, uint32_t sample,
                           const uint32_t *d_pixels, size_t pixels_bytes, uint64_t first_pixel, uint64_t n,
                           void *d_rays, size_t rays_bytes, uint64_t *d_rng, size_t rng_bytes, void *stream);
int rtw_shade_rays(rtw_ctx *ctx, const void *rays, const void *hits, const int32_t *ids, uint64_t n, uint64_t *rng,
                   void *next, void *weight, void *emitted, int32_t *event, void *pdfs);
int rtw_shade_rays_device(rtw_ctx *ctx, const void *d_rays, size_t rays_bytes, const void *d_hits, size_t hits_bytes,
                          const int32_t *d_ids, size_t ids_bytes, uint64_t n, uint64_t *d_rng, size_t rng_bytes,
                          void *d_next, size_t next_bytes, void *d_weight, size_t weight_bytes, void *d_emitted,
                          size_t emitted_bytes, int32_t *d_event, size_t event_bytes, void *d_pdfs, size_t pdfs_bytes,
                          void *stream);

/* ---- wavefront path rounds on the device: begin, advance, the batched driver ----
 * The loop above, kept on the GPU.  A PATH STATE is five arrays of the paths
 * still alive, row k one path: rays n x 6, rng n x 4 uint64, mult n x 3 (the
 * product of the weights so far), res n x 3 (the emission gathered so far) and
 * slot n uint32 -- where the path's colour goes when it ends: colour[slot], an
 * array of colour_slots x 3 values.  The slot travels with the path; a path's
 * result does not depend on its row.  All values are the context's precision.
 *
 * rtw_path_begin_device: for k < n, mult = 1, res = 0, slot = first_slot + k.
 * first_slot + n > 2^32 is RTW_E_INVALID.  No scene needs to be staged.
 *
 * rtw_path_advance: one round's bookkeeping.  In: n, the state's mult / res /
 * slot the round started from, and the round's event / weight / emitted / next /
 * rng exactly as rtw_shade_rays wrote them for the state's rays (rng: the one
 * it advanced in place).  Per path, each component in the context's precision,
 * every product rounded before the add (no fused multiply-add):
 *     MISS      colour[slot] = mult * background + res          (camera.rs:473-475)
 *     ABSORBED  colour[slot] = mult * emitted + res             (camera.rs:484-486)
 *     SCATTER   res' = res + mult * emitted, mult' = mult * weight, survives
 *     REFLECT   mult' = mult * weight, res' = res, survives     (camera.rs:488-521)
 *     any other event value ends the path as a MISS with a black background
 * A survivor is appended to the OUT-STATE as {rays = next, rng, mult', res',
 * slot}; with `last` set (the round at max_depth - 1) it is not appended but
 * ends with colour[slot] = 0 + res' (camera.rs:470-472).  The number of
 * survivors is returned: the host form writes it to *survivors, the device
 * form to the device word *d_count, which the call itself zeroes on the stream
 * first.  Only the survivors' rows of the out-state are written.
 * Order: the survivors of each block of 256 consecutive input paths are
 * contiguous in the out-state and keep their order; the order of the blocks is
 * unspecified.  Sort by slot to compare.
 * The step is out of place: an out-state array that shares a byte with an
 * in-state array, a round array, colour or another out-state array is
 * RTW_E_INVALID.  Further RTW_E_INVALID: a NULL context or array (n > 0), n or
 * colour_slots > 2^32, in the device form a buffer smaller than n records
 * (colour: colour_slots) or not aligned for its records (as rtw_shade_rays';
 * mult / res / colour as weight, slot 4, d_count 8).  RTW_E_UNSUPPORTED on a
 * multi-device or virtual-rank context.  All of these are refused before any
 * device call.  A slot >= colour_slots: the host form refuses it
 * (RTW_E_INVALID); in a device buffer it is the caller's error and that path's
 * colour is skipped, not written (rtw_camera_rays_device's policy for a pixel
 * index).  background is the camera's (3 doubles, converted to the context's
 * precision).  No scene needs to be staged.  Query stats: is_light_pdf = 6,
 * rays = n, hits = survivors.
 *
 * rtw_render_wavefront: the driver.  It adds the samples [first_sample,
 * first_sample + n_samples) of every pixel onto sums [H x W x 3] f64 (in / out;
 * row j = 0 is the bottom row, as rtw_render), in sample order, so windows
 * compose bit for bit and RTW_F64 equals rtw_render at chunk 1 bit for bit.
 * Samples run in batches of B: per batch rtw_camera_rays_device for each sample
 * b into slots [b * W * H, (b + 1) * W * H), begin, then up to max_depth rounds
 * of rtw_hit_rays_device (t_min = f64::EPSILON), rtw_shade_rays_device and the
 * advance over ALL the batch's live paths, one pinned 8-byte readback of the
 * survivor count per round (the next round's n; 0 ends the batch), and the
 * fold sums[p][c] += (double)colour[b][p][c] for b = 0 .. B - 1 in that order.
 * batch = 0: B = clamp(2^22 / (W * H), 1, n_samples); otherwise B = min(batch,
 * n_samples); B x W x H > 2^32 is RTW_E_INVALID.  The state (two path states,
 * one round's arrays, the colours: about 476 bytes a path in RTW_F64, 284 in
 * RTW_F32) belongs to the context, grows on demand and is freed with it.
 * max_depth = 0 adds 0 per sample.  Refused before anything is launched:
 * what rtw_shade_rays refuses (RTW_E_NO_SCENE, RTW_E_NO_LIGHTS,
 * RTW_E_UNSUPPORTED), a NULL cam or sums, first_sample + n_samples > 2^32, an
 * image without pixels, in the device form d_sums smaller than H x W x 3
 * doubles.  Query stats: is_light_pdf = 7, rays = the sum of the rounds' n (a
 * render's `segments`), hits = the SCATTER events (its `lambertian`), kernel_ms
 * = the device time of the whole call. */
int rtw_path_begin_device(rtw_ctx *ctx, uint64_t n, uint32_t first_slot, void *d_mult, size_t mult_bytes, void *d_res,
                          size_t res_bytes, uint32_t *d_slot, size_t slot_bytes, void *stream);
int rtw_path_advance(rtw_ctx *ctx, uint64_t n, const void *mult, const void *res, const uint32_t *slot,
                     const int32_t *event, const void *weight, const void *emitted, const void *next,
                     const uint64_t *rng, void *out_rays, uint64_t *out_rng, void *out_mult, void *out_res,
                     uint32_t *out_slot, void *colour, uint64_t colour_slots, const double background[3], int last,
                     uint64_t *survivors);
int rtw_path_advance_device(rtw_ctx *ctx, uint64_t n, const void *d_mult, size_t mult_bytes, const void *d_res,
                            size_t res_bytes, const uint32_t *d_slot, size_t slot_bytes, const int32_t *d_event,
                            size_t event_bytes, const void *d_weight, size_t weight_bytes, const void *d_emitted,
                            size_t emitted_bytes, const void *d_next, size_t next_bytes, const uint64_t *d_rng,
                            size_t rng_bytes, void *d_out_rays, size_t out_rays_bytes, uint64_t *d_out_rng,
                            size_t out_rng_bytes, void *d_out_mult, size_t out_mult_bytes, void *d_out_res,
                            size_t out_res_bytes, uint32_t *d_out_slot, size_t out_slot_bytes, void *d_colour,
                            size_t colour_bytes, uint64_t colour_slots, const double background[3], int last,
                            uint64_t *d_count, void *stream);
int rtw_render_wavefront(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed, uint32_t first_sample,
                         uint32_t n_samples, uint32_t batch, double *sums);
int rtw_render_wavefront_device(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed, uint32_t first_sample,
                                uint32_t n_samples, uint32_t batch, double *d_sums, size_t sums_bytes, void *stream);

/* ---- feature buffers for denoisers: first-hit albedo, normal, distance ----
 * One fused pass over the render's own primary rays.  For pixel (i, j) and the
 * absolute sample index s it takes the ray of Camera::get_ray (camera.rs:274-
 * 293) -- the ray a render traces for that (seed, pixel, sample): the same
 * stream, the same draws, defocus included -- and its world.hit(&r,
 * f64::EPSILON..=INFINITY).  Each sample contributes 8 channels:
 *   0-2 albedo    hit: by material -- Lambertian its texture's get_colour(u, v,
 *                 p), Metal its albedo, Dielectric (1, 1, 1), DiffuseLight its
 *                 texture's colour (the emitted colour: may exceed 1),
 *                 Invisible (0, 0, 0); miss: the camera's background
 *   3-5 normal    hit: the HitRecord normal, front-face adjusted, as
 *                 rtw_hit_rays reports it (a cuboid's in object space); miss: 0
 *   6   distance  hit: t * sqrt((dx dx + dy dy) + dz dz), each operation
 *                 rounded by itself; miss: 0
 *   7   hits      hit: 1; miss: 0
 * features[(j * W + i) * 8 + c] is the sequential f64 fold ((acc + f_s0) +
 * f_s0+1) + ... over the pixel's samples in increasing s: sums, not means, as
 * every image here; j = 0 is the bottom row.  The sums are f64 in both
 * precisions: RTW_F64 computes each sample in the reference's f64 arithmetic,
 * RTW_F32 in the plain f32 arithmetic of a query, widened exactly.
 *
 * Pixel p folds the samples [first_sample, min(first_sample + n_samples,
 * counts[p])) -- all of [first_sample, first_sample + n_samples) when counts
 * is NULL -- onto features, which is read when first_sample > 0 and defined by
 * the call when it is 0 (a pixel without samples: zeros).  So windows compose
 * bit for bit, and rtw_render_adaptive's counts with first_sample 0 and
 * n_samples = max_samples give the features of exactly the samples each
 * pixel's colour was made of.  cam->samples_per_pixel and max_depth are not
 * read.  n_samples = 0 does nothing.
 * ids (may be NULL): H*W*2 int32 {object id or -1, material id (0 on a miss)}
 * of each pixel's sample 0; written only by a call with first_sample == 0, for
 * the pixels that take a sample, and left untouched otherwise.
 *
 * The pass runs the traversal a render of the scene would run under the same
 * tuning keys (as the ray queries) on its own buffers: a render or a query
 * before and after it is unchanged.  It fills the query stats
 * (rtw_get_query_stats): rays = samples traced, hits, node_visits,
 * sphere_tests, kernel = the world that ran, is_light_pdf = 0, kernel_ms.
 * A plane whose UV is not finite (the reference panics) is handled as
 * rtw_hit_rays handles it: the NaN reaches the texture.
 *
 * Errors: RTW_E_INVALID -- before any device call -- for a NULL context,
 * camera or features, a buffer that is too small or (device form) features
 * not 16-byte aligned, first_sample + n_samples beyond 2^32 - 1, a width or
 * height of 2^16 or more; RTW_E_NO_SCENE before rtw_set_scene;
 * RTW_E_UNSUPPORTED on a multi-device or virtual-rank context.  The host form
 * is synchronous; the device form enqueues on `stream` as rtw_render_device
 * does (NULL: the context's own, RTW_STREAM_NULL: the null stream) and never
 * waits for the device. */
int rtw_render_features(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed, uint32_t first_sample,
                        uint32_t n_samples, const uint32_t *counts, double *features, int32_t *ids);
int rtw_render_features_device(rtw_ctx *ctx, const rtw_camera *cam, uint64_t seed, uint32_t first_sample,
                               uint32_t n_samples, const uint32_t *d_counts, size_t counts_bytes,
                               double *d_features, size_t features_bytes, int32_t *d_ids, size_t ids_bytes,
                               void *stream);

/* ---- denoising: an edge-avoiding a-trous filter over the feature buffers ----
 * Reads a render's colour sums, the feature sums of rtw_render_features for the
 * same samples and the sample counts, and writes the filtered per-sample MEAN
 * [H, W, 3] f64 (encode it with spp = 1).  No scene is needed.  The filter is
 * f64 arithmetic in both precisions; every operation below is one separately
 * rounded f64 operation, never contracted, in the written order, and
 * "x > y ? x : y" is that comparison and select, never fmax.  Image order, j = 0
 * the bottom row.
 *
 * Per pixel p: colour sums S[3] (f32 sums are widened exactly), feature sums
 * F[8], the count n = counts[p], or spp when counts is NULL; nd = (double)n.
 * Prepare:
 *   guide_ok = n > 0 and all 8 of F finite.  A pixel that is not guide_ok is
 *              never a tap source; its output is S / nd, or (0, 0, 0) when n == 0.
 *   c = S / nd;  valid = guide_ok and all of c finite
 *   alb_k = F[k] / nd;  a_k = alb_k > 2^-10 ? alb_k : 2^-10;  demodulate == 0: a_k = 1
 *   e_k = c_k / a_k            (the irradiance; of no account when not valid)
 *   len = sqrt((F3*F3 + F4*F4) + F5*F5);  N = len > 0 ? F[3..5] / len : 0
 *   d = F7 > 0 ? F6 / F7 : 0
 * Iteration k = 0 .. iterations - 1, step = 2^k, s_k = sigma_colour * 2^-k,
 * sc2_k = s_k * s_k (on the host), h = {1/16, 1/4, 3/8, 1/4, 1/16}.  A centre p
 * that is guide_ok visits the taps q = p + (dx, dy) * step, dy = -2..2 outer,
 * dx = -2..2 inner, and skips a tap outside the image, one whose pixel is not
 * guide_ok and one whose pixel is not valid now (a skipped tap adds nothing;
 * it is never multiplied by 0).  Else:
 *   w_n: both normals all zero: 1.  Otherwise t = (Np.x*Nq.x + Np.y*Nq.y) +
 *        Np.z*Nq.z;  t = t > 0 ? t : 0;  t = t * t, normal_power_log2 times;  w_n = t
 *   w_d: mx = dp > dq ? dp : dq.  mx > 0: r = fabs(dp - dq) / mx;  x = r /
 *        sigma_depth;  u = 1 - x*x;  u = u > 0 ? u : 0;  w_d = u * u.  Otherwise 1
 *   w_c: 1 when sigma_colour == 0 or the centre is not valid.  Otherwise g_k =
 *        ep_k - eq_k;  s = (g0*g0 + g1*g1) + g2*g2;  w_c = 1 / (1 + s / sc2_k)
 *   w = (((h[dy+2] * h[dx+2]) * w_n) * w_d) * w_c
 *   num_k = num_k + w * eq_k;  den = den + w
 * After the taps a valid centre takes e'_k = num_k / den (its own tap is a
 * source).  A guide_ok centre that is not valid becomes valid with e' = num /
 * den when fill_nonfinite and den > 0, and is a source from the next iteration
 * on; otherwise it stays as it is.  Iteration k reads the colours of iteration
 * k - 1 and writes another array; the guides do not change.
 * Finish: a valid pixel outputs e_k * a_k; a guide_ok pixel that never became
 * valid outputs S / nd, so the caller sees its NaN.
 *
 * counts may be NULL (spp > 0 then); params may be NULL (the defaults of
 * rtw_denoise_params_default).  sums_precision: RTW_F32 (what an f32 context's
 * rtw_render_image_device writes) or RTW_F64 (the adaptive, window and host
 * entries).  On a multi-device or virtual-rank context the filter runs on the
 * first device, where the gathered image is.  The filter keeps its own buffers:
 * a render, a query or a feature pass before and after it is unchanged.
 * Tuning key denoise_lds: 0 every iteration reads its taps from global memory,
 * 2 every iteration whose tile and halo fit stages them in LDS, 1 (default)
 * the plan's choice; the result is the same bit for bit.
 *
 * Errors: RTW_E_INVALID -- before any device call -- for a NULL context, sums,
 * features or out; iterations outside 1..16, normal_power_log2 above 10,
 * sigma_colour negative, sigma_depth not positive, either infinite or NaN,
 * demodulate or fill_nonfinite above 1; counts NULL with spp 0; a width or
 * height of 2^16 or more; (device form) a buffer that is too small, a pointer
 * that is not 16-byte aligned, d_out overlapping an input.  The host form is
 * synchronous; the device form enqueues on `stream` as rtw_render_device does
 * and never waits for the device. */
typedef struct rtw_denoise_params {
    uint32_t iterations;          /* 1..16 */
    uint32_t normal_power_log2;   /* 0..10: the normal weight is the clamped cosine to the power 2^this */
    double sigma_colour;          /* >= 0; 0: no colour weight */
    double sigma_depth;           /* > 0: relative distance difference at which the depth weight is 0 */
    uint32_t demodulate;          /* 1: filter colour / first-hit albedo */
    uint32_t fill_nonfinite;      /* 1: non-finite pixels take their neighbours' filtered colour */
} rtw_denoise_params;
/* iterations 5, normal_power_log2 5, sigma_colour 0.5, sigma_depth 0.125, demodulate 1, fill_nonfinite 1 */
void rtw_denoise_params_default(rtw_denoise_params *out);
int rtw_denoise(rtw_ctx *ctx, const double *sums, const double *features, const uint32_t *counts, uint32_t spp,
                uint32_t width, uint32_t height, const rtw_denoise_params *params, double *out);
int rtw_denoise_device(rtw_ctx *ctx, const void *d_sums, int sums_precision, size_t sums_bytes,
                       const double *d_features, size_t features_bytes, const uint32_t *d_counts, size_t counts_bytes,
                       uint32_t spp, uint32_t width, uint32_t height, const rtw_denoise_params *params,
                       double *d_out, size_t out_bytes, void *stream);
typedef struct rtw_denoise_stats {
    uint32_t iterations;          /* of the last denoise */
    uint32_t lds_iterations;      /* ... that staged their taps in LDS */
    uint64_t filled;              /* guide_ok pixels that were not valid and became valid */
    uint64_t left_nonfinite;      /* pixels whose output has a non-finite channel */
    double kernel_ms;             /* device time of the whole pass (HIP events) */
} rtw_denoise_stats;
/* Counters of the last denoise -- rtw_denoise or rtw_denoise_variance -- (waits
 * for it); RTW_E_INVALID before the first. */
int rtw_get_denoise_stats(rtw_ctx *ctx, rtw_denoise_stats *stats);

/* ---- variance-guided denoising: the colour stop scaled by each pixel's noise --
 * rtw_denoise's filter with another colour stop: instead of a fixed width it
 * has the width of the centre pixel's own standard error, from the luminance
 * moments {S1, S2} of the render (rtw_render_window_moments,
 * rtw_adaptive_moments), and the variance is filtered along with the colour
 * from iteration to iteration (the SVGF scheme).  A converged pixel is left
 * alone; a noisy one is smoothed.  moments: [H, W, 2] f64, image order.
 *
 * Everything not written here is rtw_denoise's contract verbatim: guide_ok,
 * valid, c, the demodulation floor 2^-10, a, e, N, d, w_n, w_d, h, the tap
 * order (dy outer, dx inner), the skipped taps, the fill, the finish.  Every
 * operation is one separately rounded f64 operation in the written order, and
 * "x > y ? x : y" is that comparison and select.
 * Prepare, additionally, with nd = (double)n:
 *   m = S1 / nd;  q = S2 / nd;  var = q - m*m;  var = var > 0 ? var : 0;
 *   v = var / (nd - 1)                      (the variance of the mean luminance)
 *   aY = ((0.2126 a0) + (0.7152 a1)) + (0.0722 a2)   (1 when demodulate == 0)
 *   ve = v / (aY * aY)                      (... of the irradiance's luminance)
 *   has_var = valid and n > 1 and S1, S2 finite and ve finite; otherwise ve = 0.
 *   (S1 and S2 are asked by themselves: a NaN var would pass the select as 0.)
 *   has_var never changes afterwards: a pixel that is filled later keeps
 *   has_var = false and ve = 0.
 * Iteration k = 0 .. iterations - 1, step = 2^k.  sv2 = sigma_var * sigma_var
 * (on the host), eps = 2^-40.  For a centre p: thr = sv2 * ve_p + eps and
 * Ye_p = ((0.2126 e0) + (0.7152 e1)) + (0.0722 e2) of the colour the iteration
 * reads.  Per tap q that is a source:
 *   g = Ye_p - Ye_q;  s = g * g;  w_c = has_var_p ? 1 / (1 + s / thr) : 1
 *   w = (((h[dy+2] * h[dx+2]) * w_n) * w_d) * w_c
 *   num_k = num_k + w * eq_k;  den = den + w;  vnum = vnum + (w * w) * ve_q
 * After the taps a centre that takes e' = num / den also takes ve' = vnum /
 * (den * den) when has_var; otherwise its ve stays.  The stop is not shrunk by
 * 2^-k: the filtered variance does that.  sigma_var = 0 is allowed (thr = eps).
 * A frame in which no pixel has has_var (every count 1, say) is rtw_denoise
 * with sigma_colour = 0, bit for bit.
 *
 * counts, params, sums_precision, the device, the buffers and tuning key
 * denoise_lds are rtw_denoise's (the staged form keeps 80 bytes per pixel of
 * the tile and its halo, so it fits up to step 4).  Errors: rtw_denoise's, with
 * sigma_var negative, infinite or NaN in place of sigma_colour, and a NULL,
 * too-small, misaligned or overlapped moments array.  rtw_get_denoise_stats
 * reports the call. */
typedef struct rtw_denoise_variance_params {
    uint32_t iterations;          /* 1..16 */
    uint32_t normal_power_log2;   /* 0..10 */
    double sigma_var;             /* >= 0: the colour stop's width in standard errors of the centre */
    double sigma_depth;           /* > 0 */
    uint32_t demodulate;          /* 1: filter colour / first-hit albedo */
    uint32_t fill_nonfinite;      /* 1: non-finite pixels take their neighbours' filtered colour */
} rtw_denoise_variance_params;
/* iterations 5, normal_power_log2 5, sigma_var 2.0, sigma_depth 0.125, demodulate 1, fill_nonfinite 1 */
void rtw_denoise_variance_params_default(rtw_denoise_variance_params *out);
int rtw_denoise_variance(rtw_ctx *ctx, const double *sums, const double *features, const double *moments,
                         const uint32_t *counts, uint32_t spp, uint32_t width, uint32_t height,
                         const rtw_denoise_variance_params *params, double *out);
int rtw_denoise_variance_device(rtw_ctx *ctx, const void *d_sums, int sums_precision, size_t sums_bytes,
                                const double *d_features, size_t features_bytes,
                                const double *d_moments, size_t moments_bytes,
                                const uint32_t *d_counts, size_t counts_bytes,
                                uint32_t spp, uint32_t width, uint32_t height,
                                const rtw_denoise_variance_params *params,
                                double *d_out, size_t out_bytes, void *stream);

/* ---- scenes::simple (scenes/src/lib.rs:155-233) ----------------------- */
/* The library owns the arrays; view them through rtw_world_scene(). grid_n =
 * 11 is the reference scene; larger n gives the synthetic C3/C5 fields. */
typedef struct rtw_world rtw_world;
rtw_world *rtw_scene_simple(uint64_t seed, int grid_n);
const rtw_scene *rtw_world_scene(const rtw_world *w);
/* the camera builder scenes::simple returns (lib.rs:219-226) + main.rs's vfov */
void rtw_world_camera_builder(const rtw_world *w, rtw_camera_builder *out);
void rtw_world_free(rtw_world *w);
/* a reference scene by its bin/src/main.rs name (scenes/src/lib.rs):
 * "simple" (seeded, grid 11), "cornell_box", "debug", "checkered_spheres",
 * "perlin_spheres", "plane", "simple_light", "simple_transform"; the seed
 * drives simple's generator and the Perlin tables.  NULL for other names. */
rtw_world *rtw_scene_named(const char *name, uint64_t seed);

/* ---- Perlin::new (perlin.rs:46-58) ------------------------------------- */
/* The reference fills the tables from thread_rng; here from the build's
 * seeded xoshiro256++: rand_vec = 256 UnitSphere samples, then perm_x, perm_y,
 * perm_z, each the identity shuffled by j = Uniform::new(i, 256) for i < 255.
 * rand_vec: 768 doubles; perm: 768 values (perm_x, perm_y, perm_z). */
int rtw_perlin_generate(uint64_t seed, double *rand_vec, uint32_t *perm);

/* ---- SampledColour / PPM (colour.rs:14-36; main.rs:89-104) ------------ */
/* sums -> 8-bit RGB, rows flipped so that row 0 is the TOP row:
 * (256 * clamp(sqrt(sum / spp), 0, 1)) as u8, saturating, NaN -> 0. */
int rtw_encode_rgb8(const double *sums, uint32_t width, uint32_t height, uint32_t spp,
                    uint8_t *out_rgb);
/* Writes the reference's P3 "image.ppm" text; returns bytes written or < 0. */
int rtw_write_ppm(const char *path, const double *sums, uint32_t width, uint32_t height,
                  uint32_t spp);
/* The same for the f32 sums of a speed-mode render (each sum widened to f64
 * exactly, then encoded as above). */
int rtw_encode_rgb8_f32(const float *sums, uint32_t width, uint32_t height, uint32_t spp,
                        uint8_t *out_rgb);
int rtw_write_ppm_f32(const char *path, const float *sums, uint32_t width, uint32_t height,
                      uint32_t spp);
/* The same arithmetic with each pixel's own sample count (counts: H*W, as
 * rtw_render_adaptive returns them) in place of spp. */
int rtw_encode_rgb8_counts(const double *sums, const uint32_t *counts, uint32_t width,
                           uint32_t height, uint8_t *out_rgb);
int rtw_write_ppm_counts(const char *path, const double *sums, const uint32_t *counts,
                         uint32_t width, uint32_t height);

#ifdef __cplusplus
}
#endif
#endif /* RTW_H */
