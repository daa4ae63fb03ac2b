/*
 * rtw_gpu.h -- C ABI of the MI355X-native path-tracing hot path.
 *
 * Drop-in boundary for dariooddenino/zig-raytracing-weekend's per-pixel sample
 * loop.  The reference's only entry point into the loop is
 *
 *     pub fn render(self: *Camera, raytrace: *RayTraceState, context: Task) !void
 *                                                        (src/camera.zig:93)
 *
 * called by RenderThread.renderFn (src/main.zig:66-68) for each of 8 Tasks
 * spawned by startRender (src/main.zig:314-326).  It reads the Camera fields
 * derived by Camera.init (src/camera.zig:118-154), the world (a BVHTree of
 * Spheres, src/bvh.zig:17-104, src/objects.zig:68-148), and writes the
 * SharedStateImageWriter float4 buffer (src/camera.zig:21-66).  The entry
 * points below replace exactly that: a host (Zig via @cImport, C++, or Python
 * via ctypes) describes the scene once (rtw_scene_create, replaces the
 * pointer graph of Hittable/Material/Texture unions), derives the camera
 * (rtw_camera_init, replaces Camera.init) and calls rtw_render for a pixel
 * range and a sample range (replaces Camera.render for one Task).
 *
 * Plain C types only; no HIP or torch types cross the boundary (streams and
 * device buffers are passed as void*).  Every function returns an RTW_* status;
 * rtw_last_error() returns a thread-local message for the last failure.
 * No exceptions cross the ABI.  The library never frees caller memory.
 *
 * Threading: render calls on one rtw_ctx may come from several threads at once
 * (the reference's 8 RenderThreads, src/main.zig:314-326): they are serialised
 * per context, and a device-API call on another stream than the previous call
 * waits for that call's work on the device.  rtw_scene_destroy must not race a
 * render on the same context.
 */
#ifndef RTW_GPU_H
#define RTW_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_ABI_VERSION 8

enum rtw_status {
    RTW_OK = 0,
    RTW_E_INVALID = -1,     /* bad argument / inconsistent scene */
    RTW_E_HIP = -2,         /* HIP runtime error (message in rtw_last_error) */
    RTW_E_OOM = -3,         /* device or host allocation failed */
    RTW_E_CANCELLED = -4,   /* cancel flag observed between sample batches */
    RTW_E_NODEVICE = -5     /* no gfx950 device visible */
};

/* ---------------------------------------------------------------------------
 * Scene description (host memory, caller-owned, read once by rtw_scene_create)
 * ------------------------------------------------------------------------- */

/* Sphere.init / Sphere.initMoving (src/objects.zig:80-92).  48 bytes. */
typedef struct rtw_sphere {
    float center1[3];
    float radius;
    float center2[3];          /* used iff is_moving: center_vec = center2 - center1 */
    uint32_t is_moving;
    uint32_t material;         /* index into materials[] */
    uint32_t _pad[3];
} rtw_sphere;

/* Material union (src/material.zig:11-144).  32 bytes. */
enum rtw_material_kind {
    RTW_MAT_LAMBERTIAN = 0,    /* albedo = textures[texture] */
    RTW_MAT_METAL = 1,         /* albedo[3], fuzz (already clamped <= 1 as Metal.fromColor does) */
    RTW_MAT_DIELECTRIC = 2,    /* ir */
    RTW_MAT_DIFFUSE_LIGHT = 3, /* emit = textures[texture] */
    RTW_MAT_ISOTROPIC = 4      /* albedo = textures[texture] (needs ConstantMedium; not in the sphere path) */
};
typedef struct rtw_material {
    uint32_t kind;
    uint32_t texture;
    float fuzz;
    float ir;
    float albedo[3];
    float _pad;
} rtw_material;

/* Texture union (src/textures.zig:10-124).  48 bytes. */
enum rtw_texture_kind {
    RTW_TEX_SOLID = 0,         /* even[] = color_value */
    RTW_TEX_CHECKER = 1,       /* scale = inv_scale, even[], odd[] */
    RTW_TEX_IMAGE = 2,         /* image = index into images[] */
    RTW_TEX_NOISE = 3          /* perlin = index into perlins[], scale */
};
typedef struct rtw_texture {
    uint32_t kind;
    uint32_t image;
    uint32_t perlin;
    float scale;
    float even[3];
    float _p0;
    float odd[3];
    float _p1;
} rtw_texture;

/* zstbi.Image as used by RtwImage (src/rtw_image.zig:5-62): RGBA8, 4 B/texel. */
typedef struct rtw_image {
    const uint8_t* data;
    uint32_t width, height, bytes_per_row, _pad;
} rtw_image;

/* Perlin tables (src/perlin.zig:76-101).  4608 bytes. */
typedef struct rtw_perlin {
    float ranvec[256][3];
    uint16_t perm_x[256], perm_y[256], perm_z[256];
} rtw_perlin;

/* Quad.init (src/objects.zig:193-210): corner q, edges u, v.  The library derives
 * normal = unitVector(cross(u, v)), d = dot(normal, q), w = n / dot(n, n) and the
 * box fromPoints(q, q + u + v).pad() exactly as Quad.init does.  48 bytes.
 * shape (formerly padding, which every caller passed as 0): the interior test on the plane
 * coordinates (alpha, beta) of the hit point.  RTW_QUAD_PARALLELOGRAM: 0 <= alpha, beta <= 1,
 * Quad.hit.  RTW_QUAD_TRIANGLE: also alpha + beta <= 1 -- the triangle q, q + u, q + v, the book's
 * first "additional 2D primitive"; same plane, normal, front face and (u, v) = (alpha, beta) as the
 * quad; its box is that of its three vertices, padded as Quad.init pads.  Any other value is
 * refused by rtw_scene_create*.  A library that knows triangles exports rtw_debug_quad_hit (the
 * ABI version and every struct are those of ABI 8). */
enum rtw_quad_shape {
    RTW_QUAD_PARALLELOGRAM = 0,
    RTW_QUAD_TRIANGLE = 1
};
typedef struct rtw_quad {
    float q[3];
    uint32_t material;
    float u[3];
    uint32_t shape;            /* rtw_quad_shape */
    float v[3];
    uint32_t _p1;
} rtw_quad;

/* A Hittable (src/objects.zig:39-48) by kind + index into its array. */
enum rtw_object_kind {
    RTW_OBJ_SPHERE = 0,        /* spheres[index] */
    RTW_OBJ_QUAD = 1,          /* quads[index] */
    RTW_OBJ_INSTANCE = 2,      /* instances[index] */
    RTW_OBJ_MEDIUM = 3         /* media[index] */
};
typedef struct rtw_object {
    uint32_t kind;
    uint32_t index;
} rtw_object;

/* Translate / RotateY (src/objects.zig:292-443). */
enum rtw_transform_kind {
    RTW_XF_TRANSLATE = 0,      /* v = offset */
    RTW_XF_ROTATE_Y = 1        /* v[0] = angle in degrees (sin/cos as RotateY.init) */
};
typedef struct rtw_transform {
    uint32_t kind;
    float v[3];
} rtw_transform;

#define RTW_MAX_XF 3
enum { RTW_INST_LIST = 1u };   /* rtw_instance.flags: the members form a HittableList (its box
                                  starts from the zero Aabb{}, objects.zig:264-279); else one primitive */
enum { RTW_INST_BVH = 2u };    /* rtw_instance.flags: the library builds a private BVH over the members in object
                                  space (a Hittable{.tree} under the transforms) and walks it instead of testing
                                  them one after another.  Same box, same closest hit as the list.  Instances of
                                  more than 127 members get one whether flagged or not. */
/* A HittableList (createBox, src/objects.zig:264-290, 510-532) of members[first ..
 * first + count) -- spheres or quads -- wrapped in xf[0] (innermost) .. xf[n_xf-1]
 * (outermost), e.g. Translate(RotateY(createBox(...))) = {ROTATE_Y, TRANSLATE}.  64 bytes. */
typedef struct rtw_instance {
    uint32_t first, count, n_xf, flags;
    rtw_transform xf[RTW_MAX_XF];
} rtw_instance;

/* ConstantMedium.initFromColor/initFromTexture (src/objects.zig:445-460): boundary is
 * a sphere, quad or instance; material = the Isotropic phase function
 * (RTW_MAT_ISOTROPIC).  The one random draw of ConstantMedium.hit (objects.zig:484)
 * is keyed by (path RNG state at the traversal, medium index), not taken from the
 * path's sequential stream, so the result does not depend on the BVH topology. */
typedef struct rtw_medium {
    rtw_object boundary;
    float density;
    uint32_t material;
} rtw_medium;

enum rtw_bvh_mode {
    RTW_BVH_REFERENCE = 0,     /* BVHTree.constructTree (src/bvh.zig:43-71): random axis from the
                                  seeded build stream, std.sort.heap by box min, median split */
    RTW_BVH_SAH = 1            /* binned SAH, single-sphere leaves, children ordered front-to-back
                                  along order_dir.  Same closest hit (topology-independent). */
};

typedef struct rtw_scene_desc {
    const rtw_sphere* spheres;     uint32_t n_spheres;
    const rtw_material* materials; uint32_t n_materials;
    const rtw_texture* textures;   uint32_t n_textures;
    const rtw_image* images;       uint32_t n_images;
    const rtw_perlin* perlins;     uint32_t n_perlins;
    uint64_t bvh_seed;
    uint32_t bvh_mode;
    float order_dir[3];        /* RTW_BVH_SAH child order hint (e.g. camera forward); 0 = (0,-1,0) */
    /* ABI 2: the rest of the Hittable union.  objects = world_objects in order (the
     * BVH leaves); NULL/0 = every sphere in order (ABI 1 behaviour). */
    const rtw_quad* quads;         uint32_t n_quads;
    const rtw_object* members;     uint32_t n_members;     /* instance list entries: spheres/quads */
    const rtw_instance* instances; uint32_t n_instances;
    const rtw_medium* media;       uint32_t n_media;
    const rtw_object* objects;     uint32_t n_objects;
} rtw_scene_desc;

/* ---------------------------------------------------------------------------
 * Camera (src/camera.zig:69-91 fields; rtw_camera_init restates Camera.init)
 * ------------------------------------------------------------------------- */
enum rtw_background_mode {
    RTW_BG_CONSTANT = 0,       /* Camera.background (camera.zig:80, 207); HEAD default black */
    RTW_BG_GRADIENT = 1        /* Book-1 sky, the commented camera.zig:204-206 */
};

typedef struct rtw_camera_params {
    float aspect_ratio;
    uint32_t image_width;
    uint32_t image_height;     /* 0 -> round(width / aspect) (camera.zig:119-121) */
    uint32_t samples_per_pixel;
    uint32_t max_depth;
    uint32_t background_mode;
    float background[3];
    float vfov;
    float lookfrom[3];
    float lookat[3];
    float vup[3];
    float defocus_angle;
    float focus_dist;
    uint32_t pixel_offset;     /* 1 reproduces camera.zig:100-101 (x = i%W + 1, y = i/W + 1) */
} rtw_camera_params;

typedef struct rtw_camera {
    uint32_t image_width, image_height, size, samples_per_pixel, max_depth;
    uint32_t background_mode, pixel_offset;
    uint32_t strata;           /* stratified pixel samples (rtw_camera_set_strata); 0 from rtw_camera_init. The
                                * word was padding: the struct and RTW_ABI_VERSION are those of ABI 8 */
    float center[3], pixel00_loc[3], pixel_delta_u[3], pixel_delta_v[3];
    float u[3], v[3], w[3];
    float defocus_disk_u[3], defocus_disk_v[3];
    float defocus_angle;
    float background[3];
} rtw_camera;

/* ---------------------------------------------------------------------------
 * Entry points
 * ------------------------------------------------------------------------- */
typedef struct rtw_ctx rtw_ctx;

/* Progress callback: samples (pixel x spp) finished so far in this call.
 * Return non-zero to cancel (like RenderThread.stop, src/main.zig:58-60). */
typedef int (*rtw_progress_fn)(uint64_t samples_done, uint64_t samples_total, void* user);

/* Device time per kernel kind of one render call (rtw_render_opts.timing). */
enum { RTW_K_GEN = 0, RTW_K_TRACE = 1, RTW_K_SHADE = 2, RTW_K_TAIL = 3, RTW_K_REDUCE = 4, RTW_K_MEGA = 5,
       RTW_K_COUNT = 8 };
typedef struct rtw_kernel_timing {
    float ms[RTW_K_COUNT];         /* summed HIP-event time of the launches of each kind */
    uint32_t launches[RTW_K_COUNT];
} rtw_kernel_timing;

typedef struct rtw_render_opts {
    uint32_t spp_batch;        /* samples per kernel launch (cancel/progress granularity); 0 = auto */
    uint32_t flags;            /* RTW_RENDER_* */
    uint64_t* counters;        /* optional device-side stats out (RTW_STAT_COUNT u64) or NULL */
    rtw_kernel_timing* timing; /* optional host out: per-kernel device time (the call then synchronises) */
    /* ABI 5: stop and progress, polled before every spp batch and after each one (a call given any of
     * them synchronises after every batch).  Samples of the batches that finished stay in the buffer
     * and its .w is the last finished batch's end (camera.zig:56), so a stopped render can resume. */
    const volatile uint8_t* running; /* RenderThread.running (src/main.zig:50, a Zig `bool`; stop() clears
                                        it, main.zig:58-60; Camera.render polls it, camera.zig:107):
                                        0 = stop, non-zero = go on; NULL = not polled */
    const volatile int32_t* cancel;  /* non-zero = stop (rtw_render's flag); NULL = not polled */
    rtw_progress_fn progress;        /* samples finished so far in this call; non-zero return = stop */
    void* user;                      /* passed to progress */
} rtw_render_opts;

enum { RTW_RENDER_NO_SYNC = 1u };  /* rtw_render_device: do not synchronise the stream */
enum { RTW_STAT_RAYS = 0, RTW_STAT_NODES = 1, RTW_STAT_LEAVES = 2, RTW_STAT_SAMPLES = 3, RTW_STAT_NAN = 4,
       RTW_STAT_TAIL_RAYS = 5, /* rays traced by the wavefront tail kernel (subset of RAYS) */
       RTW_STAT_COUNT = 8 };

int rtw_version(void);
/* ABI 6: the library's build id, the first 16 hex digits of the sha256 of its sources (csrc/Makefile);
 * PMC passes under profiles/ record it, and bench.py derives no roofline from a pass of another build. */
const char* rtw_build_id(void);
const char* rtw_last_error(void);
int rtw_device_count(int* out);

/* Camera.init (src/camera.zig:118-154). Host-only arithmetic; shared by every caller. */
int rtw_camera_init(const rtw_camera_params* params, rtw_camera* out);

/* Stratified pixel samples (the jittering of "The Rest of Your Life"; detected by this symbol's presence).
 * With strata = n > 1, sample s of a pixel -- s the absolute 0-based index, whatever call, batch, shard or
 * GPU renders it -- is jittered inside cell k = s mod n^2 of an n x n grid over the pixel: si = k mod n along
 * pixel_delta_u, sj = k div n along pixel_delta_v (row order), and with inv = 1 / (float)n
 *     px = ((si + rx) * inv) - 0.5,  py = ((sj + ry) * inv) - 0.5     (fp32, each operation rounded)
 * where rx, ry are the two draws the plain jitter -0.5 + r takes, in its order: no draw is added, and every
 * later draw of the path keeps its place.  n^2 consecutive samples from a multiple of n^2 visit every cell
 * once; samples past the last full pass are a prefix of the next one.  0 and 1 are off: the plain jitter,
 * bit for bit.  A cell is closed on both sides (px can round up to +0.5).
 * rtw_camera_set_strata stores n; n > RTW_MAX_STRATA or a null camera: RTW_E_INVALID, the camera left as
 * it was.  Every render entry point and rtw_debug_sample refuse a camera whose strata exceeds the maximum. */
#define RTW_MAX_STRATA 256
int rtw_camera_set_strata(rtw_camera* cam, uint32_t n);

/* Builds the BVH (bvh_mode) on the host, flattens it to 32-byte depth-first
 * nodes with skip links, and uploads nodes / materials / textures / images /
 * perlin tables to `device`.  Replaces generateWorld's BVHTree.init
 * (src/main.zig:309, src/bvh.zig:22-29).
 * device = RTW_DEVICE_CPU makes a HOST context (no GPU needed): rtw_render on it runs the
 * same per-sample code as the GPU on host threads (bit-identical images); the device-buffer
 * and multi-GPU entry points refuse it (RTW_E_INVALID). */
#define RTW_DEVICE_CPU (-1)
int rtw_scene_create(const rtw_scene_desc* desc, int device, rtw_ctx** out);

/* Implementation choices of a context (ABI 3).  Every setting renders the SAME image,
 * bit for bit (each one is a different schedule of the same fp32
 * operations); they exist for A/B measurement and the invariance tests.  Start from
 * rtw_tuning_defaults() -- the product defaults -- and change fields. */
enum rtw_kernel_kind {
    RTW_KERNEL_WAVEFRONT = 0,  /* wavefront path tracer (rtw_wavefront.hip), the product path */
    RTW_KERNEL_PERSISTENT = 1, /* persistent megakernel (render_persistent_v1), a baseline */
    RTW_KERNEL_SIMPLE = 2      /* one lane per pixel (render_pixels_v0), a baseline */
};
enum {  /* rtw_tuning.lds: what the kernels may stage in LDS when it fits */
    RTW_LDS_NODES = 1u,        /* the 32-B node array (wavefront trace / fused step / tail) */
    RTW_LDS_CNODES = 2u,       /* the compact nodes of every octant copy (small static sphere SAH trees) */
    RTW_LDS_MATERIALS = 4u,    /* materials beside the compact nodes */
    RTW_LDS_SHADE = 8u,        /* materials | textures | image records of small scenes */
    RTW_LDS_GEOMETRY = 16u,    /* quads | members | instances of small object scenes */
    RTW_LDS_PERLIN = 32u,      /* Perlin tables (noise scenes) */
    RTW_LDS_MEGA_NODES = 64u,  /* the persistent megakernel's node stage */
    RTW_LDS_ALL = 127u
};
enum {  /* rtw_tuning.fuse */
    RTW_FUSE_STEP = 1u,        /* gen + trace + shade of an iteration in one kernel (trees staged in LDS) */
    RTW_FUSE_TAIL_LDS = 2u,    /* the tail kernel walks the LDS stage */
    RTW_FUSE_GLOBAL = 4u       /* the fused step also for trees read through L1/L2 */
};
#define RTW_OTREE_NO_CULL 0x100u  /* rtw_tuning.object_tree */
typedef struct rtw_tuning {
    uint32_t kernel;           /* rtw_kernel_kind (default WAVEFRONT) */
    uint32_t bvh_orders;       /* 0 = auto (SAH sphere scenes: 4 for small static untextured trees whose 4-copy
                                  compact stage fits half the LDS -- Book-1 --, else 8; other scenes 1), 1, 4 or 8
                                  (4: copies ordered by the x and z signs, the walk takes y's near/far per ray;
                                  half the compact-LDS stage; ABI 7) */
    uint32_t sah_max_leaf;     /* spheres per SAH leaf (default 1) */
    uint32_t compact_nodes;    /* 1 = 16-B fp16 node walk for static sphere SAH trees (default); 2 = 32-B nodes
                                  with fp32 boxes for packed FMAs, with bvh_orders 4 (else as 1; ABI 7) */
    uint32_t fast_box;         /* 1 = FMA slab test on the padded SAH boxes (default); 0 = aabb.zig arithmetic */
    uint32_t fast_reject;      /* 1 = exact sphere fast-reject filter (default) */
    uint32_t lds;              /* RTW_LDS_* (default RTW_LDS_ALL) */
    uint32_t fuse;             /* RTW_FUSE_* (default STEP | TAIL_LDS) */
    uint32_t wf_iters;         /* wavefront iterations before the tail kernel (1..100; default 0 = auto: 4, or 100 -- every bounce, no tail -- on image-textured scenes) */
    uint32_t mega_shade_min;   /* persistent kernel: lanes ready before a shading pass (default 48; 1..64) */
    uint32_t mega_waves;       /* persistent kernel: launch-bound variant (default 1; 1, 6 or 8) */
    uint32_t mega_tile_order;  /* persistent kernel: 1 = last tile row first (default) */
    uint32_t cpu_threads;      /* host context (RTW_DEVICE_CPU): render threads, 0 = every available core */
    uint32_t wide_walk;        /* 1 = two-wide stack walk for static sphere SAH trees read through L1/L2 (default) */
    uint64_t wf_paths;         /* wavefront batch capacity in paths; 0 = auto (2^29 within 35 % of free memory) */
    uint32_t tile_lists;       /* camera rays of static sphere scenes (fused step) test per-8x8-tile candidate lists:
                                  0 = off, 1 = default (lists of <= 32 spheres, 128 for trees of > 4096 nodes),
                                  2..128 = that cap (ABI 4; 128 since ABI 8).  A tile with more candidates than the
                                  cap walks the tree.  Trees of <= 4096 nodes build the lists by a flat scan of the
                                  leaves, larger ones by a frustum walk of the tree; both serve every cap
                                  (rtw_debug_tile_lists reads them back) */
    uint32_t hoist;            /* SAH sphere scenes: spheres whose box dwarfs the rest of the scene (a ground
                                  sphere) are tested first by every walk, ahead of the tree (default 1; ABI 5) */
    uint32_t sort_iters;       /* fused step (trees staged in LDS): wavefront iterations 0 .. sort_iters-1 file
                                  their survivors into 64-slot blocks by direction, so the next iteration's
                                  waves walk coherent rays (default 3; 0 = plain appends; ABI 5) */
    uint32_t sort_bits;        /* direction-bucket key bits of those blocks: 0..4 (default 4 = 16 buckets: x, z signs,
                                  4 elevation levels; 0 = one block per wave, appends in order; ABI 5) */
    uint32_t sort_iters_split; /* the same for the split trace / shade kernels (trees through L1/L2: C4), whose
                                  HBM-bound shade pays more for the scattered block stores (default 1; ABI 5) */
    uint32_t object_tree;      /* SAH trees of object scenes (quads / instances / media), bits 0..7: inner nodes
                                  whose box has >= this % of the area of the node above are not emitted (their
                                  children take their place: box tests that almost always pass), 0 = the plain
                                  SAH tree, default 90; | RTW_OTREE_NO_CULL: instance and medium leaves do not
                                  test the instance's world box before its transforms and members (ABI 5,
                                  formerly padding) */
    uint32_t clds_shape;       /* compact-LDS kernels (fused step, tail) of a 4-copy tree: 0 = auto (= 4), 1 = one
                                  1024-thread block per CU, 4 = two blocks of 768 threads (6 waves per SIMD) when
                                  the stage fits half the LDS; the 8-copy stage always runs one block (ABI 7; ABI 8
                                  refuses the former 2 / 3, two blocks of 512 / 640 threads, which lost their A/Bs) */
    uint32_t deal;             /* how the wavefront's waves share work (ABI 8), RTW_DEAL_* bits; 0 = all static,
                                  default 59 = RUNS | TAIL | SMALL | ITERS | SINGLES16 */
} rtw_tuning;
enum {  /* rtw_tuning.deal (ABI 8: the per-stripe tail claims, bit 4, and the two-launch tail, bit 64, lost their
           A/Bs and were removed -- diag/deal_tail_modes.patch; both bits are now refused) */
    RTW_DEAL_RUNS = 1u,        /* iteration 0's runs of 16 samples of a tile (the last chunks singly) claimed from a
                                  counter per stripe group as its waves finish, instead of dealt round-robin */
    RTW_DEAL_TAIL = 2u,        /* the tail's input chunks claimed from one counter instead of each wave's own list */
    RTW_DEAL_SMALL = 8u,       /* the dynamic deal also on batches with fewer than 192 chunks of 64 paths per wave
                                  (which otherwise keep the static shares) */
    RTW_DEAL_ITERS = 16u,      /* the fused step's iterations >= 1 claim their stripe's chunks from a counter per
                                  stripe group */
    RTW_DEAL_SINGLES16 = 32u,  /* iteration 0's last 16 x (waves) chunks go singly (else the last 4 x) */
    RTW_DEAL_SMALL_SORT = 128u,/* direction bucketing (sort_iters / sort_iters_split) also on batches with fewer
                                  than 192 chunks per wave, which otherwise append in order: a test knob that runs
                                  the queues of the large benched batches on small images (same image) */
    RTW_DEAL_ALL = 187u
};

void rtw_tuning_defaults(rtw_tuning* out);
/* rtw_scene_create with explicit tuning (NULL = defaults). */
int rtw_scene_create_ex(const rtw_scene_desc* desc, int device, const rtw_tuning* tuning, rtw_ctx** out);
void rtw_scene_destroy(rtw_ctx* ctx);

/* Camera.render for the pixel range [pix_begin, pix_end) (linear index
 * i = y*W + x, the Task chunk of src/camera.zig:94-95) and the 0-based sample
 * range [spp_begin, spp_end) (number_of_samples = s+1, camera.zig:98).
 * accum: caller-owned HOST float4[W*H] (ColorAndSamples, camera.zig:21-39):
 * rgb += sample radiance in sample order, w = spp_end (camera.zig:55-56).
 * seed keys the counter-based RNG: identical (seed, pixel, sample) -> identical
 * draws regardless of ranges, batching, devices.  cancel (may be NULL) is
 * polled between sample batches (camera.zig:107).  Blocking. */
int rtw_render(rtw_ctx* ctx, const rtw_camera* cam, uint32_t pix_begin, uint32_t pix_end,
               uint32_t spp_begin, uint32_t spp_end, uint64_t seed, float* accum,
               const volatile int32_t* cancel, rtw_progress_fn progress, void* user);
/* ABI 5: the same with rtw_render_opts (spp_batch and the stop/progress fields; flags, counters and
 * timing must be 0/NULL).  A host context polls running/cancel per pixel as well (camera.zig:107).
 * A stopped call returns RTW_E_CANCELLED with the finished batches in accum. */
int rtw_render_ex(rtw_ctx* ctx, const rtw_camera* cam, uint32_t pix_begin, uint32_t pix_end,
                  uint32_t spp_begin, uint32_t spp_end, uint64_t seed, float* accum, const rtw_render_opts* opts);

/* Same, on a DEVICE buffer float4[W*H] already resident on ctx's device, on
 * `stream` (a hipStream_t, or NULL for the ctx's own stream).  With
 * RTW_RENDER_NO_SYNC the call only enqueues work. */
int rtw_render_device(rtw_ctx* ctx, const rtw_camera* cam, uint32_t pix_begin, uint32_t pix_end,
                      uint32_t spp_begin, uint32_t spp_end, uint64_t seed, float* d_accum,
                      void* stream, const rtw_render_opts* opts);

/* Row-interleaved shard of an image for multi-GPU:
 * renders rows r with (r / rows_per_block) % n_shards == shard into a compact
 * device buffer d_tile (float4[rows_in_shard * W], rows in increasing order). */
int rtw_render_rows_device(rtw_ctx* ctx, const rtw_camera* cam, uint32_t rows_per_block, uint32_t n_shards,
                           uint32_t shard, uint32_t spp_begin, uint32_t spp_end, uint64_t seed,
                           float* d_tile, void* stream, const rtw_render_opts* opts);
/* ABI 5: the same shard into a caller-owned HOST tile float4[rows_in_shard * W] (blocking), on a GPU
 * context or a host context (RTW_DEVICE_CPU: the shard rendered on host threads, e.g. one process per
 * rank without a GPU).  opts as rtw_render_ex (may be NULL). */
int rtw_render_rows(rtw_ctx* ctx, const rtw_camera* cam, uint32_t rows_per_block, uint32_t n_shards, uint32_t shard,
                    uint32_t spp_begin, uint32_t spp_end, uint64_t seed, float* tile, const rtw_render_opts* opts);
uint32_t rtw_shard_rows(uint32_t height, uint32_t rows_per_block, uint32_t n_shards, uint32_t shard);
/* Image row of row `tile_row` of a shard's compact tile (>= height: padding; 0xFFFFFFFF: bad spec).
 * The same function places rows in the render kernels and the multi-GPU gather. */
uint32_t rtw_shard_image_row(uint32_t rows_per_block, uint32_t n_shards, uint32_t shard, uint32_t tile_row);
/* ABI 7: rows_per_block | RTW_ROWS_BALANCED (every shard entry point, rtw_render_multi* included): rounds of
 * n_shards row blocks dealt in alternating order (round k: shard s takes the round's block s if k is even, block
 * n_shards - 1 - s if odd, so no shard always gets the lowest block of a round), then the rows left over (height
 * mod (rows_per_block * n_shards)) split evenly -- `sub` = ceil(rest / n_shards) consecutive rows per shard, in the
 * same alternating position, in one more block slot of its tile -- so the shards' row counts differ by at most sub
 * instead of by one block.  rtw_shard_image_row_h: the image row of a tile row under either layout (>= height:
 * padding; 0xFFFFFFFF: bad spec). */
#define RTW_ROWS_BALANCED 0x80000000u
uint32_t rtw_shard_image_row_h(uint32_t height, uint32_t rows_per_block, uint32_t n_shards, uint32_t shard,
                               uint32_t tile_row);

/* ---------------------------------------------------------------------------
 * Multi-GPU frame in one process (the north star's "8-GPU tile shard
 * + one RCCL gather" behind the FFI).  Replaces startRender's 8-thread split
 * (src/main.zig:314-326) of Camera.render (src/camera.zig:93-116) with N devices:
 * device k renders the row blocks b with b % N == k (rtw_render_rows_device) into
 * a compact tile; one grouped RCCL send/recv moves every tile to device 0, where
 * the rows are scattered into the frame.  Unless RTW_RENDER_FRESH, the frame's
 * current rows are first scattered to the devices the same way, so progressive
 * calls accumulate exactly as on one device: the result is bit-identical to
 * rtw_render_device for any N (counter-based RNG keyed by seed, pixel, sample).
 * ------------------------------------------------------------------------- */
typedef struct rtw_multi rtw_multi;
/* ctxs[k]: one context per device, each from rtw_scene_create(desc, device_k) with the
 * same desc; ctxs[0]'s device holds the frame.  Creates the RCCL communicators
 * (ncclCommInitAll) once.  The contexts must outlive the rtw_multi and must not be
 * rendered on by other callers during an rtw_render_multi* call. */
int rtw_multi_create(rtw_ctx* const* ctxs, uint32_t n, rtw_multi** out);
void rtw_multi_destroy(rtw_multi* m);
enum { RTW_RENDER_FRESH = 2u };  /* rtw_render_multi_device: start the range from zero, do not read d_accum */
/* d_accum: float4[W*H] on ctxs[0]'s device; stream: a hipStream_t of that device or NULL.
 * opts: spp_batch, flags (RTW_RENDER_NO_SYNC, RTW_RENDER_FRESH) and the ABI-5 stop/progress fields
 * are honoured (every device renders batch b, all of them finish, then progress and the flags are
 * polled; the tiles meet on device 0 once, after the last finished batch -- also on a stop, which
 * returns RTW_E_CANCELLED with the frame holding every finished batch); counters and timing must
 * be NULL. */
int rtw_render_multi_device(rtw_multi* m, const rtw_camera* cam, uint32_t rows_per_block, uint32_t spp_begin,
                            uint32_t spp_end, uint64_t seed, float* d_accum, void* stream,
                            const rtw_render_opts* opts);
/* Same on a caller-owned HOST float4[W*H] (ColorAndSamples), blocking; cancel is polled
 * between spp batches (rtw_render_multi_ex: the full rtw_render_opts, e.g. the Zig `running` flag
 * and a progress callback). */
int rtw_render_multi(rtw_multi* m, const rtw_camera* cam, uint32_t rows_per_block, uint32_t spp_begin,
                     uint32_t spp_end, uint64_t seed, float* accum, const volatile int32_t* cancel);
int rtw_render_multi_ex(rtw_multi* m, const rtw_camera* cam, uint32_t rows_per_block, uint32_t spp_begin,
                        uint32_t spp_end, uint64_t seed, float* accum, const rtw_render_opts* opts);
/* ABI 5: devices of the rtw_multi and ranks of its RCCL communicator (ncclCommCount of device 0's). */
int rtw_multi_info(rtw_multi* m, uint32_t* n_devices, int* rccl_ranks);

/* SharedStateImageWriter texel update: u8(256*clamp(sqrt(rgb/w),0,0.999)), alpha 255
 * (src/camera.zig:58-65, src/color.zig:43-62). Host, n pixels. */
int rtw_texture_from_accum(const float* accum, uint32_t n, uint8_t* rgba_out);
/* The same texel update on the device (d_accum float4[n] -> d_rgba u8x4[n], HBM), enqueued on
 * `stream` (NULL = the context's default device stream of device 0's current context). */
int rtw_texture_from_accum_device(const float* d_accum, uint32_t n, uint8_t* d_rgba, void* stream);

/* ---------------------------------------------------------------------------
 * Output formats (the reference's README TODO "Output selector"
 * and main.zig:47 "save to file").  Host-only, over the float4 accumulator.
 * ------------------------------------------------------------------------- */
enum rtw_ppm_style {
    RTW_PPM_WRITECOLOR = 0,    /* color.zig:64-69 writeColor: round(256 * toGamma(c)), "r g b\n" per pixel
                                  (the format of the reference's image2.ppm; values reach 256) */
    RTW_PPM_STDOUT = 1         /* stdout.zig:5-18 printPpmToStdout: floor(255.999 * toGamma(c)), "r g b\t"
                                  (the format of image.ppm) */
};
/* P3 PPM "P3\n<w> <h>\n255\n" + pixels row-major from the top row.  Writes at most cap
 * bytes; *len = bytes of the whole encoding (call with out = NULL to size the buffer).
 * Returns RTW_E_INVALID if out != NULL and cap < *len.  NaN components print "nan". */
int rtw_encode_ppm(const float* accum, uint32_t width, uint32_t height, uint32_t style, char* out, size_t cap,
                   size_t* len);
/* ---------------------------------------------------------------------------
 * Progressive / resumable renders.  rtw_render* accumulate
 * samples [spp_begin, spp_end) onto the buffer in sample order, so any split
 * of [0, spp) into consecutive calls -- including across a checkpoint -- is
 * bit-identical to one call.
 * ------------------------------------------------------------------------- */
/* countSamples (src/main.zig:470-477): f32 sum of accum[i][3] in index order -- the
 * control panel's progress (vs spp * n) and POWER (= samples / elapsed ms, :495-503). */
float rtw_count_samples(const float* accum, uint64_t n);
/* FNV-1a 64 of the scene's device image (nodes + geometry + materials + textures); a
 * checkpoint records it so a resume on a different scene or BVH is refused. */
int rtw_scene_hash(rtw_ctx* ctx, uint64_t* out);
/* Checkpoint file (little endian): "RTWCKPT1", u32 version 1, u32 spp_done, u64 seed,
 * u64 scene_hash, rtw_camera, u64 n_pixels, float4[n_pixels] accumulator, u32 CRC-32 of
 * everything before it.  read: cam/seed/hash/spp_done may be NULL; accum must hold
 * cap_pixels float4 (n_pixels must equal cap_pixels) -- RTW_E_INVALID on any mismatch or
 * corruption. */
int rtw_checkpoint_write(const char* path, const rtw_camera* cam, uint64_t seed, uint64_t scene_hash,
                         uint32_t spp_done, const float* accum);
int rtw_checkpoint_read(const char* path, rtw_camera* cam, uint64_t* seed, uint64_t* scene_hash,
                        uint32_t* spp_done, float* accum, uint64_t cap_pixels);

/* 8-bit RGBA PNG (zlib stored blocks, no filtering) of u8x4 texels, e.g. the
 * SharedStateImageWriter texture_buffer (rtw_texture_from_accum).  Same sizing contract. */
int rtw_encode_png(const uint8_t* rgba, uint32_t width, uint32_t height, uint8_t* out, size_t cap, size_t* len);

/* Host-only: build + flatten the BVH exactly as rtw_scene_create does, without
 * touching a device (nodes_out may be NULL to query the count). */
int rtw_scene_flatten(const rtw_scene_desc* desc, void* nodes_out, uint32_t cap, uint32_t* n_out,
                      uint32_t* depth_out);

/* Introspection for tests / reports. */
typedef struct rtw_scene_stats {
    uint32_t n_nodes, n_leaves, n_inner, depth;
    uint64_t device_bytes;
    uint32_t axis_draws;
    uint32_t n_hoisted;        /* spheres emitted ahead of the tree (rtw_tuning.hoist) */
    float extent;              /* ABI 6: E = max |coordinate| over every object box and inner node (SAH) */
    float box_pad;             /* ABI 6: E * 2^-19, the inner-box pad of the FMA slab test (0: exact walk) */
} rtw_scene_stats;
int rtw_scene_stats_get(rtw_ctx* ctx, rtw_scene_stats* out);

/* ---------------------------------------------------------------------------
 * Light importance sampling ("The Rest of Your Life": the mixture density).  With lights
 * registered, a Lambertian or Isotropic scatter aims half its directions at a uniformly
 * chosen point of a uniformly chosen light and draws the other half as before, and
 * weights the path by scattering_pdf / (0.5 light_pdf + 0.5 scattering_pdf): an unbiased
 * estimator of the same image with less noise where the lights are small.  Emission,
 * Metal and Dielectric are unchanged; there are no shadow rays.  A caller detects the
 * capability by the presence of these symbols (the ABI version and every struct are
 * those of ABI 8).  Quads are sampled by area (a triangle light, rtw_quad.shape, by folding the
 * same two draws across its diagonal, with the density over half the area), static spheres by the cone they subtend
 * (from inside a sphere light: every direction).  Sphere lights came after quad lights
 * under the same ABI version: a caller detects them by trying the call, which a library
 * without them refuses with RTW_E_INVALID.  Out of scope: lights inside instances, moving
 * spheres, and any light in a scene of spheres alone (no quad, instance or medium: those
 * scenes render with kernels of their own, which have no mixture-density form).
 * ------------------------------------------------------------------------- */
#define RTW_MAX_LIGHTS 16
/* Registers the objects that diffuse scatter samples towards. lights[k] must be a top-level
 * RTW_OBJ_QUAD or RTW_OBJ_SPHERE of the scene's object list (not an instance member, not a
 * medium boundary) whose material is RTW_MAT_DIFFUSE_LIGHT; a sphere must be static
 * (is_moving == 0) with a finite radius > 0, in a scene with at least one quad, instance or
 * medium. Quads and spheres may be mixed, no (kind, index) twice; n <= RTW_MAX_LIGHTS.
 * n = 0 (lights may be NULL) clears:
 * the context then renders exactly as one that never had lights. Must not race a render on
 * ctx. Works on GPU and host contexts.  Anything else returns RTW_E_INVALID with a message and
 * leaves the registered lights as they were.  rtw_scene_hash covers the registered list.
 * rtw_multi_create refuses contexts whose lists differ: each context is given its lights. */
int rtw_scene_set_lights(rtw_ctx* ctx, const rtw_object* lights, uint32_t n);
/* Copies the registered lights (out may be NULL to query the count; at most cap are written). */
int rtw_scene_lights_get(rtw_ctx* ctx, rtw_object* out, uint32_t cap, uint32_t* n_out);

/* ---------------------------------------------------------------------------
 * Smooth shading and mesh UVs: per-vertex normals and texture coordinates on triangles
 * (rtw_quad.shape == RTW_QUAD_TRIANGLE).  A caller detects the capability by the presence of
 * these symbols (the ABI version and every struct are those of ABI 8).  With (alpha, beta) the
 * hit's coordinates along u and v and w0 = (1 - alpha) - beta:
 *   RTW_ATTR_NORMALS: the shading normal is unit(((w0 n0) + (alpha n1)) + (beta n2)), or the
 *     geometric normal n where that sum vanishes, turned to n's side, then towards the ray as
 *     the geometric normal is (front_face stays the geometric test).  Scatter uses it; emission,
 *     the medium test and the light density keep the geometric normal.
 *   RTW_ATTR_UVS: (u, v) = ((w0 uv0) + (alpha uv1)) + (beta uv2), instead of (alpha, beta).
 * Plain fp32 in this association on every backend.  Out of scope: attributes on
 * parallelograms, tangent frames, and a guard for scattered directions below the face.
 * ------------------------------------------------------------------------- */
enum { RTW_ATTR_NORMALS = 1u, RTW_ATTR_UVS = 2u };
typedef struct rtw_vertex_attr {      /* 64 bytes; corners in the order q, q + u, q + v */
    float normal[3][3];               /* need not be unit: normalised at registration */
    float uv[3][2];
    uint32_t flags;                   /* RTW_ATTR_* */
} rtw_vertex_attr;
/* Registers attrs[k] on quad quads[k] (an index into the scene's quads, wherever the triangle
 * sits: top level, list or tree instance, medium boundary, registered light).  Replaces the
 * registered set; n = 0 (both pointers may be NULL) clears: the context then renders exactly as
 * one that never had attributes.  Refused with RTW_E_INVALID, the entry named in rtw_last_error
 * and the registered set left as it was: an index out of range, a parallelogram, an index listed
 * twice, unknown flag bits, with RTW_ATTR_NORMALS a normal that is not finite or has zero length,
 * with RTW_ATTR_UVS a uv that is not finite.  Fields whose flag is not set are ignored (stored
 * as 0).  Must not race a render on ctx.  Works on GPU and host contexts.  rtw_scene_hash covers
 * the registered set; rtw_multi_create refuses contexts whose sets differ. */
int rtw_scene_set_vertex_attrs(rtw_ctx* ctx, const uint32_t* quads, const rtw_vertex_attr* attrs, uint32_t n);
/* Copies the registered entries, normals normalised (either output may be NULL; at most cap are written). */
int rtw_scene_vertex_attrs_get(rtw_ctx* ctx, uint32_t* quads, rtw_vertex_attr* attrs, uint32_t cap, uint32_t* n_out);

/* ---------------------------------------------------------------------------
 * Environment maps: image-based lighting with importance sampling.  A caller detects the
 * capability by the presence of these symbols (the ABI version and every struct are those of
 * ABI 8).  With an environment registered, a ray that leaves the scene adds thr * env(d) instead
 * of the camera's background -- at every bounce, camera rays included, whatever background_mode
 * says -- and rtw_render_guides* report env(d) as a miss's albedo.rgb.  Ray queries are untouched.
 *   env(d): d' = (c d.x - s d.z, d.y, s d.x + c d.z) with s, c the sine and cosine of rotate_y as
 *     RotateY.init takes them (radians = degrees * pi / 180 in fp32, then sin / cos);
 *     (u, v) = sphere_uv(unit_vector(d')); column floor(clamp(u) W), row floor((1 - clamp(v)) H),
 *     both clamped to the map (texture_value's image lookup, nearest texel, row 0 = +y); the
 *     texel's radiance, scale * texel, one fp32 product per channel taken at registration.
 *   RTW_ENV_SAMPLE: the map is light number n_lights of the mixture density of
 *     rtw_scene_set_lights: the uniform pick is over n_lights + 1, the draw order stays s, then (if
 *     s < 0.5) k, a, b, and the light density is the sum over the lights plus
 *     D(texel of d) / max(sin(theta_d), 2^-12), divided by n_lights + 1.  The texel weights are
 *     lum(scale * texel) * sin(pi (row + 0.5) / H), lum = 0.2126 r + 0.7152 g + 0.0722 b; the
 *     marginal (rows) and conditional (columns) distributions are built in fp64 and stored as
 *     fp32, their last entries exactly 1; b picks the row and a the column -- the smallest index
 *     whose entry exceeds the draw --, each draw remapped linearly inside its cell; the direction
 *     is sphere_uv's inverse.  A map whose weights sum to 0 renders with sampling off.  Lambertian
 *     and Isotropic scatter use the mixture; Metal, Dielectric and emission are unchanged.
 * Plain fp32 in one association on every backend (DESIGN.md §Environment maps), so a GPU context
 * and a host context render the same bits.  Scenes of spheres alone take an environment too: they
 * then render with the general kernels instead of their own (slower; profiles/environment/).
 * Out of scope: bilinear filtering; maps above RTW_ENV_MAX_WIDTH x RTW_ENV_MAX_HEIGHT; an
 * environment hidden from camera rays; rotation about other axes; environment hits in ray
 * queries; a filter for the direct view of an HDR sun (its pixels alias as the map's texels do).
 * ------------------------------------------------------------------------- */
#define RTW_ENV_MAX_WIDTH 4096
#define RTW_ENV_MAX_HEIGHT 2048
enum { RTW_ENV_SAMPLE = 1u };         /* the map is also a light of the mixture density */
typedef struct rtw_environment {
    const float* rgb;                 /* width*height*3 floats, row-major, row 0 = +y (top): linear radiance, no 8-bit clamp */
    uint32_t width, height;
    float scale[3];                   /* radiance = scale * texel */
    float rotate_y;                   /* degrees about y, sin/cos taken as RotateY.init takes them */
    uint32_t flags;                   /* RTW_ENV_* */
    uint32_t _pad;
} rtw_environment;
/* Registers the environment (env == NULL clears: the context then renders exactly as one that
 * never had one, bit for bit).  The map is copied at the call: the caller's memory is read once.
 * Refused with RTW_E_INVALID, the offender named in rtw_last_error and the registered
 * environment left as it was: a null rgb, a zero dimension or one above the maxima, a texel or
 * scale that is negative, NaN or infinite, a non-finite rotate_y, unknown flag bits.  Must not
 * race a render on ctx.  Works on GPU and host contexts.  rtw_scene_hash covers the map, scale,
 * rotation and flags; rtw_multi_create refuses contexts whose environments differ. */
int rtw_scene_set_environment(rtw_ctx* ctx, const rtw_environment* env);
/* Copies the registered environment as given: *out (rgb = NULL; width = height = 0 when none is
 * registered) and, if rgb is non-NULL, at most cap_floats floats of the map. */
int rtw_scene_environment_get(rtw_ctx* ctx, rtw_environment* out, float* rgb, uint64_t cap_floats);
/* Host-only test hook: the device's environment functions -- the same fp32 operations -- on a
 * context of either kind.  For dirs[3i..] the radiance env(d), the density
 * D / max(sin(theta), 2^-12) of the map's own sampler (0 when the map is not sampled) and the
 * texel looked up (row * width + column); for draws[2i..] = (a, b) the sampled direction.  Any
 * pointer may be NULL.  RTW_E_INVALID without a registered environment. */
int rtw_debug_environment(rtw_ctx* ctx, uint32_t n, const float* dirs, const float* draws,
                          float* radiance, float* pdf, float* sampled_dir, uint32_t* texel);

/* ---------------------------------------------------------------------------
 * Denoised previews: first-hit guide buffers and an edge-avoiding a-trous filter (Dammertz et al. 2010) over the
 * accumulator, for the handful of samples per pixel an interactive viewer shows.  A caller detects the capability
 * by the presence of these symbols (the ABI version and every struct are those of ABI 8).  Kernels of their own:
 * no render changes by a bit.  DESIGN.md §Denoised previews.
 *
 * Guides.  One deterministic ray per pixel: from cam->center through the pixel centre (pixel_offset applied as a
 * render applies it), no jitter, no defocus disk, time 0, no RNG draw -- so no seed.  It is traced by the walk and
 * the hit record every render uses, except that it sees through ConstantMedium (smoke is noise to filter, not an
 * edge).  Both outputs are float4[W*H] in image order:
 *   hit:   normal_depth = (the record's normal -- the shading normal where vertex attributes are registered --
 *          turned towards the ray, depth = t * length(ray direction) > 0);  albedo.rgb = the texture's value at the
 *          hit (Lambertian, Isotropic), the metal's albedo, (1, 1, 1) for a dielectric, the emit texture's value
 *          for a DiffuseLight;  albedo.w = 1
 *   miss:  normal_depth = 0 (a hit is depth > 0);  albedo.rgb = the background seen by the ray;  albedo.w = 0
 * The same function runs on the GPU and on a host context: the two agree bit for bit.  Out of scope: guides
 * through glass or mirrors (first hit only) and guides under defocus.
 * rtw_render_guides: host buffers, GPU and host contexts.  rtw_render_guides_device: device buffers of a GPU
 * context (a host context is refused), enqueued on `stream` (NULL: the context's); flags: RTW_RENDER_NO_SYNC.
 *
 * Filter.  Over the accumulator's mean radiance, all in fp32, every operation rounded singly (nothing contracted),
 * one function for the host and the device, so they agree bit for bit:
 *   pre-pass   c = rgb * (1 / w);  with RTW_DENOISE_DEMODULATE  c = c / max(albedo, 2^-8) per channel
 *   pass i     (i = 0 .. passes - 1, spacing s = 2^i)  for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), the tap
 *              q = p + s (dx, dy) is skipped if it is off the image, if its colour is not finite or if its hit
 *              state (depth > 0) differs from the centre's; otherwise
 *                x = ((|dc|^2 kc + |dn|^2 kn) + dz^2 kz),  |v|^2 = (v.x v.x + v.y v.y) + v.z v.z
 *                kc = 1 / (sc sc), sc = sigma_color 2^-i  (term off -- 0 -- for the whole pixel if the centre colour
 *                     is not finite);  kn = 1 / (sigma_normal sigma_normal);
 *                kz = 1 / ((sigma_depth sigma_depth) (z_p z_p)) for a hit centre, else off;  a term whose sigma is 0
 *                     is off
 *                weight = (h[dx] h[dy]) e(x),  h = {1/16, 1/4, 3/8, 1/4, 1/16},  e(x) = exp(-x) (rtw_libm.h
 *                     rtw_expneg: relative error below 2^-20, e(0) = 1, 0 above 87)
 *              out = (sum of weight c_q) / (sum of weight), both sums in tap order; if the sum of weights is 0 the
 *              pixel keeps its input.  A finite centre contributes 9/64, so its sum cannot vanish.
 *   last pass  with DEMODULATE  c = c * max(albedo, 2^-8);  out.rgb = c * w, out.w = w: the accumulator's form, so
 *              rtw_texture_from_accum*, the encoders and the checkpoints work on the result unchanged.
 * A NaN / infinite pixel and a pixel with w = 0 are filled from their neighbours (the latter comes out 0: c * 0).
 * out may alias accum; albedo may be NULL without DEMODULATE.  The two intermediate images belong to the context
 * and grow on demand; the calls take the context lock as renders do.  RTW_E_INVALID with a message, out untouched:
 * passes outside 1 .. RTW_DENOISE_MAX_PASSES, a negative or non-finite sigma, unknown flag bits, width * height == 0
 * (or beyond 2^32 - 1), a null required pointer, rtw_denoise_device on a host context.  Out of scope: a sharded
 * multi-GPU filter (filter device 0's gathered frame), a pixel sub-range.  (The variance-guided filter is
 * rtw_denoise_guided, in the block after this one; temporal filtering is rtw_temporal_accumulate, after that.)
 * ------------------------------------------------------------------------- */
#define RTW_DENOISE_MAX_PASSES 8
enum { RTW_DENOISE_DEMODULATE = 1u };
typedef struct rtw_denoise_params {      /* 32 bytes */
    uint32_t passes;                     /* 1..8; pass i taps at spacing 2^i */
    uint32_t flags;                      /* RTW_DENOISE_* */
    float sigma_color;                   /* pass i uses sigma_color * 2^-i; 0 = term off */
    float sigma_normal, sigma_depth;     /* depth relative to the centre's; 0 = term off */
    float _pad[3];
} rtw_denoise_params;
/* The shipped parameters: the winner of the grid search recorded in profiles/denoise/defaults.json. */
void rtw_denoise_defaults(rtw_denoise_params* p);
int rtw_render_guides(rtw_ctx* ctx, const rtw_camera* cam, float* albedo, float* normal_depth);
int rtw_render_guides_device(rtw_ctx* ctx, const rtw_camera* cam, float* d_albedo, float* d_normal_depth,
                             void* stream, uint32_t flags);
/* Host buffers; GPU contexts (staged through the device: the device form is the fast path) and host contexts. */
int rtw_denoise(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* accum, const float* albedo,
                const float* normal_depth, const rtw_denoise_params* params, float* out);
/* Device buffers of a GPU context, enqueued on `stream` (NULL: the context's); flags: RTW_RENDER_NO_SYNC. */
int rtw_denoise_device(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* d_accum, const float* d_albedo,
                       const float* d_normal_depth, const rtw_denoise_params* params, float* d_out, void* stream,
                       uint32_t flags);
/* Host-only: out[i] = e(x[i]) = exp(-x[i]), the filter's edge-stopping function (rtw_expneg, the device's code). */
int rtw_debug_expneg(uint32_t n, const float* x, float* out);

/* ---------------------------------------------------------------------------
 * Noise estimates and the variance-guided filter: a running per-pixel estimate of the variance of luminance, a
 * noise measure on it (a viewer's stop criterion, a sampler's map) and SVGF's spatial filter (Schied et al. 2017):
 * the a-trous filter above with its colour term measured in standard deviations.  A caller detects the capability by
 * the presence of these symbols (the ABI version and every struct above are those of ABI 8).  Kernels of their own:
 * no render and no rtw_denoise result changes by a bit.  All in fp32, every operation rounded singly in the
 * association written (nothing contracted), one function for the host and the device: they agree bit for bit.
 * DESIGN.md §Noise estimates and the guided filter.
 *
 * Moments.  `moments` is the caller's: two float4[W*H] planes, one after the other -- plane 0 the accumulator as of
 * the last update, plane 1 (mean, M2, n, sw) of the per-batch mean luminance.  All zeros is the reset state (a caller
 * that scrubs its accumulator zeroes the moments).  rtw_moments_update, per pixel, a = accum, p = plane 0:
 *   k = a.w - p.w;  unless k > 0 neither plane changes
 *   inv = 1 / k;  d = (a.rgb - p.rgb) inv;  y = (0.2126 d.r + 0.7152 d.g) + 0.0722 d.b
 *   y not finite: plane 0 = a, plane 1 unchanged;  otherwise (West's weighted update)
 *   sw' = sw + k;  e = y - mean;  mean' = mean + e (k / sw');  M2' = M2 + (k e) (y - mean');  n' = n + 1;  plane 0 = a
 * It works after any render call -- any pixel range, chunk, shard, gather or resumed checkpoint -- and takes what it
 * finds at the first update as one batch.  Derived: for n >= 2, s2 = M2 / (n - 1) is the per-sample variance of
 * luminance (unbiased for batches of unequal size) and v = s2 / sw the variance of the pixel's mean, a v that is not
 * > 0 counting as 0; for n < 2 the variance is unknown.
 *
 * Noise estimate.  err = sqrt(v) / (|mean| + floor): +inf where the variance is unknown (the pixel needs more
 * samples), 0 where v = 0 whatever the divisor.  err (W*H) and tile_max (ceil(W/8) * ceil(H/8), the maximum over each
 * 8 x 8 pixel tile, rows of tiles in image order) may be NULL.  The summary: over = pixels with err > threshold,
 * known = pixels with n >= 2, max_err = the largest finite err (0: none).  Maxima and integer counts only, so the
 * backends agree exactly.  RTW_E_INVALID: a negative or non-finite floor or threshold.
 *
 * Guided filter.  rtw_denoise's arithmetic (pre-pass, taps, skipping, h, e, sums, the wsum = 0 rule, last pass) with
 * params->sigma_color read as sl, in standard deviations, the same in every pass, and:
 *   pre-pass   also a variance plane: v as above, -1 where unknown;  with DEMODULATE  v / (la la),
 *              la = (0.2126 a.r + 0.7152 a.g) + 0.0722 a.b of a = max(albedo, 2^-8)
 *   pass i     vbar = (sum of (g[dx] g[dy]) v_q) / (sum of g[dx] g[dy]), g = {1/4, 1/2, 1/4}, over the 3 x 3 taps at
 *              spacing 1 (dy outer, dx inner) that are on the image, have the centre's hit state, a finite colour and
 *              v_q >= 0.  kl = 1 / (sl sqrt(vbar) + 2^-20); the colour term is off for the pixel with no such tap,
 *              with sl = 0 or where the centre's colour is not finite.  Per tap of the 5 x 5 at spacing 2^i:
 *                tl = |Y_q - Y_p| kl,  Y = (0.2126 c.r + 0.7152 c.g) + 0.0722 c.b of the plane's colour
 *                x = (tl + tn) + tz;  weight = (h[dx] h[dy]) e(x)
 *              v' = (sum of (weight weight) max(v_q, 0)) / (wsum wsum), in tap order; the pixel's own v where
 *              wsum = 0; -1 through every pass where the centre's variance is unknown
 *   last pass  out as rtw_denoise;  variance_out (W*H floats, may be NULL) = v', with DEMODULATE v' (la la), -1 where
 *              unknown: the variance of the filtered mean luminance
 * out may alias accum.  Refusals are rtw_denoise's, plus a null moments; each leaves every output untouched.  The
 * device forms take device buffers of a GPU context (the summary too), are enqueued on `stream` (NULL: the
 * context's) and take flags RTW_RENDER_NO_SYNC; the host-buffer forms serve both kinds of context.  Out of scope:
 * non-uniform sample counts, per-channel variance, moments in checkpoints, a sharded multi-GPU estimate or filter,
 * a pixel sub-range.  (Temporal accumulation is rtw_temporal_accumulate, in the block after this one.)
 * ------------------------------------------------------------------------- */
typedef struct rtw_noise_summary {       /* 24 bytes */
    uint64_t over, known;
    float max_err;
    uint32_t _pad;
} rtw_noise_summary;
int rtw_moments_update(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* accum, float* moments);
int rtw_moments_update_device(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* d_accum, float* d_moments,
                              void* stream, uint32_t flags);
int rtw_noise_estimate(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* moments, float floor,
                       float threshold, float* err, float* tile_max, rtw_noise_summary* out);
int rtw_noise_estimate_device(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* d_moments, float floor,
                              float threshold, float* d_err, float* d_tile_max, rtw_noise_summary* d_out, void* stream,
                              uint32_t flags);
/* The shipped parameters: the winner of the grid search recorded in profiles/denoise_guided/defaults.json. */
void rtw_denoise_guided_defaults(rtw_denoise_params* p);
int rtw_denoise_guided(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* accum, const float* moments,
                       const float* albedo, const float* normal_depth, const rtw_denoise_params* params, float* out,
                       float* variance_out);
int rtw_denoise_guided_device(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* d_accum,
                              const float* d_moments, const float* d_albedo, const float* d_normal_depth,
                              const rtw_denoise_params* params, float* d_out, float* d_variance_out, void* stream,
                              uint32_t flags);

/* ---------------------------------------------------------------------------
 * Temporal reprojection: SVGF's temporal half (Schied et al. 2017).  When the camera of a static scene moves, the
 * accumulator and the moments of the previous camera are carried onto the new one instead of being scrubbed: the
 * guide buffers place every pixel's first hit in world space (normal_depth.w is its distance from the camera
 * centre), and the previous camera saw most of those points too.  The outputs keep the accumulator's and the
 * moments' forms, so rtw_noise_estimate, rtw_denoise_guided, the encoders and further renders take them unchanged.
 * A caller detects the capability by the presence of these symbols (the ABI version and every struct above are those
 * of ABI 8).  A kernel of its own: no render and no filter result changes by a bit.  All in fp32, every operation
 * rounded singly in the association written (nothing contracted), one function for the host and the device: they
 * agree bit for bit.  DESIGN.md §Temporal reprojection.
 *
 * Per pixel (x, y) of the current frame, dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, primes = the previous camera:
 *   look     d = ((pixel00 + du (x + off)) + dv (y + off)) - c;  u = d / sqrt(dot(d, d)) per component
 *            hit (cur_normal_depth.w > 0):  p = c + u depth;  e = p - c';  dist = sqrt(dot(e, e))
 *            miss:  e = u, a point at infinity
 *   project  n = cross(du', dv'),  a = pixel00' - c',  na = dot(n, a)  (once per call);  lambda = na / dot(n, e);
 *            unless 0 < lambda < inf the point is behind the previous camera: no history
 *            r = e lambda - a;  fx = dot(r, du') / dot(du', du') - off';  fy = dot(r, dv') / dot(dv', dv') - off'
 *            (fx, fy) = (i, j) is the centre of the previous frame's pixel (i, j).  rtw_debug_reproject runs exactly
 *            this on the host: e = points[i] - c', or e = dirs[i];  ok = 0 and xy = 0 where there is no history
 *   snap     rx = floor(fx + 1/2), ry = floor(fy + 1/2);  if |fx - rx| <= S and |fy - ry| <= S, S =
 *            RTW_TEMPORAL_SNAP, the one tap (rx, ry) with weight 1: a still camera copies, it does not diffuse
 *   taps     otherwise x0 = floor(fx), tx = fx - x0 (y likewise) and the taps, in this order, (x0, y0) with weight
 *            (1 - tx)(1 - ty), (x0 + 1, y0) with tx (1 - ty), (x0, y0 + 1) with (1 - tx) ty, (x0 + 1, y0 + 1) with tx ty
 *   valid    a tap q counts if its weight is > 0, it is on the image, prev_accum[q] is finite with w > 0, its hit
 *            state (depth > 0) is the centre's and, for hits, |depth_q - dist| <= depth_tolerance dist and
 *            dot(n_cur, n_q) >= normal_cos
 *   hidden   for a hit centre, if any tap on the image with weight > 0 saw a nearer surface (0 < depth_q and
 *            dist - depth_q > depth_tolerance dist, whatever its accumulator holds) no tap is valid: the footprint
 *            straddles an occluder's silhouette, and a point the previous camera could not see must not take the
 *            history of its visible neighbours.  (A farther or differently oriented tap is only skipped.)
 *   blend   ws = the sum of the valid weights;  g_q = weight_q / ws;  h_i = sum of g_q w_q;
 *            mean = sum of g_q (rgb_q (1 / w_q));  h = min(h_i, max_history)  (0 without a valid tap)
 *            out.rgb = mean h + cur.rgb,  out.w = h + cur.w;  with h = 0 out = cur bit for bit.  A current pixel that
 *            is not finite or has w <= 0 contributes nothing: out = (mean h, h), 0 without history either
 *            history_out (W*H floats, may be NULL) = h
 *   moments  (given prev_moments and out_moments, two float4[W*H] planes each as rtw_moments_update's)  over the
 *            valid taps with n_q >= 1:  g'_q = weight_q / (the sum of their weights);  m = sum of g'_q m_q of plane 1's
 *            (mean, M2, n, sw), zeros without such a tap;  where the cap bites (h_i > max_history)
 *            m.sw = m.sw (h / h_i) -- M2 and n stay: s2 = M2 / (n - 1) is a per-sample variance;  then
 *            rtw_moments_update's West step with k = cur.w, inv = 1 / k, y = luma(cur.rgb inv), skipped for a current
 *            pixel that contributes nothing or a y that is not finite.  out plane 1 = m, out plane 0 = out_accum
 * out_accum may be cur_accum itself.  RTW_E_INVALID with a message, every output untouched: an output that overlaps
 * a prev_* buffer (they are gathered from) or any other buffer, cameras of different image sizes, a zero-sized
 * image, a null required pointer, exactly one of prev_moments / out_moments, max_history or depth_tolerance not > 0
 * or not finite, normal_cos outside [-1, 1] or NaN, non-zero params->flags, unknown flag bits,
 * rtw_temporal_accumulate_device on a host context.
 * rtw_temporal_accumulate: host buffers; GPU contexts (staged through a device block of the call's own) and host
 * contexts.  rtw_temporal_accumulate_device: device buffers of a GPU context, enqueued on `stream` (NULL: the
 * context's); flags: RTW_RENDER_NO_SYNC.  Both take the context lock and order themselves on the stream as the
 * filters do.  Out of scope: view-dependent lag on metal and glass (the first hit only, as the guides), defocus,
 * moving spheres (points are taken as static), a sharded multi-GPU frame, history in checkpoints.
 * ------------------------------------------------------------------------- */
#define RTW_TEMPORAL_SNAP 0.015625f      /* 2^-6 pixel: DESIGN.md §Temporal reprojection has the measured round-off */
typedef struct rtw_temporal_params {     /* 32 bytes */
    float max_history;                   /* cap on the history's weight in samples; > 0 */
    float depth_tolerance;               /* relative: |d_prev_tap - |p - c_prev|| <= tol * |p - c_prev|; > 0 */
    float normal_cos;                    /* a tap is valid if dot(n_cur, n_prev_tap) >= normal_cos; in [-1, 1] */
    uint32_t flags;                      /* none yet: non-zero refused */
    float _pad[4];
} rtw_temporal_params;
/* The shipped parameters: the winner of the grid search recorded in profiles/temporal/defaults.json. */
void rtw_temporal_defaults(rtw_temporal_params* p);
int rtw_temporal_accumulate(rtw_ctx* ctx, const rtw_camera* cur_cam, const rtw_camera* prev_cam,
                            const float* cur_accum, const float* cur_normal_depth, const float* prev_accum,
                            const float* prev_normal_depth, const float* prev_moments,
                            const rtw_temporal_params* params, float* out_accum, float* out_moments,
                            float* history_out);
int rtw_temporal_accumulate_device(rtw_ctx* ctx, const rtw_camera* cur_cam, const rtw_camera* prev_cam,
                                   const float* d_cur_accum, const float* d_cur_normal_depth,
                                   const float* d_prev_accum, const float* d_prev_normal_depth,
                                   const float* d_prev_moments, const rtw_temporal_params* params, float* d_out_accum,
                                   float* d_out_moments, float* d_history_out, void* stream, uint32_t flags);
/* Host-only (no context): the projection step above for n points (points[3 i ..], dirs NULL) or n directions
 * (dirs[3 i ..], points NULL): xy[2 i ..] = (fx, fy), ok[i] = 1, or ok[i] = 0 behind the camera. */
int rtw_debug_reproject(const rtw_camera* prev_cam, uint32_t n, const float* points, const float* dirs, float* xy,
                        uint8_t* ok);

/* ---------------------------------------------------------------------------
 * Ray queries: the closest hit, or whether anything is hit, for rays the caller supplies -- picking (the object
 * under the mouse: rtw_trace_rays of one ray of rtw_debug_camera_ray), visibility between points, ambient
 * occlusion, light-map bakes, an integrator of the caller's own written against first hits.  A caller detects the
 * capability by the presence of these symbols (the ABI version and every other struct are those of ABI 8).  Kernels
 * of their own: no render changes by a bit.  DESIGN.md §Ray queries.
 *
 * Same walk as a render.  The walk and the hit record of every render's first bounce: the scene's tree with its
 * hoisted spheres and octant orderings, instance lists and instance trees, the vertex attributes where registered,
 * tmin = 0.001 and the reference's comparisons (Sphere.hit accepts 0.001 < t, Quad.hit 0.001 <= t).  The same
 * function runs on the GPU and on a host context: the two agree bit for bit.
 * Caller's tmax.  A hit is accepted only if t < tmax, whatever the primitive (+inf: unbounded).  A tmax that is not
 * > 0.001, NaN included, is a miss.
 * Media.  Rays see through ConstantMedium, as guide rays do: a medium hit needs a path's RNG key, which a bare ray
 * does not have.
 * Sphere uv.  Sphere hits always carry Sphere.getSphereUv of the outward normal in uv (a render computes it only
 * for the textures that read it).
 * Tied hits.  Of two primitives hit at exactly the same t the one the walk meets first wins (a quad met later at
 * the same t replaces it, as Quad.hit's closed interval has it in the reference): which one that is depends on the
 * tree -- the tuning, the BVH mode, whether an instance has a tree.  t itself does not.
 * Degenerate rays.  A ray with a zero direction, or an infinite or NaN component, gives an unspecified record; the
 * call still returns (the walks only move forward through their skip links) and no other ray's record is affected.
 * Far origins.  An origin further out than 7 x the scene's extent (rtw_scene_stats.extent) is walked with the
 * reference's box arithmetic instead of the FMA slab test, per ray; the hit is the same.
 * No coherence promise.  One lane walks one ray, in the caller's order: rays that start near each other in the
 * array and point the same way are faster (profiles/queries/README.md).
 *
 * A miss writes t = +inf, kind = index = member = prim_kind = prim_index = RTW_HIT_NONE and every other word 0, so
 * records can be compared bit for bit.
 *
 * rtw_trace_rays / rtw_occluded: host buffers; GPU contexts (staged through a device block of the call's own: the
 * device form is the fast path) and host contexts (on the context's cpu_threads).
 * rtw_trace_rays_device / rtw_occluded_device: device buffers of a GPU context (a host context is refused),
 * enqueued on `stream` (NULL: the context's); flags: RTW_RENDER_NO_SYNC.  The buffers are 16-byte aligned.
 * rtw_occluded*: out[i] = 1 if any surface is hit on (0.001, tmax), else 0; the walk stops at the first accepted
 * hit and builds no record.
 * n = 0 is RTW_OK and touches nothing.  RTW_E_INVALID with a message, outputs untouched: a null context, n above
 * 2^32 - 1, a null buffer with n > 0, unknown flag bits, a device entry point on a host context.  The calls take the
 * context lock and order themselves on the stream as renders do.  Out of scope: medium hits, sorting or bucketing
 * the rays, a 1-bit-per-ray mask, sharding a batch over GPUs (split the array), another tmin.
 * ------------------------------------------------------------------------- */
typedef struct rtw_ray {          /* 32 bytes */
    float origin[3];
    float tmax;                   /* hits are accepted on the open interval (0.001, tmax); +inf = unbounded */
    float dir[3];                 /* need not be unit; t is in units of |dir| */
    float time;                   /* for moving spheres (Sphere.getCenter); 0 otherwise */
} rtw_ray;

#define RTW_HIT_NONE 0xFFFFFFFFu
typedef struct rtw_hit {          /* 64 bytes */
    float t;                      /* p = origin + t dir; +inf on a miss */
    uint32_t kind;                /* rtw_object_kind of the top-level object: SPHERE, QUAD or INSTANCE; RTW_HIT_NONE on a miss */
    uint32_t index;               /* into spheres[] / quads[] / instances[] of the scene description */
    uint32_t member;              /* INSTANCE: position in [0, count) of the member hit; else RTW_HIT_NONE */
    float p[3];                   /* world-space hit point */
    uint32_t material;            /* index into materials[] */
    float normal[3];              /* the record's normal turned towards the ray (world space; the shading normal where
                                     vertex attributes are registered) */
    uint32_t front;               /* the geometric front-face test: 1 = the ray meets the outward side */
    float uv[2];
    uint32_t prim_kind, prim_index;  /* the primitive itself: the member's sphere / quad for an instance, else
                                        (kind, index) again */
} rtw_hit;
int rtw_trace_rays(rtw_ctx* ctx, uint64_t n, const rtw_ray* rays, rtw_hit* hits);
int rtw_trace_rays_device(rtw_ctx* ctx, uint64_t n, const rtw_ray* d_rays, rtw_hit* d_hits, void* stream,
                          uint32_t flags);
int rtw_occluded(rtw_ctx* ctx, uint64_t n, const rtw_ray* rays, uint8_t* out);
int rtw_occluded_device(rtw_ctx* ctx, uint64_t n, const rtw_ray* d_rays, uint8_t* d_out, void* stream,
                        uint32_t flags);

/* Copies the flattened node array (32 B per node) to host. */
int rtw_scene_nodes(rtw_ctx* ctx, void* out, uint32_t cap, uint32_t* n_out);
/* Copies the private BVH of instance `instance` (RTW_INST_BVH, or more than 127 members): 32 B per node, the
 * same pre-order / skip-link layout in the instance's object space, sized like rtw_scene_nodes (out may be
 * NULL to query the count).  Leaves: b.y = bits(member index within the instance), b.z = bits(sphere / quad
 * index), b.w = bits(moving | kind << 8); sphere leaves carry (center1, radius) in a.xyz / b.x.
 * *n_out = 0 for an instance without a tree.  Works on host contexts. */
int rtw_scene_instance_nodes(rtw_ctx* ctx, uint32_t instance, void* out, uint32_t cap, uint32_t* n_out);

/* Debug / known-answer hooks, executed ON THE DEVICE by the same device
 * functions the render kernel uses. */
int rtw_debug_rng(rtw_ctx* ctx, uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, float* out);
int rtw_debug_sample(rtw_ctx* ctx, const rtw_camera* cam, uint64_t seed, uint32_t pixel, uint32_t sample,
                     float out[3]);
/* Host-only (no context): Camera.getRay -- get_ray, the code every kernel runs -- for n (pixel, sample) pairs
 * of the render with this seed: pixel pixels[i] (y * image_width + x, the camera's pixel_offset applied as a
 * render applies it), absolute sample index samples[i].  origin[3 i ..], dir[3 i ..], time[i], and
 * jitter[2 i ..] = (px, py), the offsets inside the pixel (see rtw_camera_set_strata).  Any output may be
 * NULL.  A pixel out of range or strata > RTW_MAX_STRATA: RTW_E_INVALID. */
int rtw_debug_camera_ray(const rtw_camera* cam, uint64_t seed, uint32_t n, const uint32_t* pixels,
                         const uint32_t* samples, float* origin, float* dir, float* time, float* jitter);
/* ABI 6, host-only: the walk's sphere fast-reject (sphere_may_hit, the same fp32 operations as the
 * device) and Sphere.hit's exact accept (objects.zig:127-136, tmin = 0.001) for n sphere tests given
 * a = lengthSquared(d), half_b = dot(oc, d), c = lengthSquared(oc) - r*r and closest: the test suite
 * checks that the filter never rejects a test the exact arithmetic accepts. */
int rtw_debug_sphere_filter(uint32_t n, const float* a, const float* half_b, const float* c, const float* closest,
                            uint8_t* may_hit, uint8_t* accept);
/* Host-only (detected by the symbol's presence; the ABI version and every struct are those of ABI 8): the slot
 * arithmetic of the coherent queues' per-wave cursors, the device's code, for n pushing lanes.  A bucket's open
 * block is [blk, blk + 64) and old[i] what the lane's atomic add of 1 on the bucket's cursor returned; fresh[i] is
 * the first slot of the block the bucket opens if it overflows.  over[i] = 0xFFFFFFFF and slot[i] = old[i] inside
 * the block; past it over[i] = j = old[i] - (blk[i] + 64), the lane's index in the fresh block, and slot[i] =
 * fresh[i] + j.  rebase[i] is what the lane with j = 0 adds to the cursor so that it continues in the fresh block. */
int rtw_debug_push_cursor(uint32_t n, const uint32_t* blk, const uint32_t* old, const uint32_t* fresh,
                          uint32_t* slot, uint32_t* over, uint32_t* rebase);
/* Host-only (its presence is how a caller detects triangle support, rtw_quad.shape): Quad.init's derivation
 * (the scene builder's) and Quad.hit's interval, plane and interior tests (quad_t, the code every kernel runs) for
 * n (record, ray) pairs: record quads[i] against the ray origins[3 i ..] + t dirs[3 i ..] on the closed interval
 * [tmin[i], tmax[i]].  hit[i] = 1 with t[i] and alpha_beta[2 i ..] = the hit record's (u, v), else 0 with both
 * left as they were.  A shape other than RTW_QUAD_* returns RTW_E_INVALID naming the record. */
int rtw_debug_quad_hit(uint32_t n, const rtw_quad* quads, const float* origins, const float* dirs, const float* tmin,
                       const float* tmax, uint8_t* hit, float* t, float* alpha_beta);
/* Host-only: the hit record of a triangle with vertex attributes -- Quad.init's derivation, quad_prep and
 * quad_attr, the code every kernel runs -- for n (record, attribute, ray, t) tuples: normal[3 i ..] the shading
 * normal turned towards the ray, uv[2 i ..] the hit's (u, v), front[i] the geometric front-face test.  The
 * attribute is taken as given, except that its normals are normalised as registration normalises them; flags = 0
 * gives quad_prep's record.  A shape other than RTW_QUAD_* or unknown flag bits return RTW_E_INVALID. */
int rtw_debug_quad_shade(uint32_t n, const rtw_quad* quads, const rtw_vertex_attr* attrs, const float* origins,
                         const float* dirs, const float* t, float* normal, float* uv, uint8_t* front);
/* GPU contexts, after a wavefront render: the stripe capacity (slots) of its last batch and the 3 x 256 stripe
 * counters (slots used per output stripe, of the last iterations' queues; a set already reset reads 0).  No
 * counter may exceed the capacity: the queues are not bound-checked on the device. */
int rtw_debug_stripe_counters(rtw_ctx* ctx, uint32_t* stripe_cap, uint32_t counters[768]);
/* GPU contexts (detected by the symbol's presence; the ABI version and every struct are those of ABI 8): the
 * camera-ray candidate lists (rtw_tuning.tile_lists) that a render of pixels [pix_begin, pix_end) with this camera
 * would build, read back.  The launch and its 8x8 tiles are set up as rtw_render_device sets them up; the context's
 * list buffer is filled with 0xFF, one builder runs -- builder 0: the one a render picks, 1: the flat scan, 2: the
 * frustum walk; both run on any tree with compact nodes -- and nothing else: no render kernel, no accumulator.
 * cap 0 = the context's cap, 2..128 = that cap for this call.  *n_tiles tiles, tile t covering x in
 * 8 (t % *n_tx) .. +7 and rows *row0 + 8 (t / *n_tx) .. +7, clipped to the image and the pixel range; counts[t] =
 * the tile's candidates, 0xFFFFFFFF when they exceed the cap (the tile walks the tree); entries[8 (t cap + k) ..] =
 * entry k as the device holds it: bits(centre.xyz), bits(radius * radius), the ordering-0 leaf index, bits(tlow: a
 * lower bound of the ray parameter of a hit), 0, 0, sorted by (tlow, index).  A slot no builder wrote has index
 * 0xFFFFFFFF.  RTW_E_INVALID: a host context, a context that renders without lists (objects, media, moving
 * spheres, fewer than 4 orderings, no compact nodes, tile_lists 0, a camera of max_depth 0), an empty range, or
 * tiles_cap < *n_tiles (which is set first: counts holds tiles_cap words, entries 8 * cap * tiles_cap). */
int rtw_debug_tile_lists(rtw_ctx* ctx, const rtw_camera* cam, uint32_t pix_begin, uint32_t pix_end, uint32_t builder,
                         uint32_t cap, uint32_t* n_tiles, uint32_t* n_tx, uint32_t* row0, uint32_t* counts,
                         uint32_t* entries, uint32_t tiles_cap);
/* Host-only (no context): tile_frustum and tile_reach -- the geometry of both list builders, the same fp32
 * operations -- for the tile whose rendered pixels span [x0, x1] x [y0, y1] (the camera's pixel_offset applied as a
 * render applies it) and n spheres centres[3 i ..], radii[i]: reach[i] = 1 if a camera ray of the tile may hit the
 * sphere (conservative), tlow[i] = the lower bound of such a hit's ray parameter (0 when the sphere reaches the
 * camera plane or is rejected behind it).  *frame_ok (may be NULL) = 0 when the camera's pixel plane gives no frame
 * (pixel_delta_u, pixel_delta_v not orthogonal to 1e-4, or the plane not in front of the centre): the builders then
 * send every tile to the tree walk. */
int rtw_debug_tile_reach(const rtw_camera* cam, float x0, float x1, float y0, float y1, uint32_t n,
                         const float* centres, const float* radii, uint8_t* reach, float* tlow, uint8_t* frame_ok);

#ifdef __cplusplus
}
#endif
#endif /* RTW_GPU_H */
