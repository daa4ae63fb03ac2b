// rtw_internal.h -- private declarations shared by the host runtime
// (rtw_host.hip), the BVH builder (rtw_bvh.hip) and the kernels (rtw_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <condition_variable>
#include <atomic>
#include <algorithm>
#include <mutex>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "rtw_layout.h"
#include "../../include/rtw_gpu.h"

struct rtw_scene_desc;

// Everything one launch of the path-tracing kernel reads (passed by value as
// kernel arguments; scalars live in SGPRs).
struct rtw_launch {
    // scene (device pointers)
    const float4* nodes;
    const uint4* cnodes;         // compact 16-B copy of `nodes` (static sphere SAH trees) or null; with cnode32
                                 // the 32-B fp32-box form (two uint4 per node, 4-copy trees)
    const uint4* w2nodes;        // two-wide records of ordering 0 (rtw_wide2_nodes) or null
    const uint32_t* w2leaf;      // their leaf slots' hit ids (ordering-0 leaf index)
    const float4* cvec;          // per-sphere center_vec (moving spheres)
    const rtw_dev_sphere* sph;   // every sphere (instance members)
    const rtw_dev_quad* quads;
    const rtw_dev_instance* insts;
    const uint32_t* members;
    const rtw_dev_medium* media;
    const rtw_dev_material* mats;
    const rtw_dev_texture* texs;
    const uint8_t* images;
    const rtw_dev_image* img_info;
    const float4* perlin;        // RTW_PERLIN_BYTES per table
    uint32_t n_nodes;
    uint32_t n_perlin;
    uint32_t w2_stack;           // entries of the two-wide walk's per-lane LDS stack (its max depth)
    uint32_t tile_lists;         // camera rays of the fused step of static sphere scenes test per-tile candidate
                                 // lists of at most this many spheres (0 = off; more candidates: the walk)

    // camera (Camera.init outputs, src/camera.zig:118-154)
    float center[3], pixel00[3], du[3], dv[3], disk_u[3], disk_v[3], background[3];
    float defocus_angle;
    uint32_t W, H, max_depth, bg_mode, pixel_offset;

    // work: rows [row0, row0 + n_rows) of the logical row space, pixels
    // restricted to linear range [pix_begin, pix_end); samples [s0, s1)
    uint32_t row0, n_rows;
    uint32_t pix_begin, pix_end;
    uint32_t s0, s1;
    // row mapping: logical row r -> image row
    //   shard mode (n_shards > 0): y = ((r / rpb) * n_shards + shard) * rpb + r % rpb, out idx = r*W + x
    //   plain mode: y = r, out idx = y*W + x
    uint32_t rpb, n_shards, shard;
    uint64_t key0;               // mix64(seed + 0*G): render-domain key
    float4* accum;
    unsigned long long* counters;  // RTW_STAT_COUNT or nullptr

    // persistent kernel (v1) work queue: tiles of RTW_TILE_W x RTW_TILE_H logical pixels
    uint32_t* work_counter;      // zeroed before every launch
    uint32_t n_tiles_x, n_tiles;
    uint32_t shade_min;          // lanes that must be ready before a shading pass (<= 64)
    // Two words no kernel reads (the host's dispatchers alone read `feat`; the second held a launch-bound variant
    // nothing consults): the scene features in 12 bits, and beside them the address of the registered environment's
    // block (rtw_dev_env, rtw_layout.h; rtw_scene_set_environment) in 48 -- every address a device or a host
    // hands out fits --, 0 = none.  In place, so sizeof(rtw_launch) and every offset a kernel reads stay what they
    // were (see vattrs below).  Read through rtw_env_of, by the RTW_F_ENV kernels only.
    uint32_t feat : 12;          // RTW_F_* scene features up to RTW_F_TREE (selects the kernel instantiation)
    uint32_t _spare : 4;
    uint32_t env_hi : 16;        // bits 32 .. 47 of the environment block's address
    uint32_t env_lo;             // bits 0 .. 31
    uint32_t tile_order;         // 1 = last tile row first (default), 0 = first row first
    uint32_t use_lds;            // 1 = stage the BVH in LDS when it fits (default), 0 = read nodes from L1/L2
    uint32_t fast_reject;        // 1 = exact sphere fast-reject filter (default), 0 = always the IEEE path
    uint32_t fast_box;           // 1 = FMA slab test on padded boxes (SAH trees only), 0 = aabb.zig arithmetic
    uint32_t inst_cull;          // 1 = instance / medium leaves test the instance's padded world box first
                                 // (only with fast_box; rtw_tuning.object_tree without RTW_OTREE_NO_CULL)
    uint32_t n_orders;           // 1, or 4 / 8 sign-ordered copies of the node array (SAH sphere scenes)
    uint32_t cnode32;            // 1: cnodes are the 32-B fp32-box nodes (rtw_tuning.compact_nodes 2)
    // per-vertex normals / uvs of triangles (rtw_scene_set_vertex_attrs; RTW_F_ATTR kernels), read through L1/L2.
    // The pointer sits where two of the four dispatch knobs below were, and those four -- read by the host's
    // launch code only, never by a kernel -- share one word: sizeof(rtw_launch) and every offset a kernel reads stay
    // what they were.  (The kernels that call texture_value out of line keep a copy of this struct in scratch: one
    // more pointer at its end cost each of them 16 B of scratch.)
    const rtw_dev_vattr* vattrs; // null: none registered; else one record per quad, parallel to `quads`
    uint32_t clds_shape : 8;     // compact-LDS kernels of a 4-copy tree: 0 / 1 = one 1024-thread block per CU,
                                 // 4 = two blocks of 768 threads (rtw_tuning.clds_shape)
    uint32_t wf_lds : 8;         // wavefront trace: stage the node array(s) in LDS when they fit
    uint32_t wf_clds : 8;        // wavefront trace: stage the compact nodes (all orders) in LDS when they fit
    uint32_t wf_fuse : 8;        // with the compact LDS stage: one gen+trace+shade kernel per iteration,
                                 // bit 1: the tail walks the LDS stage too (bits 0 .. 2 of rtw_tuning.fuse)
    uint32_t strata;             // rtw_camera.strata: n x n jitter cells per pixel (0 / 1: off; rtw_device.h stratum_of)
    uint32_t perlin_lds;         // fused step with the node array in LDS: Perlin tables staged in LDS too
    uint32_t mat_lds;            // compact-LDS fused step: bytes of the material array staged in LDS (0: off)
    uint32_t shade_lds;          // node-LDS kernels: bytes of materials | textures | image records (contiguous
                                 // in the scene blob) staged in LDS when small; 0 = read through L1/L2
    uint32_t geom_lds;           // node-LDS step/tail: bytes of quads | members | instances (contiguous in the
                                 // scene blob) staged in LDS too; 0 = read through L1/L2
    // per-instance trees (RTW_F_TREE scenes; rtw_bvh.hip InstTreeBuilder), read through L1/L2
    const float4* inodes;        // every instance tree's 32-B nodes, one after the other (rtw_dev_instance.tree)
    uint32_t hit_bits;           // RTW_F_TREE kernels: the hit id is leaf node | member << hit_bits (else 24)
    // light importance sampling (rtw_scene_set_lights; RTW_F_PDF kernels), read through L1/L2
    uint32_t n_lights;           // 0: none registered -- the kernels without RTW_F_PDF run
    const rtw_dev_light* lights; // n_lights records by kind: a quad's geometry is quads[lights[k].quad], a
                                 // sphere's centre and radius are in the record
};
static_assert(sizeof(rtw_launch) == 416 && offsetof(rtw_launch, env_lo) == 328 && offsetof(rtw_launch, vattrs) == 360 && offsetof(rtw_launch, perlin_lds) == 376 &&
                  offsetof(rtw_launch, inodes) == 392 && offsetof(rtw_launch, lights) == 408,
              "rtw_launch keeps its size and the offsets its kernels read");

#define RTW_TILE_W 16
#define RTW_TILE_H 16
#define RTW_TILE (RTW_TILE_W * RTW_TILE_H)

// scene feature bits: kernels are instantiated per feature set so Book-1
// (solid textures, static spheres, no lights) carries no texture/motion code
#define RTW_F_CHECKER 1u
#define RTW_F_IMAGE 2u
#define RTW_F_NOISE 4u
#define RTW_F_MOVING 8u
#define RTW_F_LIGHT 16u
#define RTW_F_GEOM 32u      // quads / instances (non-sphere BVH leaves)
#define RTW_F_MEDIUM 64u    // ConstantMedium leaves
#define RTW_F_SPHERES 31u   // every sphere-scene feature
#define RTW_F_ALL 127u
#define RTW_F_TREE 128u     // some instance has a private BVH (inst_tree_t); only ever set on top of RTW_F_ALL
#define RTW_F_PDF 256u      // lights are registered (rtw_launch.n_lights > 0): diffuse scatter samples the mixture
                            // density (scatter_finish); only ever set on top of RTW_F_ALL [| RTW_F_TREE], by the
                            // dispatchers (rtw_feat_of), never stored in rtw_launch.feat
#define RTW_F_ATTR 512u     // vertex attributes are registered (rtw_launch.vattrs): a triangle's hit record takes its
                            // shading normal and (u, v) from them (quad_attr); only ever set on top of RTW_F_ALL |
                            // RTW_F_TREE [| RTW_F_PDF], by the dispatchers (rtw_feat_of), never stored in rtw_launch.feat
#define RTW_F_ENV 1024u     // an environment is registered (rtw_env_of(L) != null): a miss looks the map up instead of
                            // the camera's background, and with RTW_ENV_SAMPLE the map is one more light of the mixture
                            // density; only ever set on top of RTW_F_ALL | RTW_F_TREE | RTW_F_PDF [| RTW_F_ATTR], by
                            // the dispatchers (rtw_feat_of), never stored in rtw_launch.feat

// max nodes staged in LDS by the persistent kernel (48 KiB)
#define RTW_MEGA_LDS_NODES_MAX 1536

struct rtw_kernel_info {
    int blocks_per_cu;
    int n_cu;
};
// the registered environment's block, or null (host and device)
__host__ __device__ inline const rtw_dev_env* rtw_env_of(const rtw_launch& L) {
    return reinterpret_cast<const rtw_dev_env*>(((uint64_t)L.env_hi << 32) | (uint64_t)L.env_lo);
}
inline bool rtw_env_set(rtw_launch& L, const rtw_dev_env* e) {
    const uint64_t a = reinterpret_cast<uint64_t>(e);
    L.env_hi = (uint32_t)(a >> 32) & 0xFFFFu;
    L.env_lo = (uint32_t)a;
    return rtw_env_of(L) == e;  // false: an address above 2^48
}
// the features a launch's kernels are picked by: the scene's, | RTW_F_PDF with lights registered, | RTW_F_ATTR with
// vertex attributes registered, | RTW_F_ENV with an environment registered
inline uint32_t rtw_feat_of(const rtw_launch& L) {
    return L.feat | (L.n_lights ? RTW_F_PDF : 0u) | (L.vattrs ? RTW_F_ATTR : 0u) | (rtw_env_of(L) ? RTW_F_ENV : 0u);
}
// What the registered features make of a feature set, the rule every dispatcher opens with (pick_feat below, the
// wavefront's wf_pick_feat): vertex attributes run on top of every feature and the instance trees (a scene without
// a tree runs them too: inst_hit_t falls back to the member loop), with or without the lights' mixture density;
// lights on top of every feature; instance trees (inst_tree_t) likewise.  0: none of the three bits is set.
// RTW_F_TREE is only ever set on top of RTW_F_ALL, so a dispatcher's "checker only" rule never sees it: testing
// TREE before that rule (here) or after it picks the same class.  An environment runs on top of all of it, the
// mixture density included (its kernels check n_lights, vattrs and the sample flag at run time as the RTW_F_PDF and
// RTW_F_ATTR code does): two classes, with and without the vertex attributes, cover every combination -- a scene of
// spheres alone too, whose 32-B node arrays (octant copies, hoisted leaves) the general walk reads.
inline uint32_t rtw_feat_prefix(uint32_t f) {
    if (f & RTW_F_ENV) return RTW_F_ALL | RTW_F_TREE | RTW_F_PDF | RTW_F_ENV | (f & RTW_F_ATTR);
    if (f & RTW_F_ATTR) return RTW_F_ALL | RTW_F_TREE | RTW_F_ATTR | (f & RTW_F_PDF);
    if (f & RTW_F_PDF) return RTW_F_ALL | (f & RTW_F_TREE) | RTW_F_PDF;
    return (f & RTW_F_TREE) ? (RTW_F_ALL | RTW_F_TREE) : 0u;
}
// The class of the per-sample kernels (render_pixels_v0, render_persistent_v1, debug_sample_kernel, the host
// backend's sample loop): the prefix, the two sphere-scene classes, else every feature.
inline uint32_t rtw_pick_feat(uint32_t f) {
    if (const uint32_t p = rtw_feat_prefix(f)) return p;
    if ((f & ~RTW_F_CHECKER) == 0) return f ? RTW_F_CHECKER : 0u;
    return RTW_F_ALL;
}
// The class table of those kernels: visit(c, f) calls f(std::integral_constant<uint32_t, c>) if c is listed.
template <uint32_t... C>
struct RtwClasses {
    template <typename F>
    static bool visit(uint32_t c, F&& f) {
        return ((c == C && (f(std::integral_constant<uint32_t, C>{}), true)) || ...);
    }
};
using RtwObjectClasses =
    RtwClasses<RTW_F_ALL, RTW_F_ALL | RTW_F_TREE, RTW_F_ALL | RTW_F_PDF, RTW_F_ALL | RTW_F_TREE | RTW_F_PDF,
               RTW_F_ALL | RTW_F_TREE | RTW_F_ATTR, RTW_F_ALL | RTW_F_TREE | RTW_F_PDF | RTW_F_ATTR,
               RTW_F_ALL | RTW_F_TREE | RTW_F_PDF | RTW_F_ENV, RTW_F_ALL | RTW_F_TREE | RTW_F_PDF | RTW_F_ATTR | RTW_F_ENV>;
using RtwSphereClasses = RtwClasses<0u, RTW_F_CHECKER>;
// The classes of the first-hit kernels -- the guide buffers (rtw_denoise.hip) and the ray queries (rtw_query.hip),
// where nothing scatters (RTW_F_PDF is irrelevant): every feature but the media (object_leaf gives a medium leaf
// no hit: a medium hit needs a path's RNG key), with the instance trees, with the vertex attributes.
constexpr uint32_t kRtwFirstHitBase = RTW_F_ALL & ~RTW_F_MEDIUM;
using RtwFirstHitClasses =
    RtwClasses<kRtwFirstHitBase, kRtwFirstHitBase | RTW_F_TREE, kRtwFirstHitBase | RTW_F_TREE | RTW_F_ATTR>;
inline uint32_t rtw_first_hit_class(const rtw_launch& L) {
    const uint32_t f = rtw_feat_of(L);
    if (f & RTW_F_ATTR) return kRtwFirstHitBase | RTW_F_TREE | RTW_F_ATTR;
    return (f & RTW_F_TREE) ? (kRtwFirstHitBase | RTW_F_TREE) : kRtwFirstHitBase;
}
// The guide kernels' classes (rtw_denoise.hip): the first-hit ones, and with an environment registered -- a miss's
// albedo is its radiance -- those with the trees [and the attributes] | RTW_F_ENV.  (The ray queries keep
// RtwFirstHitClasses: an environment is no hit.)
using RtwGuideEnvClasses =
    RtwClasses<kRtwFirstHitBase | RTW_F_TREE | RTW_F_ENV, kRtwFirstHitBase | RTW_F_TREE | RTW_F_ATTR | RTW_F_ENV>;
inline uint32_t rtw_guide_class(const rtw_launch& L) {
    const uint32_t f = rtw_feat_of(L);
    if (f & RTW_F_ENV) return kRtwFirstHitBase | RTW_F_TREE | RTW_F_ENV | (f & RTW_F_ATTR);
    return rtw_first_hit_class(L);
}
// Calls f with the class of the features `feat` (rtw_feat_of): one of the eight object classes, or with SPHERES
// (the persistent kernel) also one of the two sphere-scene classes, which the other kernels run as RTW_F_ALL.
template <bool SPHERES, typename F>
void rtw_with_class(uint32_t feat, F&& f) {
    const uint32_t c = rtw_pick_feat(SPHERES ? feat : feat | RTW_F_ALL);
    if constexpr (SPHERES) {
        if (RtwSphereClasses::visit(c, f)) return;
    }
    (void)RtwObjectClasses::visit(c, f);
}
// ... and with a runtime bool as a std::bool_constant (the persistent kernel's LDS stage)
template <typename F>
void rtw_with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
int rtw_persistent_grid(uint32_t feat, uint32_t n_nodes, bool use_lds);

void rtw_launch_render(const rtw_launch& L, void* stream, int variant, int grid);
void rtw_set_error(const char* msg);  // the thread's rtw_last_error() message (rtw_host.hip)
// Checks the render entry points of rtw_host.hip and rtw_multi.hip share (they set the error message): the camera
// is non-null and initialised, its image addressable and its strata within RTW_MAX_STRATA; the host-buffer entry points' options hold stop / progress
// and spp_batch only.  And the automatic batch: samples per launch of `pixels` pixels, at most spp.
struct rtw_ctx;
int rtw_validate_cam(const rtw_camera* cam);
struct rtw_launch;
void rtw_launch_camera(rtw_launch& L, const rtw_camera* c, uint64_t seed);  // the camera's fields and the key
int rtw_check_host_opts(const rtw_render_opts* o);
uint32_t rtw_auto_batch(const rtw_ctx* ctx, uint64_t pixels, uint32_t spp);
// A device buffer that grows on demand: replaces *buf (after the work on `s` that may still use it) by a fresh
// allocation of `bytes` and sets *size -- the caller's measure of it -- to new_size.  If the allocation fails *buf
// is null and *size 0; the caller clears or reports the error.
template <typename T, typename N>
hipError_t rtw_device_grow(T** buf, N* size, N new_size, size_t bytes, hipStream_t s) {
    if (*buf) {
        if (const hipError_t e = hipStreamSynchronize(s)) return e;
        (void)hipFree(*buf);
    }
    *buf = nullptr;
    *size = 0;
    if (const hipError_t e = hipMalloc(reinterpret_cast<void**>(buf), bytes)) return e;
    *size = new_size;
    return hipSuccess;
}
// ABI-5 stop flags of rtw_render_opts: RenderThread.running (a Zig bool, 0 = stop) or cancel (non-zero = stop)
inline bool rtw_stop_requested(const rtw_render_opts* o) {
    return o && ((o->running && *o->running == 0) || (o->cancel && *o->cancel != 0));
}
// does the caller poll between batches (stop flags or progress)?
inline bool rtw_polled(const rtw_render_opts* o) { return o && (o->running || o->cancel || o->progress); }

// host backend (rtw_cpu.hip): samples [L.s0, L.s1) of the logical pixels [begin, end) onto host float4 `out`.
// Plain launches (L.n_shards == 0): logical pixel = image pixel, out = the frame.  Shard launches: logical
// pixel r * W + x of the shard's tile (image row rtw_tile_row_image(L.rpb, L.n_shards, L.shard, r)), out =
// the tile.  `stop` (may be null) is polled per pixel, as Camera.render polls `running` (camera.zig:107).
int rtw_cpu_render(const rtw_launch& L, uint32_t begin, uint32_t end, float* out, uint32_t threads,
                   const rtw_render_opts* stop);
void rtw_launch_debug_rng(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, float* d_out, void* stream);
void rtw_launch_debug_sample(const rtw_launch& L, uint32_t pixel, uint32_t sample, float* d_out, void* stream);

// Per-kernel HIP-event timing of one render call (rtw_render_opts.timing).
struct rtw_timer {
    struct rec {
        int kind;
        hipEvent_t a, b;
    };
    std::vector<rec> recs;
    std::vector<hipEvent_t> pool;
    hipStream_t stream = nullptr;
    int cur = -1;
    hipEvent_t ev() {
        hipEvent_t e = nullptr;
        if (!pool.empty()) {
            e = pool.back();
            pool.pop_back();
        } else {
            (void)hipEventCreate(&e);
        }
        return e;
    }
    void begin(int kind) {
        recs.push_back({kind, ev(), nullptr});
        (void)hipEventRecord(recs.back().a, stream);
    }
    void end() {
        recs.back().b = ev();
        (void)hipEventRecord(recs.back().b, stream);
    }
};
// begin/end a timed launch when a timer is attached
#define RTW_TIME_BEGIN(T, kind) \
    if (T) (T)->begin(kind);
#define RTW_TIME_END(T) \
    if (T) (T)->end();

// Host copies of the device geometry arrays besides the nodes (rtw_layout.h records).
struct rtw_geometry {
    std::vector<float> cvec;                 // float4 per sphere: center_vec (moving spheres)
    std::vector<rtw_dev_sphere> spheres;     // every sphere
    std::vector<rtw_dev_quad> quads;
    std::vector<rtw_dev_instance> insts;
    std::vector<uint32_t> members;           // RTW_REF
    std::vector<rtw_dev_medium> media;
    uint32_t feat = 0;                       // RTW_F_GEOM | RTW_F_MEDIUM | RTW_F_TREE as present
    std::vector<rtw_node> inodes;            // the instance trees (rtw_dev_instance.tree = first node + 1)
};

// Quad.init (objects.zig:201-210): the device record of a quad description -- normal = unitVector(cross(u, v)),
// d = dot(normal, q), w = n / dot(n, n); the shape is the top bit of mat (rtw_layout.h).  One definition for the
// scene builder (rtw_bvh.hip) and rtw_debug_quad_hit (rtw_cpu.hip).
inline void rtw_quad_init(const rtw_quad& q, rtw_dev_quad& o) {
    float n[3], nn[3];
    n[0] = q.u[1] * q.v[2] - q.u[2] * q.v[1];
    n[1] = q.u[2] * q.v[0] - q.u[0] * q.v[2];
    n[2] = q.u[0] * q.v[1] - q.u[1] * q.v[0];
    const float len = __builtin_sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (int k = 0; k < 3; k++) nn[k] = n[k] / len;
    const float nd = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    o = rtw_dev_quad{};
    o.d = nn[0] * q.q[0] + nn[1] * q.q[1] + nn[2] * q.q[2];
    for (int k = 0; k < 3; k++) {
        o.q[k] = q.q[k];
        o.n[k] = nn[k];
        o.u[k] = q.u[k];
        o.v[k] = q.v[k];
        o.w[k] = n[k] / nd;
    }
    o.mat = q.material | (q.shape == RTW_QUAD_TRIANGLE ? RTW_QUAD_TRI_BIT : 0u);
}

// The stored form of a vertex attribute's normals (rtw_scene_set_vertex_attrs and rtw_debug_quad_shade): each
// divided by its fp32 length sqrt((x x + y y) + z z).  False: a normal is not finite or has zero length.
inline bool rtw_vattr_normalise(const rtw_vertex_attr& a, rtw_vertex_attr& o) {
    for (int c = 0; c < 3; c++) {
        const float x = a.normal[c][0], y = a.normal[c][1], z = a.normal[c][2];
        const float len = __builtin_sqrtf(x * x + y * y + z * z);
        if (!(len > 0.0f) || !(len <= 3.4028234e38f)) return false;
        o.normal[c][0] = x / len;
        o.normal[c][1] = y / len;
        o.normal[c][2] = z / len;
    }
    return true;
}

// Validates the object graph, derives the geometry records and builds the BVH
// over world_objects.  box_pad/extent (out, may be null): SAH trees pad every
// inner box by extent * 2^-19 so the FMA slab test (box_next) stays conservative.
// SAH trees: `orders` (1 or 8) pre-order arrays, one per ray-direction octant when 8
// (concatenated; node indices and skip links are relative to each array).
// 16-B node of the compact walk (rtw_bvh.hip rtw_compact_nodes)
struct rtw_cnode {
    uint32_t v[4];
};
// false: the tree cannot be encoded (coordinates beyond fp16 range, non-finite radius).
// fp32 (4 copies only): 32-B nodes with fp32 boxes instead (2 rtw_cnode per node; rtw_compact_nodes)
bool rtw_compact_nodes(const std::vector<rtw_node>& nodes, uint32_t orders, std::vector<rtw_cnode>& out,
                       bool fp32 = false);

// two-wide 32-B records (2 x rtw_cnode per inner node) of ordering 0 for the stack walk of large static
// sphere SAH trees (rtw_bvh.hip rtw_wide2_nodes); false: not encodable (leaf runs, fp16 range)
bool rtw_wide2_nodes(const std::vector<rtw_node>& nodes, uint32_t n_per, std::vector<rtw_cnode>& out,
                     std::vector<uint32_t>& leaf_id, uint32_t* max_stack);

// hoist (SAH sphere scenes): emit spheres whose box dwarfs the rest ahead of the tree (*n_hoisted of them)
// flatten_pct (SAH trees): inner nodes with >= that % of the area of the node above are not emitted
// (0 = off; SahBuilder::emit_tree)
int rtw_build_bvh(const rtw_scene_desc& desc, std::vector<rtw_node>& nodes, rtw_geometry& geom,
                  uint32_t* depth, uint32_t* axis_draws, float* box_pad = nullptr, float* extent = nullptr,
                  uint32_t orders = 1, uint32_t sah_max_leaf = 1, uint32_t hoist = 0, uint32_t* n_hoisted = nullptr,
                  uint32_t flatten_pct = 0);

// One scene on one device (the opaque rtw_ctx of include/rtw_gpu.h).
struct rtw_ctx {
    int device = 0;                // RTW_DEVICE_CPU: a host context (rtw_cpu.hip)
    std::vector<uint8_t> host_blob;  // host context: the scene image the launch pointers address
    hipStream_t stream = nullptr;
    void* d_blob = nullptr;        // single allocation holding every scene array
    size_t blob_bytes = 0;
    rtw_launch base{};
    rtw_scene_stats stats{};
    std::vector<rtw_node> nodes_host;
    std::vector<rtw_node> inodes_host;       // the instance trees, and per instance (first node, node count)
    std::vector<std::pair<uint32_t, uint32_t>> inst_tree;
    float* d_scratch = nullptr;    // host-API accum staging (rtw_render_ex: the callers' chunks of one frame)
    size_t scratch_bytes = 0;
    float* d_rows = nullptr;       // rtw_render_rows' tile staging (its own: render_ex chunks may be staged
    size_t rows_bytes = 0;         //   in d_scratch while it runs)
    float* d_dbg = nullptr;        // debug kernels output
    uint32_t* d_work = nullptr;    // persistent-kernel work counter (zeroed before each launch)
    uint32_t feat = 0;             // RTW_F_* scene features
    int grid = 0;                  // resident blocks of the persistent kernel
    int variant = 2;               // 2 = wavefront v2 (default), 1 = persistent v1, 0 = simple v0 (rtw_tuning.kernel)
    void* d_tl = nullptr;          // camera-ray tile candidate lists (rtw_wavefront.h), tl_cap tiles
    uint64_t tl_cap = 0;
    void* d_wf = nullptr;          // wavefront path state (rtw_wavefront.h), wf_cap paths
    uint64_t wf_cap = 0;
    uint32_t* wf_len = nullptr;    // the last batch's stripe counters (3 sets) and capacity: rtw_debug_stripe_counters
    uint32_t wf_stripe_cap = 0;
    uint64_t wf_max_paths = 1u << 26;  // paths per wavefront batch (x RTW_WF_PATH_BYTES); set at scene creation
    uint32_t wf_iters = 9;         // wavefront bounces before the tail kernel (rtw_tuning.wf_iters)
    uint32_t wf_sort_mask = 15;    // their bucket key bits (rtw_tuning.sort_bits)
    uint32_t wf_sort_iters_split = 1;  // the same for the split kernels (rtw_tuning.sort_iters_split)
    uint32_t wf_sort_iters = 3;    // iterations whose survivors are filed by direction (rtw_tuning.sort_iters)
    uint32_t cpu_threads = 0;      // host context: worker threads (rtw_tuning.cpu_threads; 0 = all)
    uint32_t wf_deal = 0;          // iteration 0's runs dealt dynamically (rtw_tuning.deal)
    int n_cu = 256;                // compute units of the device (wavefront grids)
    std::vector<hipEvent_t> ev_pool;  // recycled timing events
    uint64_t scene_hash = 0;       // FNV-1a 64 of the uploaded scene image
    // light importance sampling (rtw_scene_set_lights): the registered list, what validates it (host copies
    // of the quads and spheres, the instance member and medium boundary references, the materials' kinds) and the
    // device records (GPU context: d_lights, RTW_MAX_LIGHTS records; host context: lights_rec itself)
    std::vector<rtw_object> lights;
    std::vector<rtw_dev_light> lights_rec;
    rtw_dev_light* d_lights = nullptr;
    std::vector<rtw_dev_quad> quads_host;
    std::vector<rtw_dev_sphere> spheres_host;
    std::vector<uint32_t> members_host, boundaries_host, mat_kind_host;
    // vertex attributes (rtw_scene_set_vertex_attrs): the registered entries as given back by
    // rtw_scene_vertex_attrs_get (normals normalised), the dense records parallel to quads_host (host context:
    // base.vattrs addresses them) and their device copy (GPU context; allocated at the first registration)
    std::vector<uint32_t> vattr_quads;
    std::vector<rtw_vertex_attr> vattr_set;
    std::vector<rtw_dev_vattr> vattrs_rec;
    rtw_dev_vattr* d_vattrs = nullptr;
    // environment map (rtw_scene_set_environment): the block of rtw_layout.h's rtw_dev_env with host addresses
    // (base's env words address it on a host context; rtw_debug_environment and the getter read it on both kinds)
    // and its device copy (GPU context: one allocation per registration, freed at the next), the caller's record
    // and map as given, and their digest (0: none; rtw_scene_hash, rtw_multi_create)
    std::vector<float4> env_block;
    void* d_env = nullptr;
    rtw_environment env_given{};
    std::vector<float> env_rgb;
    uint64_t env_hash = 0;
    float box_pad = 0;             // absolute pad baked into the inner boxes (SAH trees), 0 = none
    float extent = 0;              // max |coordinate| over the scene's boxes
    // Concurrent callers (the reference's 8 RenderThreads call Camera.render at once, main.zig:314-326):
    // one caller at a time enqueues work on a context -- the wavefront state and staging buffers are per
    // context -- and work on another stream than the previous enqueue's waits for that work on the
    // device.  The host-buffer API (rtw_render_ex) holds the lock only while it enqueues one spp batch,
    // so the 8 Tasks' batches interleave; host_calls counts its calls with a chunk staged in d_scratch.
    std::mutex mu;
    std::condition_variable host_cv;
    int host_calls = 0;
    std::atomic<uint32_t> cpu_calls{0};  // host context: calls rendering now (they share cpu_threads)
    hipEvent_t last_done = nullptr;
    hipStream_t last_stream = nullptr;
    // the denoiser's two ping-pong images (rtw_denoise.hip), dn_cap pixels each: device float4 planes of a GPU
    // context, grown on demand under the lock; a host context keeps them in dn_host
    float4* d_dn[2] = {nullptr, nullptr};
    uint64_t dn_cap = 0;
    std::vector<float4> dn_host[2];
    // the guided filter's two variance planes (one float per pixel) beside them, grown the same way
    float* d_dnv[2] = {nullptr, nullptr};
    uint64_t dnv_cap = 0;
    std::vector<float> dnv_host[2];
};
// What the entry points of rtw_denoise.hip share with the render entry points (rtw_host.hip; the caller holds
// ctx->mu): the launch of a camera on a context, and the stream ordering of consecutive calls on it
rtw_launch rtw_make_launch(const rtw_ctx* ctx, const rtw_camera* c, uint64_t seed);
int rtw_stream_enter(rtw_ctx* ctx, hipStream_t s);
int rtw_stream_leave(rtw_ctx* ctx, hipStream_t s);

// The error helpers of every host file: a failed HIP call sets the thread's message and returns RTW_E_OOM /
// RTW_E_HIP (rtw_host.hip), a refused argument sets it and returns RTW_E_INVALID.
int rtw_hip_fail(hipError_t e, const char* where);
inline int rtw_invalid(const char* msg) {
    rtw_set_error(msg);
    return RTW_E_INVALID;
}
#define HIP_TRY(expr)                                         \
    do {                                                      \
        hipError_t _e = (expr);                               \
        if (_e != hipSuccess) return rtw_hip_fail(_e, #expr); \
    } while (0)

// The host backend's thread pool: [0, n) in contiguous chunks [n t / T, n (t + 1) / T) -- startRender's Tasks
// (main.zig:318-324) -- on T host threads, T = threads (0: all the machine's) but at most max(1, n / min_chunk); the
// calling thread takes chunk 0.  f(begin, end) runs once per chunk.  (n < 2^32: n * T stays in 64 bits.)
template <typename F>
void rtw_host_ranges(uint64_t n, uint32_t threads, uint64_t min_chunk, F&& f) {
    if (threads == 0) threads = std::max(1u, std::thread::hardware_concurrency());
    threads = (uint32_t)std::min<uint64_t>(threads, std::max<uint64_t>(1, n / min_chunk));
    auto work = [&](uint32_t t) { f(n * t / threads, n * (t + 1) / threads); };
    std::vector<std::thread> pool;
    pool.reserve(threads);
    for (uint32_t t = 1; t < threads; t++) pool.emplace_back(work, t);
    work(0);
    for (std::thread& th : pool) th.join();
}
