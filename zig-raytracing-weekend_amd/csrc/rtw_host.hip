// rtw_host.hip -- C ABI implementation (include/rtw_gpu.h): scene upload,
// Camera.init, batched launches with cancel/progress, sharded row rendering.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rtw_gpu.h"
#include "rtw_internal.h"
#include "rtw_layout.h"
#include "rtw_rng.h"
#include "rtw_wavefront.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* msg) {
    g_err = msg;
    return code;
}

}  // namespace

int rtw_hip_fail(hipError_t e, const char* where) {
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? RTW_E_OOM : RTW_E_HIP;
}

void rtw_set_error(const char* msg) { g_err = msg ? msg : ""; }

// struct rtw_ctx: see rtw_internal.h

namespace {
// the material kinds that read a texture
bool textured(const rtw_material& m) {
    return m.kind == RTW_MAT_LAMBERTIAN || m.kind == RTW_MAT_DIFFUSE_LIGHT || m.kind == RTW_MAT_ISOTROPIC;
}

uint32_t scene_features(const rtw_scene_desc* d) {
    uint32_t f = 0;
    for (uint32_t i = 0; i < d->n_spheres; i++)
        if (d->spheres[i].is_moving) f |= RTW_F_MOVING;
    for (uint32_t i = 0; i < d->n_materials; i++) {
        const rtw_material& m = d->materials[i];
        if (m.kind == RTW_MAT_DIFFUSE_LIGHT || m.kind == RTW_MAT_ISOTROPIC) f |= RTW_F_LIGHT;
        if (!textured(m)) continue;
        const uint32_t k = d->textures[m.texture].kind;
        if (k == RTW_TEX_CHECKER) f |= RTW_F_CHECKER;
        if (k == RTW_TEX_IMAGE) f |= RTW_F_IMAGE;
        if (k == RTW_TEX_NOISE) f |= RTW_F_NOISE;
    }
    return f;
}

// ---- scene creation (rtw_scene_create_ex), step by step ----

int check_tuning(const rtw_tuning& tu) {
    if (tu.kernel > RTW_KERNEL_SIMPLE) return fail(RTW_E_INVALID, "tuning.kernel out of range");
    if (tu.bvh_orders != 0 && tu.bvh_orders != 1 && tu.bvh_orders != 4 && tu.bvh_orders != 8)
        return fail(RTW_E_INVALID, "tuning.bvh_orders must be 0, 1, 4 or 8");
    if (tu.clds_shape != 0 && tu.clds_shape != 1 && tu.clds_shape != 4)
        return fail(RTW_E_INVALID, "tuning.clds_shape must be 0, 1 or 4 (ABI 8)");
    if (tu.deal & ~(uint32_t)RTW_DEAL_ALL)
        return fail(RTW_E_INVALID, "tuning.deal: bits 1 | 2 | 8 | 16 | 32 | 128 (RTW_DEAL_*)");
    if (tu.wf_iters > RTW_WF_MAX_ITERS) return fail(RTW_E_INVALID, "tuning.wf_iters out of range");
    if ((tu.object_tree & 0xFFu) > 100 || (tu.object_tree & ~(0xFFu | RTW_OTREE_NO_CULL)))
        return fail(RTW_E_INVALID, "tuning.object_tree: 0..100 [| RTW_OTREE_NO_CULL]");
    if (tu.sort_bits > RTW_WF_BUCKET_BITS) return fail(RTW_E_INVALID, "tuning.sort_bits out of range");
    if (tu.mega_shade_min < 1 || tu.mega_shade_min > 64)
        return fail(RTW_E_INVALID, "tuning.mega_shade_min out of range");
    if (tu.mega_waves != 1 && tu.mega_waves != 6 && tu.mega_waves != 8)
        return fail(RTW_E_INVALID, "tuning.mega_waves must be 1, 6 or 8");
    if (tu.wf_paths && tu.wf_paths < 4096) return fail(RTW_E_INVALID, "tuning.wf_paths must be 0 or >= 4096");
    return RTW_OK;
}

// the description lists something to render (rtw_scene_create_ex, rtw_scene_flatten)
bool has_objects(const rtw_scene_desc* d) {
    return !(d->n_spheres && !d->spheres) && (d->objects ? d->n_objects : d->n_spheres) != 0;
}

int check_desc(const rtw_scene_desc* d) {
    if (!has_objects(d)) return fail(RTW_E_INVALID, "scene has no objects");
    if (d->n_materials == 0 || !d->materials) return fail(RTW_E_INVALID, "scene has no materials");
    for (uint32_t i = 0; i < d->n_spheres; i++)
        if (d->spheres[i].material >= d->n_materials) return fail(RTW_E_INVALID, "sphere material index out of range");
    for (uint32_t i = 0; i < d->n_materials; i++) {
        const rtw_material& m = d->materials[i];
        if (m.kind > RTW_MAT_ISOTROPIC) return fail(RTW_E_INVALID, "unknown material kind");
        if (textured(m) && m.texture >= d->n_textures)
            return fail(RTW_E_INVALID, "material texture index out of range");
    }
    for (uint32_t i = 0; i < d->n_textures; i++) {
        const rtw_texture& t = d->textures[i];
        if (t.kind > RTW_TEX_NOISE) return fail(RTW_E_INVALID, "unknown texture kind");
        if (t.kind == RTW_TEX_IMAGE && t.image >= d->n_images)
            return fail(RTW_E_INVALID, "texture image index out of range");
        if (t.kind == RTW_TEX_NOISE && t.perlin >= d->n_perlins)
            return fail(RTW_E_INVALID, "texture perlin index out of range");
    }
    for (uint32_t i = 0; d->quads && i < d->n_quads; i++)
        if (d->quads[i].shape > RTW_QUAD_TRIANGLE) {
            char msg[160];
            std::snprintf(msg, sizeof msg, "quad %u: unknown shape %u (RTW_QUAD_PARALLELOGRAM = 0 or "
                          "RTW_QUAD_TRIANGLE = 1)", i, d->quads[i].shape);
            return fail(RTW_E_INVALID, msg);
        }
    for (uint32_t i = 0; i < d->n_images; i++) {
        const rtw_image& im = d->images[i];
        if (im.width && im.height && (!im.data || im.bytes_per_row < 4 * im.width))
            return fail(RTW_E_INVALID, "bad image");
    }
    return RTW_OK;
}

// SAH trees of sphere scenes: 8 octant-ordered copies of the node array (tuning.bvh_orders 4: copies by the
// x and z signs; 1: one, ordered along order_dir).  Scenes with quads/instances/media keep one order: their leaf
// tests are costly, and lanes walking different orders stop executing them together (Cornell: -31 % with 8 orders).
uint32_t choose_orders(const rtw_scene_desc* d, const rtw_tuning& tu, uint32_t sfeat, bool objects) {
    uint32_t orders = (d->bvh_mode == RTW_BVH_SAH && !objects) ? 8u : 1u;
    // Round 5: small static untextured sphere trees (Book-1, C2 / C3) take 4 copies (x, z signs): their compact
    // stage (+ materials) then fits half the LDS and the fused step and tail run two 768-thread blocks per CU, 6
    // waves per SIMD (C2 +4.6 %, profiles/r5_stage/).  (A tree of ~2 nodes per sphere; the check is redone on the
    // built tree by the launcher, which falls back to one block.)
    const size_t mat_b = (size_t)d->n_materials * sizeof(rtw_dev_material);
    if (orders == 8 && !tu.bvh_orders && tu.compact_nodes == 1 && tu.fast_box && !(sfeat & ~RTW_F_CHECKER) &&
        (2 * (size_t)d->n_spheres + 8) * 4 * 16 + mat_b + RTW_WF_CURSOR_BYTES(768u) <= RTW_WF_CLDS2_MAX)
        orders = 4;
    // (object scenes keep one ordering: their hit ids carry an instance member where sphere scenes carry the copy)
    if (tu.bvh_orders) orders = (d->bvh_mode == RTW_BVH_SAH && !objects && tu.bvh_orders > 1) ? tu.bvh_orders : 1u;
    return orders;
}

// The hit id is one 32-bit word, -1 = miss: leaf node | instance member << bits.  Without instance trees
// the split is fixed (24 node bits, 7 member bits: lists of at most 127).  With them (RTW_F_TREE) it is
// per scene: as many bits as the world tree's nodes need, the rest up to bit 30 for the member.
int split_hit_id(const rtw_geometry& geom, size_t nodes, uint32_t* hit_bits) {
    *hit_bits = RTW_HIT_NODE_BITS;
    if (geom.feat & RTW_F_TREE) {
        auto bits = [](uint64_t max_value) {
            uint32_t b = 1;
            while (b < 32 && (max_value >> b)) b++;
            return b;
        };
        uint32_t max_count = 1;
        for (const rtw_dev_instance& in : geom.insts) max_count = std::max(max_count, in.count);
        const uint32_t nb = bits(nodes - 1), mb = bits(max_count - 1);
        if (nb + mb > 31) {
            char msg[200];
            std::snprintf(msg, sizeof msg,
                          "hit id limit: %zu BVH nodes (%u bits) and an instance of %u members (%u bits) need more "
                          "than 31 bits together", nodes, nb, max_count, mb);
            return fail(RTW_E_INVALID, msg);
        }
        *hit_bits = nb;
    } else if ((geom.feat & RTW_F_GEOM) && nodes >= (1u << RTW_HIT_NODE_BITS)) {
        return fail(RTW_E_INVALID, "scenes with instances are limited to 2^24 BVH nodes");
    }
    return RTW_OK;
}

// The walks' derived records of a GPU context's static sphere SAH tree (empty where they do not apply)
struct WalkRecords {
    std::vector<rtw_cnode> cnodes;  // compact 16-B walk (rtw_compact_nodes), or with cnode32 the 32-B fp32-box form
    bool cnode32 = false;
    std::vector<rtw_cnode> w2;      // two-wide records for the stack walk of trees read through L1/L2 (rtw_wide2_nodes)
    std::vector<uint32_t> w2leaf;
    uint32_t w2_stack = 0;
};
void build_walk_records(const rtw_scene_desc* d, const rtw_tuning& tu, const rtw_ctx* ctx, uint32_t orders,
                        bool objects, WalkRecords& R) {
    const std::vector<rtw_node>& nodes = ctx->nodes_host;
    bool want = d->bvh_mode == RTW_BVH_SAH && !objects && ctx->box_pad > 0 && tu.compact_nodes &&
                ctx->device != RTW_DEVICE_CPU;
    for (uint32_t i = 0; want && i < d->n_spheres; i++) want = !d->spheres[i].is_moving;
    // compact_nodes 2: the 32-B fp32-box form where it applies (4 copies), else the 16-B fp16 form
    R.cnode32 = want && tu.compact_nodes == 2 && orders == 4 && rtw_compact_nodes(nodes, orders, R.cnodes, true);
    if (want && !R.cnode32 && !rtw_compact_nodes(nodes, orders, R.cnodes)) R.cnodes.clear();
    if (!R.cnodes.empty() && !R.cnode32 && tu.wide_walk && tu.sah_max_leaf <= 1 &&
        !rtw_wide2_nodes(nodes, (uint32_t)(nodes.size() / orders), R.w2, R.w2leaf, &R.w2_stack))
        R.w2.clear();
    if (R.w2_stack > RTW_W2_STACK_MAX) R.w2.clear();
}

// The device records of the description's materials, textures (one more, zero), Perlin tables (one more) and
// images (each 256-B aligned in `bytes`; one more info record)
std::vector<rtw_dev_material> dev_materials(const rtw_scene_desc* d) {
    std::vector<rtw_dev_material> out(d->n_materials);
    for (uint32_t i = 0; i < d->n_materials; i++) {
        rtw_dev_material& m = out[i];
        m.kind = d->materials[i].kind;
        m.texture = d->materials[i].texture;
        m.fuzz = d->materials[i].fuzz;
        m.ir = d->materials[i].ir;
        for (int k = 0; k < 3; k++) m.albedo[k] = d->materials[i].albedo[k];
    }
    return out;
}
std::vector<rtw_dev_texture> dev_textures(const rtw_scene_desc* d) {
    std::vector<rtw_dev_texture> out(d->n_textures + 1);
    for (uint32_t i = 0; i < d->n_textures; i++) {
        rtw_dev_texture& t = out[i];
        const rtw_texture& s = d->textures[i];
        t.kind = s.kind; t.image = s.image; t.perlin = s.perlin; t.scale = s.scale;
        for (int k = 0; k < 3; k++) { t.even[k] = s.even[k]; t.odd[k] = s.odd[k]; }
    }
    return out;
}
std::vector<uint8_t> dev_perlins(const rtw_scene_desc* d) {
    std::vector<uint8_t> out((size_t)(d->n_perlins + 1) * RTW_PERLIN_BYTES, 0);
    for (uint32_t i = 0; i < d->n_perlins; i++) {
        uint8_t* base = out.data() + (size_t)i * RTW_PERLIN_BYTES;
        float* vec = reinterpret_cast<float*>(base);
        for (int k = 0; k < 256; k++) {
            vec[4 * k + 0] = d->perlins[i].ranvec[k][0];
            vec[4 * k + 1] = d->perlins[i].ranvec[k][1];
            vec[4 * k + 2] = d->perlins[i].ranvec[k][2];
            vec[4 * k + 3] = 0.0f;
        }
        uint32_t* perm = reinterpret_cast<uint32_t*>(base + 256 * 16);
        for (int k = 0; k < 256; k++) {
            perm[k] = d->perlins[i].perm_x[k];
            perm[256 + k] = d->perlins[i].perm_y[k];
            perm[512 + k] = d->perlins[i].perm_z[k];
        }
    }
    return out;
}
void dev_images(const rtw_scene_desc* d, std::vector<rtw_dev_image>& info, std::vector<uint8_t>& bytes) {
    info.assign(d->n_images + 1, rtw_dev_image{});
    size_t total = 0;
    for (uint32_t i = 0; i < d->n_images; i++) {
        info[i].offset = total;
        info[i].width = d->images[i].width;
        info[i].height = d->images[i].height;
        info[i].bytes_per_row = d->images[i].bytes_per_row;
        total += ((size_t)d->images[i].bytes_per_row * d->images[i].height + 255) & ~size_t(255);
    }
    bytes.assign(total, 0);
    for (uint32_t i = 0; i < d->n_images; i++) {
        const size_t nb = (size_t)d->images[i].bytes_per_row * d->images[i].height;
        if (nb) std::memcpy(bytes.data() + info[i].offset, d->images[i].data, nb);
    }
}

// Everything the scene blob is made of besides the world tree (ctx->nodes_host)
struct SceneParts {
    rtw_geometry geom;
    WalkRecords walk;
    std::vector<rtw_dev_material> mats;
    std::vector<rtw_dev_texture> texs;
    std::vector<rtw_dev_image> img_info;
    std::vector<uint8_t> perlin, images;
};

// One section of the scene blob: `bytes` copied from src, `pad` more reserved behind them (zero), the sum rounded
// up to 256 B; `present` false: the section's launch pointer is null (its bytes, if any, are laid out all the same)
struct Section {
    const void* src;
    size_t bytes, pad;
    bool present;
    size_t off;
};
template <typename T>
Section section(const std::vector<T>& v, size_t pad = 0, bool present = true) {
    return Section{v.data(), v.size() * sizeof(T), pad, present, 0};
}
// Blob layout, in this order: nodes | cvec | spheres | quads | members | instances | media | materials | textures |
// images-info | perlin | image bytes || compact nodes | two-wide records | their leaf ids | instance trees.
// The scene image that rtw_scene_hash covers is [S_CVEC, S_CNOD): the walks' derived records behind it depend on
// the backend and the tuning, so a checkpoint's hash matches on every context of the same scene (the node array,
// whose layout also follows the tuning, is left out of the hash as well).
enum { S_NODES, S_CVEC, S_SPH, S_QUAD, S_MEMB, S_INST, S_MED, S_MATS, S_TEXS, S_IMGI, S_PERL, S_IMGS, S_CNOD, S_W2,
       S_W2L, S_INOD, S_COUNT };
struct Blob {
    Section s[S_COUNT];
    size_t bytes;
    template <typename T>
    const T* at(const uint8_t* base, int k) const {
        return s[k].present ? reinterpret_cast<const T*>(base + s[k].off) : nullptr;
    }
};
Blob lay_out_blob(const rtw_ctx* ctx, const SceneParts& P) {
    const rtw_geometry& g = P.geom;
    const bool w2 = !P.walk.w2.empty();
    Blob B{{section(ctx->nodes_host), section(g.cvec, 16), section(g.spheres, 16), section(g.quads, 16),
            section(g.members, 16), section(g.insts, 16), section(g.media, 16), section(P.mats), section(P.texs),
            section(P.img_info), section(P.perlin), section(P.images, 16),
            section(P.walk.cnodes, 0, !P.walk.cnodes.empty()), section(P.walk.w2, 0, w2),
            section(P.walk.w2leaf, 0, w2), section(g.inodes, 0, !g.inodes.empty())},
           0};
    for (Section& x : B.s) {
        x.off = B.bytes;
        B.bytes = (B.bytes + x.bytes + x.pad + 255) & ~size_t(255);
    }
    return B;
}
std::vector<uint8_t> fill_blob(const Blob& B) {
    std::vector<uint8_t> blob(B.bytes, 0);
    for (const Section& x : B.s)
        if (x.bytes) std::memcpy(blob.data() + x.off, x.src, x.bytes);
    return blob;
}

// FNV-1a 64 of the scene image (rtw_scene_hash): the tree kind (and the reference topology's seed),
// then every section after the nodes -- the node array's layout depends on the tuning (orderings,
// hoisting, object_tree), the image does not
uint64_t hash_blob(const rtw_scene_desc* d, const std::vector<uint8_t>& blob, const Blob& B) {
    uint64_t h = 0xCBF29CE484222325ull;
    const uint64_t key[2] = {(uint64_t)d->bvh_mode, d->bvh_mode == RTW_BVH_REFERENCE ? (uint64_t)d->bvh_seed : 0ull};
    const unsigned char* kb = reinterpret_cast<const unsigned char*>(key);
    for (size_t i = 0; i < sizeof key; i++) h = (h ^ kb[i]) * 0x100000001B3ull;
    for (size_t i = B.s[S_CVEC].off; i < B.s[S_CNOD].off; i++) h = (h ^ blob[i]) * 0x100000001B3ull;
    return h;
}

int upload_blob(rtw_ctx* ctx, const std::vector<uint8_t>& blob) {
    hipError_t e = hipSetDevice(ctx->device);
    // blocking stream: orders with the legacy NULL stream (torch's default), so a caller passing
    // device buffers and stream == NULL sees its prior NULL-stream work (e.g. zero fills) complete first
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamDefault);
    if (e == hipSuccess) e = hipMalloc(&ctx->d_blob, blob.size());
    if (e == hipSuccess) e = hipMemcpy(ctx->d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&ctx->d_dbg, 64 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&ctx->d_work, 256);
    return e == hipSuccess ? RTW_OK : rtw_hip_fail(e, "rtw_scene_create upload");
}

// the launch's scene pointers: the sections of the blob at `base` (the device copy, or a host context's own)
void set_scene_pointers(rtw_launch& L, const uint8_t* base, const Blob& B, const WalkRecords& walk) {
    L.nodes = B.at<float4>(base, S_NODES);
    L.cvec = B.at<float4>(base, S_CVEC);
    L.sph = B.at<rtw_dev_sphere>(base, S_SPH);
    L.quads = B.at<rtw_dev_quad>(base, S_QUAD);
    L.members = B.at<uint32_t>(base, S_MEMB);
    L.insts = B.at<rtw_dev_instance>(base, S_INST);
    L.media = B.at<rtw_dev_medium>(base, S_MED);
    L.mats = B.at<rtw_dev_material>(base, S_MATS);
    L.texs = B.at<rtw_dev_texture>(base, S_TEXS);
    L.img_info = B.at<rtw_dev_image>(base, S_IMGI);
    L.perlin = B.at<float4>(base, S_PERL);
    L.images = B.at<uint8_t>(base, S_IMGS);
    L.cnodes = B.at<uint4>(base, S_CNOD);
    L.w2nodes = B.at<uint4>(base, S_W2);
    L.w2leaf = B.at<uint32_t>(base, S_W2L);
    L.w2_stack = walk.w2.empty() ? 0u : walk.w2_stack;
    L.inodes = B.at<float4>(base, S_INOD);
    L.cnode32 = walk.cnode32 ? 1u : 0u;
    L.n_lights = 0;  // rtw_scene_set_lights
    L.lights = nullptr;
    L.vattrs = nullptr;  // rtw_scene_set_vertex_attrs
}

// the host copies the context keeps: what rtw_scene_set_lights / rtw_scene_set_vertex_attrs validate against and
// what rtw_scene_instance_nodes gives back
void keep_host_copies(rtw_ctx* ctx, const rtw_scene_desc* d, const rtw_geometry& geom) {
    ctx->quads_host = geom.quads;
    ctx->spheres_host = geom.spheres;
    ctx->members_host = geom.members;
    for (const rtw_dev_medium& m : geom.media) ctx->boundaries_host.push_back(m.boundary);
    for (uint32_t i = 0; i < d->n_materials; i++) ctx->mat_kind_host.push_back(d->materials[i].kind);
    ctx->inodes_host = geom.inodes;
    ctx->inst_tree.clear();
    for (const rtw_dev_instance& in : geom.insts)
        ctx->inst_tree.emplace_back(in.tree ? in.tree - 1u : 0u, in.tree ? 2u * in.count - 1u : 0u);
}

void set_stats(rtw_ctx* ctx, const rtw_scene_desc* d, uint32_t orders, uint32_t depth, uint32_t draws,
               uint32_t n_hoisted) {
    rtw_scene_stats& st = ctx->stats;
    st.n_nodes = (uint32_t)(ctx->nodes_host.size() / orders);  // per ordering
    st.n_leaves = d->objects ? d->n_objects : d->n_spheres;
    st.n_inner = st.n_nodes - st.n_leaves;
    st.depth = depth;
    st.device_bytes = ctx->blob_bytes;
    st.axis_draws = draws;
    st.n_hoisted = n_hoisted;
    st.extent = ctx->extent;
    st.box_pad = ctx->box_pad;
}

// the wavefront's batch and iteration knobs, and the device's size
void set_wavefront_knobs(rtw_ctx* ctx, const rtw_tuning& tu, uint32_t sfeat) {
    const bool host = ctx->device == RTW_DEVICE_CPU;
    ctx->wf_deal = tu.deal;
    {
        // wavefront batch capacity: up to 2^29 paths (BASELINE config 2 = 480M samples in one
        // batch: one drain of long paths per render instead of one per 64M), within ~35 % of
        // the device's FREE memory at scene creation (RTW_WF_PATH_BYTES per path); the
        // allocation halves the batch on failure (run_wavefront)
        size_t free_b = 0, total_b = 0;
        uint64_t cap = 1ull << 29;
        if (!host && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b)
            cap = std::min<uint64_t>(cap, (uint64_t)(0.35 * (double)free_b) / RTW_WF_PATH_BYTES);
        ctx->wf_max_paths = tu.wf_paths ? tu.wf_paths : std::max<uint64_t>(cap, 1u << 20);
    }
    // Round 5, with the dynamic tail (deal bit 2): fewer iterations before the tail pay everywhere but on
    // image-textured scenes -- same-box A/B, 9 -> 4 iterations: C2 +3.7 %, C4 +3.3 %, Cornell +6.8 %, smoke
    // +1.2 %, simple_light +1.9 %.  Image-textured scenes run no tail at all (every bounce a wavefront
    // iteration: the launcher clamps to max_depth): C5 9 / 24 / 32 / 50 iterations 9425 / 9750 / 9816 / 9990
    // Msamples/s (profiles/r5_iters/).
    ctx->wf_iters = tu.wf_iters ? tu.wf_iters : (sfeat & RTW_F_IMAGE) ? (uint32_t)RTW_WF_MAX_ITERS : 4u;
    ctx->wf_sort_iters = tu.sort_iters;
    ctx->wf_sort_iters_split = tu.sort_iters_split;
    ctx->wf_sort_mask = (1u << tu.sort_bits) - 1u;
    int n_cu = 0;
    if (host || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess ||
        n_cu < 1)
        n_cu = 256;
    ctx->n_cu = n_cu;
    ctx->cpu_threads = tu.cpu_threads;
}

// the launch's knobs (ctx->base): what the tuning and the built scene make of the kernels' switches
void set_launch_knobs(rtw_ctx* ctx, const rtw_scene_desc* d, const rtw_tuning& tu, uint32_t orders, const Blob& B) {
    rtw_launch& L = ctx->base;
    const uint32_t n_nodes = ctx->stats.n_nodes;  // per ordering
    // default cap: 32 candidates for small trees (flat prepass: C2 16/32/64 -> 5765/5789/5769), 128 for large
    // ones (frustum-walked prepass: C4 32/64 -> 2440/2458; round 6, 64/96/128 -> 3147/3156/3166,
    // profiles/r6_late_rest/)
    L.tile_lists = tu.tile_lists == 1 ? (n_nodes <= 4096 ? 32u : 128u) : std::min<uint32_t>(tu.tile_lists, RTW_TL_MAX);
    L.n_nodes = n_nodes;
    L.n_orders = orders;
    L.clds_shape = tu.clds_shape ? tu.clds_shape : 4u;  // auto: two 768-thread blocks where the stage fits
    L.n_perlin = d->n_perlins;
    L.feat = ctx->feat;
    L.work_counter = ctx->d_work;
    L.shade_min = tu.mega_shade_min;
    L.tile_order = tu.mega_tile_order ? 1u : 0u;
    // (an unfiltered variant measured +-0 on C2 and -20 % on C4: its codegen slowed the L1/L2 walk)
    L.fast_reject = tu.fast_reject ? 1u : 0u;
    // the octant copies do not fit the megakernel's stage
    L.use_lds = orders == 1 && (tu.lds & RTW_LDS_MEGA_NODES) ? 1u : 0u;
    // wavefront trace: node array staged in LDS when one ordering fits (object scenes,
    // reference trees; +2 % on Cornell); the 8 octant copies of SAH sphere trees do not
    L.wf_lds = (tu.lds & RTW_LDS_NODES) ? 1u : 0u;
    // small static sphere SAH trees: the compact nodes of all 8 orders in LDS (C2: +1 %)
    L.wf_clds = (tu.lds & RTW_LDS_CNODES) ? 1u : 0u;
    // compact LDS stage: gen, trace and shade of an iteration fused in one kernel
    // (the ray/hit hand-off through HBM disappears), tail on the LDS stage
    L.wf_fuse = tu.fuse & 7u;
    // Perlin tables (7 KiB each) staged in LDS by the fused step when at most 4 (noise scenes)
    L.perlin_lds = (ctx->feat & RTW_F_NOISE) && d->n_perlins <= 4 && (tu.lds & RTW_LDS_PERLIN) ? 1u : 0u;
    // materials of sphere scenes staged in LDS by the compact-LDS fused step when they fit beside the
    // nodes (wf_run_fused checks the total): hit_prep's material load stops waiting on L1/L2
    const size_t mat_bytes = (d->n_materials * sizeof(rtw_dev_material) + 15) & ~size_t(15);
    L.mat_lds = (tu.lds & RTW_LDS_MATERIALS) ? (uint32_t)mat_bytes : 0u;
    const size_t shade_bytes = B.s[S_PERL].off - B.s[S_MATS].off;
    L.shade_lds = shade_bytes <= 8192 && (tu.lds & RTW_LDS_SHADE) ? (uint32_t)shade_bytes : 0u;
    // quads, instance member lists and instances of small object scenes (Cornell: ~2 KiB) staged in LDS
    // with the node array: the member loop's loads stop waiting on L1
    const size_t geom_bytes = B.s[S_MED].off - B.s[S_QUAD].off;
    const bool geom_fits = (ctx->feat & RTW_F_GEOM) && geom_bytes <= 16384;
    L.geom_lds = geom_fits && (tu.lds & RTW_LDS_GEOMETRY) ? (uint32_t)geom_bytes : 0u;
    // SAH trees: FMA slab test on the padded boxes (only enlarges the set of visited nodes;
    // reference trees keep the exact aabb.zig walk)
    L.fast_box = ctx->box_pad > 0 && tu.fast_box ? 1u : 0u;
    L.inst_cull = (tu.object_tree & RTW_OTREE_NO_CULL) ? 0u : 1u;  // consulted only with fast_box
    if (ctx->device == RTW_DEVICE_CPU) {  // the exact aabb.zig slab test and IEEE sphere test (the hardware
        L.fast_box = 0;                   // estimates are device-only)
        L.fast_reject = 0;
    }
}

struct CtxDestroy {
    void operator()(rtw_ctx* ctx) const { rtw_scene_destroy(ctx); }
};

// The upload-and-publish step of a registration (rtw_scene_set_lights, rtw_scene_set_vertex_attrs; the caller
// holds ctx->mu): the records `rec` become the context's -- `kept` on the host and, on a GPU context, *d_buf,
// allocated for `cap` records at the first registration -- and `ptr`, the field of `base` the kernels read them
// through, addresses them (null: none registered).
template <typename T>
int publish_records(rtw_ctx* ctx, rtw_launch& base, std::vector<T>& kept, const std::vector<T>& rec, T** d_buf,
                    size_t cap, const T*& ptr) {
    const bool host = ctx->device == RTW_DEVICE_CPU;
    if (!host) {
        HIP_TRY(hipSetDevice(ctx->device));
        // a render left on a caller's stream (RTW_RENDER_NO_SYNC) may still read the records
        if (ctx->last_done) HIP_TRY(hipEventSynchronize(ctx->last_done));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (!rec.empty() && !*d_buf) HIP_TRY(hipMalloc(reinterpret_cast<void**>(d_buf), cap * sizeof(T)));
        if (!rec.empty()) HIP_TRY(hipMemcpy(*d_buf, rec.data(), rec.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    kept = rec;
    ptr = rec.empty() ? nullptr : host ? kept.data() : *d_buf;
    // the persistent kernel's resident grid is its instantiation's
    if (!host) ctx->grid = rtw_persistent_grid(rtw_feat_of(base), ctx->stats.n_nodes, base.use_lds != 0);
    return RTW_OK;
}
}  // namespace

extern "C" {

int rtw_version(void) { return RTW_ABI_VERSION; }

const char* rtw_last_error(void) { return g_err.c_str(); }

int rtw_device_count(int* out) {
    if (!out) return fail(RTW_E_INVALID, "null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *out = n;
    return RTW_OK;
}

// Camera.init (src/camera.zig:118-154).  Plain fp32 host arithmetic in the
// Zig expression order; tan is the host libm (the Zig std tan is a musl port).
int rtw_camera_init(const rtw_camera_params* p, rtw_camera* c) {
#pragma STDC FP_CONTRACT OFF
    if (!p || !c) return fail(RTW_E_INVALID, "null camera params");
    if (p->image_width == 0) return fail(RTW_E_INVALID, "image_width == 0");
    std::memset(c, 0, sizeof *c);
    uint32_t H = p->image_height;
    if (H == 0) H = (uint32_t)std::round((float)p->image_width / p->aspect_ratio);
    if (H < 1) H = 1;
    const uint32_t W = p->image_width;
    c->image_width = W;
    c->image_height = H;
    c->size = W * H;
    c->samples_per_pixel = p->samples_per_pixel;
    c->max_depth = p->max_depth;
    c->background_mode = p->background_mode;
    c->pixel_offset = p->pixel_offset;
    for (int k = 0; k < 3; k++) c->background[k] = p->background[k];
    const float pi = 3.1415926535897932385f;
    const float theta = p->vfov * pi / 180.0f;
    const float h = std::tan(theta / 2.0f);
    const float vh = 2 * h * p->focus_dist;
    const float vw = vh * ((float)W / (float)H);
    float w[3], u[3], v[3], tmp[3];
    for (int k = 0; k < 3; k++) tmp[k] = p->lookfrom[k] - p->lookat[k];
    auto unit = [](const float* a, float* o) {
        float l = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int k = 0; k < 3; k++) o[k] = a[k] / l;
    };
    auto cross = [](const float* a, const float* b, float* o) {
        o[0] = a[1] * b[2] - a[2] * b[1];
        o[1] = a[2] * b[0] - a[0] * b[2];
        o[2] = a[0] * b[1] - a[1] * b[0];
    };
    unit(tmp, w);
    cross(p->vup, w, tmp);
    unit(tmp, u);
    cross(w, u, v);
    float vu[3], vv[3];
    for (int k = 0; k < 3; k++) {
        vu[k] = vw * u[k];
        vv[k] = vh * -v[k];
        c->pixel_delta_u[k] = vu[k] / (float)W;
        c->pixel_delta_v[k] = vv[k] / (float)H;
        const float upper_left = ((p->lookfrom[k] - p->focus_dist * w[k]) - vu[k] / 2.0f) - vv[k] / 2.0f;
        c->pixel00_loc[k] = upper_left + 0.5f * (c->pixel_delta_u[k] + c->pixel_delta_v[k]);
        c->center[k] = p->lookfrom[k];
        c->u[k] = u[k];
        c->v[k] = v[k];
        c->w[k] = w[k];
    }
    const float defocus_radius = p->focus_dist * std::tan((p->defocus_angle / 2.0f) * pi / 180.0f);
    for (int k = 0; k < 3; k++) {
        c->defocus_disk_u[k] = u[k] * defocus_radius;
        c->defocus_disk_v[k] = v[k] * defocus_radius;
    }
    c->defocus_angle = p->defocus_angle;
    return RTW_OK;
}

// Stratified pixel samples: n x n jitter cells per pixel (rtw_device.h stratum_of); 0 and 1 are off
int rtw_camera_set_strata(rtw_camera* cam, uint32_t n) {
    if (!cam) return fail(RTW_E_INVALID, "rtw_camera_set_strata: null camera");
    if (n > RTW_MAX_STRATA) return fail(RTW_E_INVALID, "rtw_camera_set_strata: strata exceeds RTW_MAX_STRATA (256)");
    cam->strata = n;
    return RTW_OK;
}

void rtw_tuning_defaults(rtw_tuning* t) {
    if (!t) return;
    std::memset(t, 0, sizeof *t);
    t->kernel = RTW_KERNEL_WAVEFRONT;
    t->bvh_orders = 0;
    t->sah_max_leaf = 1;
    t->compact_nodes = 1;
    t->fast_box = 1;
    t->fast_reject = 1;
    t->lds = RTW_LDS_ALL;
    t->fuse = RTW_FUSE_STEP | RTW_FUSE_TAIL_LDS;
    t->wf_iters = 0;  // auto: 4, or every bounce (no tail) on image-textured scenes (profiles/r5_iters/)
    t->mega_shade_min = 48;  // tuned on C2: 8..64 -> 48 best
    t->mega_waves = 1;
    t->mega_tile_order = 1;
    t->cpu_threads = 0;
    t->wide_walk = 1;
    t->tile_lists = 1;
    t->hoist = 1;
    t->sort_iters = 3;
    t->sort_bits = RTW_WF_BUCKET_BITS;
    t->object_tree = 90;  // Cornell 1356 -> 1475, Cornell smoke +5.5 %
    t->sort_iters_split = 1;  // C4: 1 -> 2577, 3 -> 2518, 0 -> 2523 Msamples/s
    t->wf_paths = 0;
    // dynamic dealing of iteration 0 (runs, then 16 x waves singles), iterations >= 1 and the tail's input, on every
    // batch size: C2 +11 % over deal 3, C4 +7 %, C3 +9 %, a C2 shard of 8 +11 % (profiles/r5_deal/)
    t->deal = 59;
}

int rtw_scene_create(const rtw_scene_desc* d, int device, rtw_ctx** out) {
    return rtw_scene_create_ex(d, device, nullptr, out);
}

int rtw_scene_create_ex(const rtw_scene_desc* d, int device, const rtw_tuning* tuning, rtw_ctx** out) {
    if (!d || !out) return fail(RTW_E_INVALID, "null scene desc");
    rtw_tuning tu;
    rtw_tuning_defaults(&tu);
    if (tuning) tu = *tuning;
    if (int rc = check_tuning(tu)) return rc;
    *out = nullptr;
    if (int rc = check_desc(d)) return rc;
    const bool host = device == RTW_DEVICE_CPU;  // a host context: no GPU involved (rtw_cpu.hip)
    if (!host) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RTW_E_NODEVICE, "no HIP device visible");
        if (device < 0 || device >= ndev) return fail(RTW_E_INVALID, "device index out of range");
    }

    std::unique_ptr<rtw_ctx, CtxDestroy> ctx(new rtw_ctx());
    ctx->device = device;
    SceneParts P;
    const bool objects = d->n_quads || d->n_instances || d->n_media;
    const uint32_t sfeat = scene_features(d);
    const uint32_t orders = choose_orders(d, tu, sfeat, objects);
    uint32_t depth = 0, draws = 0, n_hoisted = 0;
    int rc = rtw_build_bvh(*d, ctx->nodes_host, P.geom, &depth, &draws, &ctx->box_pad, &ctx->extent, orders,
                           tu.sah_max_leaf, tu.hoist && !objects ? 1u : 0u, &n_hoisted,
                           objects ? (tu.object_tree & 0xFFu) : 0u);
    if (rc != RTW_OK) return fail(rc, "BVH build failed (bad object graph or bvh_mode)");
    if (int rh = split_hit_id(P.geom, ctx->nodes_host.size(), &ctx->base.hit_bits)) return rh;
    build_walk_records(d, tu, ctx.get(), orders, objects, P.walk);
    P.mats = dev_materials(d);
    P.texs = dev_textures(d);
    P.perlin = dev_perlins(d);
    dev_images(d, P.img_info, P.images);
    const Blob B = lay_out_blob(ctx.get(), P);
    std::vector<uint8_t> blob = fill_blob(B);
    if (!host)
        if (int ru = upload_blob(ctx.get(), blob)) return ru;
    ctx->blob_bytes = B.bytes;
    ctx->scene_hash = hash_blob(d, blob, B);
    if (host) ctx->host_blob = std::move(blob);  // the launch pointers address the host copy
    set_scene_pointers(ctx->base, host ? ctx->host_blob.data() : static_cast<const uint8_t*>(ctx->d_blob), B, P.walk);
    keep_host_copies(ctx.get(), d, P.geom);
    ctx->feat = sfeat | P.geom.feat;
    ctx->variant = tu.kernel == RTW_KERNEL_WAVEFRONT ? 2 : tu.kernel == RTW_KERNEL_PERSISTENT ? 1 : 0;

    set_stats(ctx.get(), d, orders, depth, draws, n_hoisted);
    set_wavefront_knobs(ctx.get(), tu, sfeat);
    set_launch_knobs(ctx.get(), d, tu, orders, B);
    ctx->grid = host ? 0 : rtw_persistent_grid(ctx->feat, ctx->stats.n_nodes, ctx->base.use_lds != 0);
    *out = ctx.release();
    return RTW_OK;
}

void rtw_scene_destroy(rtw_ctx* ctx) {
    if (!ctx) return;
    if (ctx->device == RTW_DEVICE_CPU) {
        delete ctx;
        return;
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->last_done) (void)hipEventSynchronize(ctx->last_done);  // a render left on a caller's stream
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->last_done) (void)hipEventDestroy(ctx->last_done);
    if (ctx->d_blob) (void)hipFree(ctx->d_blob);
    if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
    if (ctx->d_rows) (void)hipFree(ctx->d_rows);
    if (ctx->d_dbg) (void)hipFree(ctx->d_dbg);
    if (ctx->d_work) (void)hipFree(ctx->d_work);
    if (ctx->d_wf) (void)hipFree(ctx->d_wf);
    if (ctx->d_tl) (void)hipFree(ctx->d_tl);
    if (ctx->d_lights) (void)hipFree(ctx->d_lights);
    if (ctx->d_vattrs) (void)hipFree(ctx->d_vattrs);
    if (ctx->d_env) (void)hipFree(ctx->d_env);
    for (float4* p : ctx->d_dn)
        if (p) (void)hipFree(p);
    for (float* p : ctx->d_dnv)
        if (p) (void)hipFree(p);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int rtw_scene_flatten(const rtw_scene_desc* d, void* out, uint32_t cap, uint32_t* n_out, uint32_t* depth_out) {
    if (!d || !has_objects(d)) return fail(RTW_E_INVALID, "scene has no objects");
    std::vector<rtw_node> nodes;
    rtw_geometry geom;
    uint32_t depth = 0, draws = 0;
    int rc = rtw_build_bvh(*d, nodes, geom, &depth, &draws);
    if (rc != RTW_OK) return fail(rc, "BVH build failed");
    const uint32_t n = (uint32_t)nodes.size();
    if (n_out) *n_out = n;
    if (depth_out) *depth_out = depth;
    if (out) std::memcpy(out, nodes.data(), sizeof(rtw_node) * (cap < n ? cap : n));
    return RTW_OK;
}

int rtw_scene_hash(rtw_ctx* ctx, uint64_t* out) {
    if (!ctx || !out) return fail(RTW_E_INVALID, "null ctx");
    // the scene image, then the registered lights in order (none: the image's hash as it was): a checkpoint
    // taken with lights is another estimator's partial sum than one taken without
    std::lock_guard<std::mutex> lock(ctx->mu);  // the registrations write these vectors under it
    uint64_t h = ctx->scene_hash;
    auto mix = [&h](uint32_t w) {
        for (int b = 0; b < 4; b++) h = (h ^ ((w >> (8 * b)) & 0xFFu)) * 0x100000001B3ull;
    };
    if (!ctx->lights.empty()) {
        mix(0x5447494Cu);  // "LIGT"
        mix((uint32_t)ctx->lights.size());
        for (const rtw_object& o : ctx->lights) {
            mix(o.kind);
            mix(o.index);
        }
    }
    // then the registered vertex attributes (none: the hash as it was): another image
    if (!ctx->vattr_quads.empty()) {
        mix(0x52545441u);  // "ATTR"
        mix((uint32_t)ctx->vattr_quads.size());
        for (size_t k = 0; k < ctx->vattr_quads.size(); k++) {
            mix(ctx->vattr_quads[k]);
            uint32_t w[16];
            std::memcpy(w, &ctx->vattr_set[k], sizeof w);
            for (uint32_t x : w) mix(x);
        }
    }
    // then the registered environment (none: the hash as it was): its digest covers map, scale, rotation and flags
    if (ctx->env_hash) {
        mix(0x52564E45u);  // "ENVR"
        mix((uint32_t)ctx->env_hash);
        mix((uint32_t)(ctx->env_hash >> 32));
    }
    *out = h;
    return RTW_OK;
}

int rtw_scene_set_environment(rtw_ctx* ctx, const rtw_environment* env) {
#pragma STDC FP_CONTRACT OFF
    if (!ctx) return fail(RTW_E_INVALID, "null ctx");
    const bool host = ctx->device == RTW_DEVICE_CPU;
    std::vector<float4> block;
    std::vector<float> rgb;
    uint64_t digest = 0;
    char msg[240];
    if (env) {
        if (!env->rgb) return fail(RTW_E_INVALID, "rtw_scene_set_environment: null rgb");
        const uint32_t W = env->width, H = env->height;
        if (W == 0 || H == 0 || W > RTW_ENV_MAX_WIDTH || H > RTW_ENV_MAX_HEIGHT) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_environment: a map of %u x %u (1 x 1 up to %d x %d)", W, H,
                          RTW_ENV_MAX_WIDTH, RTW_ENV_MAX_HEIGHT);
            return fail(RTW_E_INVALID, msg);
        }
        for (int k = 0; k < 3; k++)
            if (!(env->scale[k] >= 0.0f) || !std::isfinite(env->scale[k])) {
                std::snprintf(msg, sizeof msg, "rtw_scene_set_environment: scale[%d] is negative or not finite", k);
                return fail(RTW_E_INVALID, msg);
            }
        if (!std::isfinite(env->rotate_y)) return fail(RTW_E_INVALID, "rtw_scene_set_environment: rotate_y is not finite");
        if (env->flags & ~(uint32_t)RTW_ENV_SAMPLE) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_environment: unknown flag bits 0x%x", env->flags);
            return fail(RTW_E_INVALID, msg);
        }
        const size_t n = (size_t)W * H;
        rgb.assign(env->rgb, env->rgb + 3 * n);  // the one read of the caller's memory
        for (size_t i = 0; i < 3 * n; i++)
            if (!(rgb[i] >= 0.0f) || !std::isfinite(rgb[i])) {
                std::snprintf(msg, sizeof msg, "rtw_scene_set_environment: texel (%zu, %zu) channel %zu is negative or "
                              "not finite", (i / 3) % W, (i / 3) / W, i % 3);
                return fail(RTW_E_INVALID, msg);
            }
        // the block: head (4 float4), texels, marginal, conditional (rtw_layout.h rtw_dev_env)
        const size_t head = sizeof(rtw_dev_env) / 16, tab = (H + n + 3) / 4;
        block.assign(head + n + tab, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        float4* tex = block.data() + head;
        float* marg = reinterpret_cast<float*>(tex + n);
        float* cond = marg + H;
        // radiance = scale * texel: one fp32 product per channel; a product that overflows is refused as a texel is
        for (size_t i = 0; i < n; i++) {
            tex[i] = make_float4(env->scale[0] * rgb[3 * i], env->scale[1] * rgb[3 * i + 1], env->scale[2] * rgb[3 * i + 2], 0.0f);
            if (!std::isfinite(tex[i].x) || !std::isfinite(tex[i].y) || !std::isfinite(tex[i].z)) {
                std::snprintf(msg, sizeof msg, "rtw_scene_set_environment: scale * texel (%zu, %zu) is not finite", i % W,
                              i / W);
                return fail(RTW_E_INVALID, msg);
            }
        }
        // The sampling tables, in fp64, stored as fp32: w = lum(radiance) sin(pi (j + 0.5) / H); the conditional
        // distribution of each row over its columns and the marginal one over the rows, cumulative, each divided
        // by its total and its last entry set to exactly 1 (a row of no weight: all 1, never picked -- its marginal
        // cell is empty); D = P_ij W H / (2 pi^2).
        const double pi = 3.14159265358979323846;
        std::vector<double> row_w(H, 0.0);
        double total = 0.0;
        for (uint32_t j = 0; j < H; j++) {
            const double sn = std::sin(pi * ((double)j + 0.5) / (double)H);
            double acc = 0.0;
            for (uint32_t i = 0; i < W; i++) {
                const float4 t = tex[(size_t)j * W + i];
                acc += (0.2126 * (double)t.x + 0.7152 * (double)t.y + 0.0722 * (double)t.z) * sn;
            }
            row_w[j] = acc;
            total += acc;
        }
        const bool sampled = (env->flags & RTW_ENV_SAMPLE) && total > 0.0 && std::isfinite(total);
        if (sampled) {
            const double dk = (double)W * (double)H / (2.0 * pi * pi);
            double macc = 0.0;
            for (uint32_t j = 0; j < H; j++) {
                const double sn = std::sin(pi * ((double)j + 0.5) / (double)H);
                double acc = 0.0;
                for (uint32_t i = 0; i < W; i++) {
                    float4& t = tex[(size_t)j * W + i];
                    const double w = (0.2126 * (double)t.x + 0.7152 * (double)t.y + 0.0722 * (double)t.z) * sn;
                    acc += w;
                    cond[(size_t)j * W + i] = row_w[j] > 0.0 ? (float)(acc / row_w[j]) : 1.0f;
                    t.w = (float)(w / total * dk);
                }
                cond[(size_t)j * W + W - 1] = 1.0f;
                macc += row_w[j];
                marg[j] = (float)(macc / total);
            }
            // rounding to fp32 may lift an entry onto 1 before the last row or column of weight: keep every entry
            // below the last cell of weight strictly below 1, so that cell stays pickable
            auto cap = [](float* c, uint32_t m, auto weight) {
                uint32_t last = m - 1;
                while (last > 0 && !(weight(last) > 0.0)) last--;
                for (uint32_t k = 0; k < last; k++)
                    if (c[k] >= 1.0f) c[k] = 0x1.fffffep-1f;
                for (uint32_t k = last; k < m; k++) c[k] = 1.0f;
            };
            cap(marg, H, [&](uint32_t j) { return row_w[j]; });
            for (uint32_t j = 0; j < H; j++)
                if (row_w[j] > 0.0)
                    cap(cond + (size_t)j * W, W, [&](uint32_t i) {
                        const float4 t = tex[(size_t)j * W + i];
                        return 0.2126 * (double)t.x + 0.7152 * (double)t.y + 0.0722 * (double)t.z;
                    });
        }
        rtw_dev_env hd{};
        hd.width = W;
        hd.height = H;
        {   // RotateY.init (objects.zig:352-355): degreesToRadians in fp32, then sin / cos, as rtw_bvh.hip takes them
            const float pi32 = 3.1415926535897932385f;
            const float radians = env->rotate_y * pi32 / 180.0f;
            hd.sin_y = std::sin(radians);
            hd.cos_y = std::cos(radians);
        }
        hd.sampled = sampled ? 1u : 0u;
        hd.texels = tex;
        hd.marginal = marg;
        hd.conditional = cond;
        std::memcpy(block.data(), &hd, sizeof hd);
        // the digest: FNV-1a 64 of dimensions, scale, rotation, flags and the map as given; never 0
        uint64_t h = 0xCBF29CE484222325ull;
        auto mixb = [&h](const void* p, size_t nb) {
            const uint8_t* b = static_cast<const uint8_t*>(p);
            for (size_t i = 0; i < nb; i++) h = (h ^ b[i]) * 0x100000001B3ull;
        };
        mixb(&W, 4);
        mixb(&H, 4);
        mixb(env->scale, 12);
        mixb(&env->rotate_y, 4);
        mixb(&env->flags, 4);
        mixb(rgb.data(), rgb.size() * 4);
        digest = h ? h : 1;
    }
    std::lock_guard<std::mutex> lock(ctx->mu);
    rtw_launch base = ctx->base;
    void* d_new = nullptr;
    if (!host) {
        HIP_TRY(hipSetDevice(ctx->device));
        // a render left on a caller's stream (RTW_RENDER_NO_SYNC) may still read the old block
        if (ctx->last_done) HIP_TRY(hipEventSynchronize(ctx->last_done));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (env) {
            HIP_TRY(hipMalloc(&d_new, block.size() * 16));
            // the device copy's head addresses the device copy's tables
            std::vector<float4> headv(block.begin(), block.begin() + sizeof(rtw_dev_env) / 16);
            rtw_dev_env hd;
            std::memcpy(&hd, headv.data(), sizeof hd);
            const char* hb = reinterpret_cast<const char*>(block.data());
            char* db = static_cast<char*>(d_new);
            hd.texels = reinterpret_cast<const float4*>(db + (reinterpret_cast<const char*>(hd.texels) - hb));
            hd.marginal = reinterpret_cast<const float*>(db + (reinterpret_cast<const char*>(hd.marginal) - hb));
            hd.conditional = reinterpret_cast<const float*>(db + (reinterpret_cast<const char*>(hd.conditional) - hb));
            hipError_t e = hipMemcpy(d_new, block.data(), block.size() * 16, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(d_new, &hd, sizeof hd, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(d_new);
                return rtw_hip_fail(e, "rtw_scene_set_environment: upload");
            }
        }
    }
    // (moving the vector keeps its storage: the head's host addresses stay valid)
    const rtw_dev_env* addr = !env ? nullptr : host ? reinterpret_cast<const rtw_dev_env*>(block.data())
                                                    : static_cast<const rtw_dev_env*>(d_new);
    if (!rtw_env_set(base, addr)) {
        if (d_new) (void)hipFree(d_new);
        return fail(RTW_E_INVALID, "rtw_scene_set_environment: the block's address does not fit 48 bits");
    }
    if (ctx->d_env) (void)hipFree(ctx->d_env);
    ctx->d_env = d_new;
    ctx->env_block = std::move(block);
    ctx->env_rgb = std::move(rgb);
    ctx->env_given = env ? *env : rtw_environment{};
    ctx->env_given.rgb = nullptr;
    ctx->env_hash = digest;
    // the persistent kernel's resident grid is its instantiation's
    if (!host) ctx->grid = rtw_persistent_grid(rtw_feat_of(base), ctx->stats.n_nodes, base.use_lds != 0);
    ctx->base = base;
    return RTW_OK;
}

int rtw_scene_environment_get(rtw_ctx* ctx, rtw_environment* out, float* rgb, uint64_t cap_floats) {
    if (!ctx) return fail(RTW_E_INVALID, "null ctx");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (out) *out = ctx->env_given;
    if (rgb && !ctx->env_rgb.empty())
        std::memcpy(rgb, ctx->env_rgb.data(), 4 * (size_t)std::min<uint64_t>(cap_floats, ctx->env_rgb.size()));
    return RTW_OK;
}

int rtw_scene_set_vertex_attrs(rtw_ctx* ctx, const uint32_t* quads, const rtw_vertex_attr* attrs, uint32_t n) {
    if (!ctx) return fail(RTW_E_INVALID, "null ctx");
    if (n && (!quads || !attrs)) return fail(RTW_E_INVALID, "rtw_scene_set_vertex_attrs: null quads or attrs");
    const size_t nq = ctx->quads_host.size();
    std::vector<rtw_dev_vattr> rec(n ? nq : 0);  // dense, parallel to the quads: flags = 0 where none is registered
    std::vector<rtw_vertex_attr> set(n);
    std::vector<uint8_t> seen(n ? nq : 0, 0);
    char msg[240];
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t qi = quads[k];
        if (qi >= nq) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_vertex_attrs: entry %u: quad index %u out of range", k, qi);
            return fail(RTW_E_INVALID, msg);
        }
        if (!(ctx->quads_host[qi].mat & RTW_QUAD_TRI_BIT)) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_vertex_attrs: entry %u: quad %u is a parallelogram (only "
                          "RTW_QUAD_TRIANGLE records take attributes)", k, qi);
            return fail(RTW_E_INVALID, msg);
        }
        if (seen[qi]) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_vertex_attrs: entry %u: quad %u is listed twice", k, qi);
            return fail(RTW_E_INVALID, msg);
        }
        seen[qi] = 1;
        const rtw_vertex_attr& a = attrs[k];
        if (a.flags & ~(uint32_t)(RTW_ATTR_NORMALS | RTW_ATTR_UVS)) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_vertex_attrs: entry %u (quad %u): unknown flag bits 0x%x", k,
                          qi, a.flags);
            return fail(RTW_E_INVALID, msg);
        }
        rtw_vertex_attr o{};
        o.flags = a.flags;
        if (a.flags & RTW_ATTR_NORMALS) {
            if (!rtw_vattr_normalise(a, o)) {
                std::snprintf(msg, sizeof msg, "rtw_scene_set_vertex_attrs: entry %u (quad %u): a normal is not finite "
                              "or has zero length", k, qi);
                return fail(RTW_E_INVALID, msg);
            }
        }
        if (a.flags & RTW_ATTR_UVS) {
            for (int c = 0; c < 3; c++)
                for (int i = 0; i < 2; i++) {
                    if (!std::isfinite(a.uv[c][i])) {
                        std::snprintf(msg, sizeof msg, "rtw_scene_set_vertex_attrs: entry %u (quad %u): a uv is not "
                                      "finite", k, qi);
                        return fail(RTW_E_INVALID, msg);
                    }
                    o.uv[c][i] = a.uv[c][i];
                }
        }
        set[k] = o;
        static_assert(sizeof(rtw_dev_vattr) == sizeof(rtw_vertex_attr), "the device record is the public one");
        std::memcpy(&rec[qi], &o, sizeof o);
    }
    std::lock_guard<std::mutex> lock(ctx->mu);
    rtw_launch base = ctx->base;
    if (int rc = publish_records(ctx, base, ctx->vattrs_rec, rec, &ctx->d_vattrs, nq, base.vattrs)) return rc;
    ctx->vattr_quads.assign(quads, quads + n);
    ctx->vattr_set = set;
    ctx->base = base;
    return RTW_OK;
}

int rtw_scene_vertex_attrs_get(rtw_ctx* ctx, uint32_t* quads, rtw_vertex_attr* attrs, uint32_t cap, uint32_t* n_out) {
    if (!ctx) return fail(RTW_E_INVALID, "null ctx");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const uint32_t n = (uint32_t)ctx->vattr_quads.size();
    if (n_out) *n_out = n;
    const uint32_t m = cap < n ? cap : n;
    if (quads && m) std::memcpy(quads, ctx->vattr_quads.data(), sizeof(uint32_t) * m);
    if (attrs && m) std::memcpy(attrs, ctx->vattr_set.data(), sizeof(rtw_vertex_attr) * m);
    return RTW_OK;
}

int rtw_scene_set_lights(rtw_ctx* ctx, const rtw_object* lights, uint32_t n) {
    if (!ctx) return fail(RTW_E_INVALID, "null ctx");
    if (n && !lights) return fail(RTW_E_INVALID, "rtw_scene_set_lights: null lights");
    if (n > RTW_MAX_LIGHTS) return fail(RTW_E_INVALID, "rtw_scene_set_lights: more than RTW_MAX_LIGHTS (16) lights");
    std::vector<rtw_dev_light> rec(n);
    char msg[240];
    for (uint32_t k = 0; k < n; k++) {
        const rtw_object o = lights[k];
        if (o.kind != RTW_OBJ_QUAD && o.kind != RTW_OBJ_SPHERE) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_lights: light %u is neither a quad nor a sphere (instances "
                          "and media cannot be sampled)", k);
            return fail(RTW_E_INVALID, msg);
        }
        const bool sph = o.kind == RTW_OBJ_SPHERE;
        const char* what = sph ? "sphere" : "quad";
        if (o.index >= (sph ? ctx->spheres_host.size() : ctx->quads_host.size())) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_lights: light %u: %s index %u out of range", k, what,
                          o.index);
            return fail(RTW_E_INVALID, msg);
        }
        if (sph && !(ctx->feat & RTW_F_GEOM)) {
            // sphere scenes walk octant copies, compact nodes, tile lists and hoisted spheres, which the
            // RTW_F_ALL | RTW_F_PDF kernels do not
            std::snprintf(msg, sizeof msg, "rtw_scene_set_lights: light %u (sphere %u): a scene of spheres alone "
                          "cannot register lights (its kernels have no mixture-density form; out of scope)", k,
                          o.index);
            return fail(RTW_E_INVALID, msg);
        }
        const uint32_t ref = RTW_REF(o.kind, o.index);
        if (std::find(ctx->members_host.begin(), ctx->members_host.end(), ref) != ctx->members_host.end()) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_lights: light %u (%s %u) is an instance member", k, what,
                          o.index);
            return fail(RTW_E_INVALID, msg);
        }
        if (std::find(ctx->boundaries_host.begin(), ctx->boundaries_host.end(), ref) != ctx->boundaries_host.end()) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_lights: light %u (%s %u) is a medium boundary", k, what,
                          o.index);
            return fail(RTW_E_INVALID, msg);
        }
        bool top = false;  // a leaf of the world tree (the first ordering: object scenes keep one)
        for (uint32_t i = 0; i < ctx->stats.n_nodes && !top; i++) {
            uint32_t aw, bz, bw;
            std::memcpy(&aw, &ctx->nodes_host[i].a[3], 4);
            std::memcpy(&bz, &ctx->nodes_host[i].b[2], 4);
            std::memcpy(&bw, &ctx->nodes_host[i].b[3], 4);
            top = (aw & RTW_LEAF_BIT) && RTW_LEAF_KIND(bw) == o.kind && bz == o.index;
        }
        if (!top) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_lights: light %u (%s %u) is not in the scene's object list",
                          k, what, o.index);
            return fail(RTW_E_INVALID, msg);
        }
        const uint32_t mat = sph ? ctx->spheres_host[o.index].mat : RTW_QUAD_MAT(ctx->quads_host[o.index].mat);
        if (ctx->mat_kind_host[mat] != RTW_MAT_DIFFUSE_LIGHT) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_lights: light %u (%s %u): its material is not "
                          "RTW_MAT_DIFFUSE_LIGHT", k, what, o.index);
            return fail(RTW_E_INVALID, msg);
        }
        for (uint32_t j = 0; j < k; j++)
            if (lights[j].kind == o.kind && lights[j].index == o.index) {
                std::snprintf(msg, sizeof msg, "rtw_scene_set_lights: %s %u is listed twice", what, o.index);
                return fail(RTW_E_INVALID, msg);
            }
        rec[k] = rtw_dev_light{};
        rec[k].kind = o.kind;
        if (sph) {
            const rtw_dev_sphere& s = ctx->spheres_host[o.index];
            if (s.moving) {
                std::snprintf(msg, sizeof msg, "rtw_scene_set_lights: light %u (sphere %u) is a moving sphere (out of "
                              "scope: only static spheres can be sampled)", k, o.index);
                return fail(RTW_E_INVALID, msg);
            }
            if (!(s.radius > 0.0f) || !std::isfinite(s.radius)) {
                std::snprintf(msg, sizeof msg, "rtw_scene_set_lights: light %u (sphere %u) has no finite positive "
                              "radius", k, o.index);
                return fail(RTW_E_INVALID, msg);
            }
            rec[k].radius = s.radius;
            for (int i = 0; i < 3; i++) rec[k].c[i] = s.c1[i];
            continue;
        }
        const rtw_dev_quad& q = ctx->quads_host[o.index];
        // area = |cross(u, v)| (vec3.zig:31-33 cross, fp32); a triangle's (RTW_QUAD_TRI_BIT, rtw_layout.h): half of it
        const float cx = q.u[1] * q.v[2] - q.u[2] * q.v[1], cy = q.u[2] * q.v[0] - q.u[0] * q.v[2],
                    cz = q.u[0] * q.v[1] - q.u[1] * q.v[0];
        const float par = std::sqrt(cx * cx + cy * cy + cz * cz);
        const float area = (q.mat & RTW_QUAD_TRI_BIT) ? par / 2.0f : par;
        if (!(area > 0.0f) || !std::isfinite(area)) {
            std::snprintf(msg, sizeof msg, "rtw_scene_set_lights: light %u (quad %u) has no area", k, o.index);
            return fail(RTW_E_INVALID, msg);
        }
        rec[k].quad = o.index;
        rec[k].area = area;
    }
    std::lock_guard<std::mutex> lock(ctx->mu);
    rtw_launch base = ctx->base;
    base.n_lights = n;
    if (int rc = publish_records(ctx, base, ctx->lights_rec, rec, &ctx->d_lights, RTW_MAX_LIGHTS, base.lights))
        return rc;
    ctx->lights.assign(lights, lights + n);
    ctx->base = base;
    return RTW_OK;
}

int rtw_scene_lights_get(rtw_ctx* ctx, rtw_object* out, uint32_t cap, uint32_t* n_out) {
    if (!ctx) return fail(RTW_E_INVALID, "null ctx");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const uint32_t n = (uint32_t)ctx->lights.size();
    if (n_out) *n_out = n;
    if (out && n) std::memcpy(out, ctx->lights.data(), sizeof(rtw_object) * (cap < n ? cap : n));
    return RTW_OK;
}

int rtw_scene_stats_get(rtw_ctx* ctx, rtw_scene_stats* out) {
    if (!ctx || !out) return fail(RTW_E_INVALID, "null ctx");
    *out = ctx->stats;
    return RTW_OK;
}

int rtw_scene_nodes(rtw_ctx* ctx, void* out, uint32_t cap, uint32_t* n_out) {
    if (!ctx) return fail(RTW_E_INVALID, "null ctx");
    const uint32_t n = ctx->stats.n_nodes;  // the first ordering
    if (n_out) *n_out = n;
    if (out) std::memcpy(out, ctx->nodes_host.data(), sizeof(rtw_node) * (cap < n ? cap : n));
    return RTW_OK;
}

int rtw_scene_instance_nodes(rtw_ctx* ctx, uint32_t instance, void* out, uint32_t cap, uint32_t* n_out) {
    if (!ctx) return fail(RTW_E_INVALID, "null ctx");
    if (instance >= ctx->inst_tree.size()) return fail(RTW_E_INVALID, "instance index out of range");
    const uint32_t first = ctx->inst_tree[instance].first, n = ctx->inst_tree[instance].second;
    if (n_out) *n_out = n;
    if (out && n) std::memcpy(out, ctx->inodes_host.data() + first, sizeof(rtw_node) * (cap < n ? cap : n));
    return RTW_OK;
}

}  // extern "C"

namespace {

rtw_launch make_launch(const rtw_ctx* ctx, const rtw_camera* c, uint64_t seed) {
    rtw_launch L = ctx->base;
    rtw_launch_camera(L, c, seed);
    if (L.fast_box) {
        // the box pad covers ray origins with |o| <= 7 * extent (rtw_bvh.hip): primary
        // origins are the camera centre + the defocus disk; secondary ones lie in the scene
        float o = 0;
        for (int k = 0; k < 3; k++)
            o = std::max(o, std::fabs(c->center[k]) + std::fabs(c->defocus_disk_u[k]) +
                                std::fabs(c->defocus_disk_v[k]));
        if (!(o <= 7.0f * ctx->extent)) L.fast_box = 0;
    }
    return L;
}

}  // namespace

rtw_launch rtw_make_launch(const rtw_ctx* ctx, const rtw_camera* c, uint64_t seed) { return make_launch(ctx, c, seed); }

// the camera's part of a launch, and the render-domain key (make_launch; rtw_debug_camera_ray, which has no context)
void rtw_launch_camera(rtw_launch& L, const rtw_camera* c, uint64_t seed) {
    for (int k = 0; k < 3; k++) {
        L.center[k] = c->center[k];
        L.pixel00[k] = c->pixel00_loc[k];
        L.du[k] = c->pixel_delta_u[k];
        L.dv[k] = c->pixel_delta_v[k];
        L.disk_u[k] = c->defocus_disk_u[k];
        L.disk_v[k] = c->defocus_disk_v[k];
        L.background[k] = c->background[k];
    }
    L.defocus_angle = c->defocus_angle;
    L.W = c->image_width;
    L.H = c->image_height;
    L.max_depth = c->max_depth;
    L.bg_mode = c->background_mode;
    L.pixel_offset = c->pixel_offset;
    L.strata = c->strata;
    L.key0 = rtw_mix64(seed);
}

uint32_t rtw_auto_batch(const rtw_ctx* ctx, uint64_t pixels, uint32_t spp) {
    // ~64M samples per launch (the wavefront: its batch capacity): long enough to
    // amortise the launches, short enough to poll cancel
    const uint64_t target = ctx->variant == 2 ? ctx->wf_max_paths : (64ull << 20);
    uint64_t b = pixels ? target / pixels : spp;
    if (b < 1) b = 1;
    if (b > spp) b = spp;
    return (uint32_t)b;
}

int rtw_validate_cam(const rtw_camera* cam) {
    if (!cam) return fail(RTW_E_INVALID, "null camera");
    if (cam->image_width == 0 || cam->image_height == 0) return fail(RTW_E_INVALID, "camera not initialised");
    if ((uint64_t)cam->image_width * cam->image_height > 0xFFFFFFFFull) return fail(RTW_E_INVALID, "image too large");
    if (cam->strata > RTW_MAX_STRATA) return fail(RTW_E_INVALID, "camera: strata exceeds RTW_MAX_STRATA (256)");
    return RTW_OK;
}

// the ABI-5 options of the host-buffer entry points: stop/progress and spp_batch only
int rtw_check_host_opts(const rtw_render_opts* o) {
    if (o && (o->flags || o->counters || o->timing))
        return fail(RTW_E_INVALID, "host-buffer render: flags, counters and timing must be 0/NULL");
    return RTW_OK;
}

namespace {

// Bytes of the wavefront state run_wavefront takes from one allocation: per slot set (two) the ray_o, ray_d,
// thr, acc streams (16 B) and rng (8 B); the hit records (8 B) by slot; the radiance (12 B) by path; the three
// stripe-counter sets; each take 256-B aligned.  RTW_WF_PATH_BYTES is the per-path part of the same sum.
size_t wf_state_bytes(uint64_t Q, uint64_t P) {
    auto al = [](uint64_t b) { return (size_t)((b + 255) & ~uint64_t(255)); };
    return 2 * (4 * al(Q * 16) + al(Q * 8)) + al(Q * 8) + al(P * sizeof(rtw_rgb)) +
           3 * al((uint64_t)RTW_WF_STRIPES * RTW_WF_LEN_STRIDE * 4) + al(RTW_WF_DEAL_COUNTERS * 4);
}
static_assert(RTW_WF_PATH_BYTES == 2 * (4 * 16 + 8) + 8 + sizeof(rtw_rgb),
              "RTW_WF_PATH_BYTES = wf_state_bytes per path");

// The launch's 8x8 tiles over its rows (W.n_tx; returns the logical pixels, 64 per tile) and the context's
// camera-ray candidate lists for them (the compact-LDS fused step of static sphere scenes, rtw_tuning.tile_lists):
// W.tl / W.tl_count, left null when the launch has none.  (run_wavefront and rtw_debug_tile_lists)
uint64_t wf_tile_grid(const rtw_launch& L, rtw_wf& W) {
    W.n_tx = (L.W + 7) / 8;
    return (uint64_t)W.n_tx * ((L.n_rows + 7) / 8) * 64;
}
void wf_tile_buffer(rtw_ctx* ctx, const rtw_launch& L, rtw_wf& W, uint64_t n_pix, hipStream_t stream) {
    if (L.tile_lists && L.cnodes && L.n_orders >= 4) {
        const uint64_t tiles = n_pix / 64;
        if (ctx->tl_cap < tiles &&
            rtw_device_grow(&ctx->d_tl, &ctx->tl_cap, tiles, tiles * RTW_TL_BYTES + 256, stream) != hipSuccess)
            (void)hipGetLastError();  // no lists: the walk
        if (ctx->tl_cap >= tiles) {
            W.tl = static_cast<uint4*>(ctx->d_tl);
            W.tl_count = reinterpret_cast<uint32_t*>(static_cast<char*>(ctx->d_tl) + tiles * RTW_TL_MAX * 32);
        }
    }
}

// Wavefront (v2) render of samples [L.s0, L.s1): batches of n_s samples so that
// n_pix * n_s paths fit the path-state buffer (grown on demand, kept in the ctx).
int run_wavefront(rtw_ctx* ctx, rtw_launch L, hipStream_t stream, rtw_timer* T) {
    rtw_wf W{};
    const uint64_t n_pix = wf_tile_grid(L, W);
    const uint32_t spp = L.s1 - L.s0;
    uint64_t n_s = std::max<uint64_t>(1, ctx->wf_max_paths / n_pix);
    if (n_s > spp) n_s = spp;
    uint64_t need = n_pix * n_s;
    if (need > 0x7FFFFFFFull) return fail(RTW_E_INVALID, "wavefront batch too large");
    // stripe capacity: a stripe receives the survivors of nw/STRIPES waves that
    // each take <= ceil(chunks / nw) 64-path chunks (rtw_wavefront.h)
    const uint64_t max_waves = rtw_wavefront_max_waves(ctx->n_cu);
    // + direction-bucketed iterations: every wave of a stripe may leave one partly filled 64-slot block per
    //   bucket (wf_push_bucketed)
    const bool bucketed = ctx->wf_sort_iters || ctx->wf_sort_iters_split;
    const uint64_t bucket_blocks = bucketed ? (max_waves / RTW_WF_STRIPES + 1) * RTW_WF_BUCKETS : 0;
    // + the dynamic deal of iteration 0 (rtw_tuning.deal bit 1): a stripe group claims whole runs of 16 chunks
    //   and then singles, so it may end up to one run and one single chunk above its even share (RUN + 1), whatever
    //   the grid's waves per stripe (a device or partition with few CUs)
    const uint64_t deal_slack = ctx->wf_deal ? (1u << 4) + 1u : 0u;
    auto stripe_cap = [&](uint64_t paths) {
        return ((paths + 63) / 64 / RTW_WF_STRIPES + 1 + max_waves / RTW_WF_STRIPES + bucket_blocks + deal_slack) * 64;
    };
    // slots per set: every path (iteration 0: slot = path id) or every stripe's capacity
    auto slots = [&](uint64_t paths) { return std::max<uint64_t>(paths, stripe_cap(paths) * RTW_WF_STRIPES); };
    if (ctx->wf_cap < need) {
        for (;;) {  // device memory taken since scene creation (other contexts, torch): halve the batch
            const size_t bytes = wf_state_bytes(slots(need), need);
            const hipError_t e = rtw_device_grow(&ctx->d_wf, &ctx->wf_cap, need, bytes, stream);
            if (e == hipSuccess) break;
            if (e != hipErrorOutOfMemory || n_s == 1) return rtw_hip_fail(e, "wavefront path state");
            (void)hipGetLastError();  // clear the sticky OOM before the retry
            n_s = (n_s + 1) / 2;
            need = n_pix * n_s;
            ctx->wf_max_paths = need;  // later renders start from the size that fit
        }
    }
    if (n_s * n_pix > ctx->wf_cap) n_s = std::max<uint64_t>(1, ctx->wf_cap / n_pix);
    const uint64_t P = ctx->wf_cap, Q = slots(P);
    // (the takes below are the layout wf_state_bytes sizes)
    char* cur = static_cast<char*>(ctx->d_wf);
    auto take = [&](size_t nb) {
        char* p = cur;
        cur += (nb + 255) & ~size_t(255);
        return p;
    };
    for (int k = 0; k < 2; k++) {
        rtw_wf_set& S = W.set[k];
        S.ray_o = reinterpret_cast<float4*>(take(Q * 16));
        S.ray_d = reinterpret_cast<float4*>(take(Q * 16));
        S.thr = reinterpret_cast<float4*>(take(Q * 16));
        S.acc = reinterpret_cast<float4*>(take(Q * 16));
        S.rng = reinterpret_cast<uint64_t*>(take(Q * 8));
    }
    W.hit = reinterpret_cast<float2*>(take(Q * 8));
    W.ls = reinterpret_cast<rtw_rgb*>(take(P * sizeof(rtw_rgb)));
    for (int k = 0; k < 3; k++) W.len[k] = reinterpret_cast<uint32_t*>(take(RTW_WF_STRIPES * RTW_WF_LEN_STRIDE * 4));
    uint32_t* deal = reinterpret_cast<uint32_t*>(take(RTW_WF_DEAL_COUNTERS * 4));
    W.deal = ctx->wf_deal ? deal : nullptr;
    W.deal_mode = ctx->wf_deal;
    W.deal_it = nullptr;  // set per launch (deal bit 16)
    W.n_pix = (uint32_t)n_pix;
    W.iters = ctx->wf_iters;
    W.sort_iters = ctx->wf_sort_iters;
    W.sort_iters_split = ctx->wf_sort_iters_split;
    W.sort_mask = ctx->wf_sort_mask;
    W.run_log2 = 4;  // set per launch grid by wf_coherence (rtw_wavefront.hip)
    wf_tile_buffer(ctx, L, W, n_pix, stream);
    const uint32_t s_end = L.s1;
    for (uint32_t s = L.s0; s < s_end; s += (uint32_t)n_s) {
        L.s0 = s;
        L.s1 = (s_end - s < n_s) ? s_end : s + (uint32_t)n_s;
        W.n_s = L.s1 - L.s0;
        W.n_paths = (uint32_t)(n_pix * W.n_s);
        W.stripe_cap = (uint32_t)stripe_cap(W.n_paths);
        ctx->wf_len = W.len[0];
        ctx->wf_stripe_cap = W.stripe_cap;
        rtw_wavefront_batch(L, W, stream, ctx->n_cu, T);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return rtw_hip_fail(e, "wavefront launch");
    }
    return RTW_OK;
}

// Enqueue [s0, s1) in batches of `batch` samples on `stream`.  When the caller polls (ctl's stop
// flags or progress, ABI 5) the stop flags are read before every batch and, after each one, the stream
// is synchronised and progress called: a stop keeps the finished batches (their .w = the last batch's end).
int run_batches(rtw_ctx* ctx, rtw_launch L, uint32_t s0, uint32_t s1, uint32_t batch, hipStream_t stream,
                const rtw_render_opts* ctl, uint64_t pixels, rtw_timer* T = nullptr) {
    const uint64_t total = pixels * (uint64_t)(s1 - s0);
    const bool polled = rtw_polled(ctl);
    for (uint32_t s = s0; s < s1; s += batch) {
        if (rtw_stop_requested(ctl)) return fail(RTW_E_CANCELLED, "cancelled");
        L.s0 = s;
        L.s1 = (s1 - s < batch) ? s1 : s + batch;
        if (ctx->variant == 2) {
            if (int rc = run_wavefront(ctx, L, stream, T)) return rc;
        } else {
            if (ctx->variant == 1) HIP_TRY(hipMemsetAsync(ctx->d_work, 0, 256, stream));
            RTW_TIME_BEGIN(T, RTW_K_MEGA)
            rtw_launch_render(L, stream, ctx->variant, ctx->grid);
            RTW_TIME_END(T)
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return rtw_hip_fail(e, "render launch");
        }
        if (polled) {
            HIP_TRY(hipStreamSynchronize(stream));
            if (ctl->progress && ctl->progress(pixels * (uint64_t)(L.s1 - s0), total, ctl->user))
                return fail(RTW_E_CANCELLED, "cancelled by progress callback");
        }
    }
    return RTW_OK;
}

// Host context: samples [s0, s1) in batches on host threads (rtw_cpu.hip), stop flags polled per pixel,
// progress after each batch.  begin/end/out as rtw_cpu_render.
int run_host(rtw_ctx* ctx, rtw_launch L, uint32_t begin, uint32_t end, uint32_t s0, uint32_t s1,
             uint32_t batch, float* out, const rtw_render_opts* ctl, uint64_t pixels) {
    // concurrent callers (the 8 Tasks on one host context) share the context's threads instead of each
    // starting a pool of its own: a call takes cpu_threads / (calls in flight), at least 1
    struct Count {
        std::atomic<uint32_t>& c;
        uint32_t n;
        explicit Count(std::atomic<uint32_t>& a) : c(a), n(a.fetch_add(1) + 1) {}
        ~Count() { c.fetch_sub(1); }
    } in_flight(ctx->cpu_calls);
    const uint32_t pool = ctx->cpu_threads ? ctx->cpu_threads : std::max(1u, std::thread::hardware_concurrency());
    const uint32_t threads = std::max(1u, pool / in_flight.n);
    // stop flags: with an explicit spp_batch they are polled between batches only, so a stopped render
    // holds whole batches (every pixel's .w is the last finished batch's end, and a resume from it adds
    // no sample twice); without one, per pixel as Camera.render polls `running` (camera.zig:107) --
    // then each pixel's .w says how far that pixel got
    const bool per_pixel = batch == 0;
    if (!batch) batch = s1 - s0;
    const uint64_t total = pixels * (uint64_t)(s1 - s0);
    for (uint32_t s = s0; s < s1; s += batch) {
        if (!per_pixel && rtw_stop_requested(ctl)) return fail(RTW_E_CANCELLED, "cancelled");
        L.s0 = s;
        L.s1 = (s1 - s < batch) ? s1 : s + batch;
        if (rtw_cpu_render(L, begin, end, out, threads, per_pixel ? ctl : nullptr) == RTW_E_CANCELLED)
            return fail(RTW_E_CANCELLED, "cancelled");
        if (ctl && ctl->progress && ctl->progress(pixels * (uint64_t)(L.s1 - s0), total, ctl->user))
            return fail(RTW_E_CANCELLED, "cancelled by progress callback");
    }
    return RTW_OK;
}

// Synchronise and sum the timer's events per kernel kind into `out`.
int harvest_timing(rtw_ctx* ctx, rtw_timer& T, rtw_kernel_timing* out) {
    HIP_TRY(hipStreamSynchronize(T.stream));
    std::memset(out, 0, sizeof *out);
    for (const rtw_timer::rec& r : T.recs) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        if (r.kind >= 0 && r.kind < RTW_K_COUNT) {
            out->ms[r.kind] += ms;
            out->launches[r.kind]++;
        }
        ctx->ev_pool.push_back(r.a);
        ctx->ev_pool.push_back(r.b);
    }
    T.recs.clear();
    return RTW_OK;
}

void set_tiles(rtw_launch& L) {
    L.n_tiles_x = (L.W + RTW_TILE_W - 1) / RTW_TILE_W;
    L.n_tiles = L.n_tiles_x * ((L.n_rows + RTW_TILE_H - 1) / RTW_TILE_H);
}

// the context's device staging buffer of the host-buffer entry points, >= bytes
int ensure_scratch(rtw_ctx* ctx, size_t bytes) {
    if (ctx->scratch_bytes >= bytes) return RTW_OK;
    HIP_TRY(rtw_device_grow(&ctx->d_scratch, &ctx->scratch_bytes, bytes, bytes, ctx->stream));
    return RTW_OK;
}

// Order this call's stream after the previous call's work on this context (another stream).
int stream_enter(rtw_ctx* ctx, hipStream_t s) {
    if (ctx->last_stream && ctx->last_stream != s) HIP_TRY(hipStreamWaitEvent(s, ctx->last_done, 0));
    return RTW_OK;
}
int stream_leave(rtw_ctx* ctx, hipStream_t s) {
    if (!ctx->last_done) HIP_TRY(hipEventCreateWithFlags(&ctx->last_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ctx->last_done, s));
    ctx->last_stream = s;
    return RTW_OK;
}

// the launch's work fields for the pixels [pix_begin, pix_end) of the image (plain mode: no shards)
void set_plain_range(rtw_launch& L, uint32_t pix_begin, uint32_t pix_end) {
    L.pix_begin = pix_begin;
    L.pix_end = pix_end;
    L.row0 = pix_begin / L.W;
    L.n_rows = (pix_end - 1) / L.W - L.row0 + 1;
    L.n_shards = 0;
    set_tiles(L);
}

bool shard_spec_ok(uint32_t rpb, uint32_t n_shards, uint32_t shard) {
    return (rpb & ~RTW_ROWS_FLAGS) && n_shards && shard < n_shards;
}

// Enqueue the device render of samples [spp_begin, spp_end) of the prepared launch on stream s and finish the
// call (the caller holds ctx->mu and has entered the stream): opts' counters, batch size, timing and
// RTW_RENDER_NO_SYNC; `pixels` is what the progress callback and the automatic batch count.
int enqueue_and_finish(rtw_ctx* ctx, rtw_launch& L, uint32_t spp_begin, uint32_t spp_end, hipStream_t s,
                       const rtw_render_opts* opts, uint64_t pixels) {
    L.counters = opts ? reinterpret_cast<unsigned long long*>(opts->counters) : nullptr;
    const uint32_t batch = opts && opts->spp_batch ? opts->spp_batch : rtw_auto_batch(ctx, pixels, spp_end - spp_begin);
    rtw_timer T;
    T.stream = s;
    T.pool.swap(ctx->ev_pool);
    rtw_timer* tp = (opts && opts->timing) ? &T : nullptr;
    int rc = run_batches(ctx, L, spp_begin, spp_end, batch, s, opts, pixels, tp);
    ctx->ev_pool.swap(T.pool);
    if (int rl = stream_leave(ctx, s)) return rl;
    if (tp && rc == RTW_OK) rc = harvest_timing(ctx, T, opts->timing);
    if (rc) return rc;
    if (!(opts && (opts->flags & RTW_RENDER_NO_SYNC))) HIP_TRY(hipStreamSynchronize(s));
    return RTW_OK;
}

// A GPU context's shard render into the device tile on stream s (the caller holds ctx->mu and has set
// the device and entered the stream): row blocks b with b % n_shards == shard, tile rows in order.
int render_rows_locked(rtw_ctx* ctx, const rtw_camera* cam, uint32_t rpb, uint32_t n_shards, uint32_t shard,
                       uint32_t spp_begin, uint32_t spp_end, uint64_t seed, float* d_tile, hipStream_t s,
                       const rtw_render_opts* opts, uint32_t rows) {
    rtw_launch L = make_launch(ctx, cam, seed);
    L.accum = reinterpret_cast<float4*>(d_tile);
    L.row0 = 0;
    // logical rows 0 .. (the shard's whole blocks); rows past H (or past a balanced shard's share) are masked
    L.n_rows = rtw_shard_tile_rows(cam->image_height, rpb, n_shards, shard);
    L.rpb = rpb;
    L.n_shards = n_shards;
    L.shard = shard;
    L.pix_begin = 0;
    L.pix_end = cam->size;
    set_tiles(L);
    return enqueue_and_finish(ctx, L, spp_begin, spp_end, s, opts, (uint64_t)rows * cam->image_width);
}

}  // namespace

int rtw_stream_enter(rtw_ctx* ctx, hipStream_t s) { return stream_enter(ctx, s); }
int rtw_stream_leave(rtw_ctx* ctx, hipStream_t s) { return stream_leave(ctx, s); }

extern "C" {

int rtw_render(rtw_ctx* ctx, const rtw_camera* cam, uint32_t pix_begin, uint32_t pix_end, uint32_t spp_begin,
               uint32_t spp_end, uint64_t seed, float* accum, const volatile int32_t* cancel,
               rtw_progress_fn progress, void* user) {
    rtw_render_opts o{};
    o.cancel = cancel;
    o.progress = progress;
    o.user = user;
    return rtw_render_ex(ctx, cam, pix_begin, pix_end, spp_begin, spp_end, seed, accum, &o);
}

int rtw_render_ex(rtw_ctx* ctx, const rtw_camera* cam, uint32_t pix_begin, uint32_t pix_end, uint32_t spp_begin,
                  uint32_t spp_end, uint64_t seed, float* accum, const rtw_render_opts* opts) {
    if (!ctx || !accum) return fail(RTW_E_INVALID, "null ctx/accum");
    if (int rc = rtw_validate_cam(cam)) return rc;
    if (int rc = rtw_check_host_opts(opts)) return rc;
    if (pix_end > cam->size || pix_begin > pix_end) return fail(RTW_E_INVALID, "pixel range out of image");
    if (spp_begin > spp_end) return fail(RTW_E_INVALID, "bad sample range");
    if (pix_begin == pix_end || spp_begin == spp_end) return RTW_OK;
    const uint32_t ubatch = opts ? opts->spp_batch : 0u;
    if (ctx->device == RTW_DEVICE_CPU) {  // host context: Camera.render on host threads (rtw_cpu.hip)
        rtw_launch L;
        {
            std::lock_guard<std::mutex> lock(ctx->mu);
            L = make_launch(ctx, cam, seed);
        }
        // the scene image is read-only: concurrent callers (the 8 Tasks) render their ranges at once
        L.n_shards = 0;
        return run_host(ctx, L, pix_begin, pix_end, spp_begin, spp_end, ubatch, accum, opts, pix_end - pix_begin);
    }
    // GPU context.  The context lock is held only while a call enqueues work, never while it waits for
    // the device, so concurrent callers -- the reference's 8 Tasks on disjoint chunks (main.zig:314-326)
    // -- interleave their spp batches on the context's stream and advance samples-outer together, as
    // the 8 workers of camera.zig:98-111 do.  Each call stages only its own chunk of the shared
    // full-frame device buffer, so the chunks never overlap.
    const size_t bytes = (size_t)cam->size * 16;
    const size_t o = (size_t)pix_begin * 16, nb = (size_t)(pix_end - pix_begin) * 16;
    const uint64_t pixels = pix_end - pix_begin;
    hipEvent_t done = nullptr;
    uint32_t batch = 0;
    {
        std::unique_lock<std::mutex> lock(ctx->mu);
        HIP_TRY(hipSetDevice(ctx->device));
        // the staging buffer grows only while no other host-buffer call has a chunk staged in it
        ctx->host_cv.wait(lock, [&] { return ctx->scratch_bytes >= bytes || ctx->host_calls == 0; });
        if (int rc = stream_enter(ctx, ctx->stream)) return rc;
        if (int rc = ensure_scratch(ctx, bytes)) return rc;
        HIP_TRY(hipMemcpyAsync((char*)ctx->d_scratch + o, (char*)accum + o, nb, hipMemcpyHostToDevice, ctx->stream));
        if (int rc = stream_leave(ctx, ctx->stream)) return rc;
        HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));  // (last: no early return leaks it)
        ctx->host_calls++;
        batch = ubatch ? ubatch : rtw_auto_batch(ctx, pixels, spp_end - spp_begin);
    }
    const bool polled = rtw_polled(opts);
    const uint64_t total = pixels * (uint64_t)(spp_end - spp_begin);
    int rc = RTW_OK;
    for (uint32_t s = spp_begin; s < spp_end && rc == RTW_OK; s += batch) {
        if (rtw_stop_requested(opts)) {
            rc = fail(RTW_E_CANCELLED, "cancelled");
            break;
        }
        const uint32_t s_end = (spp_end - s < batch) ? spp_end : s + batch;
        {
            std::lock_guard<std::mutex> lock(ctx->mu);
            if (hipSetDevice(ctx->device) != hipSuccess || stream_enter(ctx, ctx->stream)) {
                rc = fail(RTW_E_HIP, "rtw_render_ex: device");
                break;
            }
            rtw_launch L = make_launch(ctx, cam, seed);
            L.accum = reinterpret_cast<float4*>(ctx->d_scratch);
            L.counters = nullptr;
            set_plain_range(L, pix_begin, pix_end);
            rc = run_batches(ctx, L, s, s_end, s_end - s, ctx->stream, nullptr, pixels);
            if (rc == RTW_OK) rc = stream_leave(ctx, ctx->stream);
            if (rc == RTW_OK && hipEventRecord(done, ctx->stream) != hipSuccess) rc = fail(RTW_E_HIP, "event");
        }
        if (rc == RTW_OK && polled) {  // wait for this batch without the lock, then report it
            if (hipEventSynchronize(done) != hipSuccess) rc = fail(RTW_E_HIP, "rtw_render_ex: batch");
            else if (opts->progress && opts->progress(pixels * (uint64_t)(s_end - spp_begin), total, opts->user))
                rc = fail(RTW_E_CANCELLED, "cancelled by progress callback");
        }
    }
    // copy back whatever was rendered (also on cancel: completed batches are valid)
    hipError_t e;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        e = hipSetDevice(ctx->device);
        if (e == hipSuccess && ctx->last_stream && ctx->last_stream != ctx->stream)
            e = hipStreamWaitEvent(ctx->stream, ctx->last_done, 0);
        if (e == hipSuccess)
            e = hipMemcpyAsync((char*)accum + o, (char*)ctx->d_scratch + o, nb, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(done, ctx->stream);
        if (e == hipSuccess) (void)stream_leave(ctx, ctx->stream);
    }
    if (e == hipSuccess) e = hipEventSynchronize(done);
    (void)hipEventDestroy(done);
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        ctx->host_calls--;
    }
    ctx->host_cv.notify_all();
    if (e != hipSuccess) return rtw_hip_fail(e, "rtw_render copy back");
    return rc;
}

int rtw_render_device(rtw_ctx* ctx, const rtw_camera* cam, uint32_t pix_begin, uint32_t pix_end, uint32_t spp_begin,
                      uint32_t spp_end, uint64_t seed, float* d_accum, void* stream, const rtw_render_opts* opts) {
    if (!ctx || !d_accum) return fail(RTW_E_INVALID, "null ctx/accum");
    if (ctx->device == RTW_DEVICE_CPU) return fail(RTW_E_INVALID, "host context: use rtw_render");
    if (int rc = rtw_validate_cam(cam)) return rc;
    if (pix_end > cam->size || pix_begin > pix_end) return fail(RTW_E_INVALID, "pixel range out of image");
    if (spp_begin > spp_end) return fail(RTW_E_INVALID, "bad sample range");
    if (pix_begin == pix_end || spp_begin == spp_end) return RTW_OK;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (int rc = stream_enter(ctx, s)) return rc;
    rtw_launch L = make_launch(ctx, cam, seed);
    L.accum = reinterpret_cast<float4*>(d_accum);
    set_plain_range(L, pix_begin, pix_end);
    return enqueue_and_finish(ctx, L, spp_begin, spp_end, s, opts, pix_end - pix_begin);
}

uint32_t rtw_shard_rows(uint32_t H, uint32_t rpb, uint32_t n_shards, uint32_t shard) {
    if (!shard_spec_ok(rpb, n_shards, shard)) return 0;
    uint32_t rows = 0;
    const uint32_t t = rtw_shard_tile_rows(H, rpb, n_shards, shard);
    for (uint32_t r = 0; r < t; r++) rows += rtw_shard_row(H, rpb, n_shards, shard, r) < H ? 1u : 0u;
    return rows;
}

uint32_t rtw_shard_image_row(uint32_t rpb, uint32_t n_shards, uint32_t shard, uint32_t tile_row) {
    if (!shard_spec_ok(rpb, n_shards, shard) || (rpb & RTW_ROWS_FLAGS)) return 0xFFFFFFFFu;  // plain shards only
    return rtw_tile_row_image(rpb, n_shards, shard, tile_row);
}

uint32_t rtw_shard_image_row_h(uint32_t H, uint32_t rpb, uint32_t n_shards, uint32_t shard, uint32_t tile_row) {
    if (!shard_spec_ok(rpb, n_shards, shard)) return 0xFFFFFFFFu;
    return rtw_shard_row(H, rpb, n_shards, shard, tile_row);
}

int rtw_render_rows_device(rtw_ctx* ctx, const rtw_camera* cam, uint32_t rpb, uint32_t n_shards, uint32_t shard,
                           uint32_t spp_begin, uint32_t spp_end, uint64_t seed, float* d_tile, void* stream,
                           const rtw_render_opts* opts) {
    if (!ctx || !d_tile) return fail(RTW_E_INVALID, "null ctx/tile");
    if (ctx->device == RTW_DEVICE_CPU) return fail(RTW_E_INVALID, "host context: use rtw_render_rows");
    if (int rc = rtw_validate_cam(cam)) return rc;
    if (!shard_spec_ok(rpb, n_shards, shard)) return fail(RTW_E_INVALID, "bad shard spec");
    if (spp_begin > spp_end) return fail(RTW_E_INVALID, "bad sample range");
    const uint32_t rows = rtw_shard_rows(cam->image_height, rpb, n_shards, shard);
    if (rows == 0 || spp_begin == spp_end) return RTW_OK;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (int rc = stream_enter(ctx, s)) return rc;
    return render_rows_locked(ctx, cam, rpb, n_shards, shard, spp_begin, spp_end, seed, d_tile, s, opts, rows);
}

int rtw_render_rows(rtw_ctx* ctx, const rtw_camera* cam, uint32_t rpb, uint32_t n_shards, uint32_t shard,
                    uint32_t spp_begin, uint32_t spp_end, uint64_t seed, float* tile, const rtw_render_opts* opts) {
    if (!ctx || !tile) return fail(RTW_E_INVALID, "null ctx/tile");
    if (int rc = rtw_validate_cam(cam)) return rc;
    if (int rc = rtw_check_host_opts(opts)) return rc;
    if (!shard_spec_ok(rpb, n_shards, shard)) return fail(RTW_E_INVALID, "bad shard spec");
    if (spp_begin > spp_end) return fail(RTW_E_INVALID, "bad sample range");
    const uint32_t rows = rtw_shard_rows(cam->image_height, rpb, n_shards, shard);
    if (rows == 0 || spp_begin == spp_end) return RTW_OK;
    std::lock_guard<std::mutex> lock(ctx->mu);
    const uint32_t W = cam->image_width;
    if (ctx->device == RTW_DEVICE_CPU) {  // the shard on host threads (rtw_cpu.hip), tile rows in order
        rtw_launch L = make_launch(ctx, cam, seed);
        L.rpb = rpb;
        L.n_shards = n_shards;
        L.shard = shard;
        return run_host(ctx, L, 0, rows * W, spp_begin, spp_end, opts ? opts->spp_batch : 0u, tile, opts,
                        (uint64_t)rows * W);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = stream_enter(ctx, ctx->stream)) return rc;
    // the tile is staged in its own buffer, never in d_scratch: rtw_render_ex calls on this context release
    // the lock between batches with their chunks staged there
    const size_t nb = (size_t)rows * W * 16;
    if (ctx->rows_bytes < nb) HIP_TRY(rtw_device_grow(&ctx->d_rows, &ctx->rows_bytes, nb, nb, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_rows, tile, nb, hipMemcpyHostToDevice, ctx->stream));
    rtw_render_opts ctl{};
    if (opts) ctl = *opts;
    int rc = render_rows_locked(ctx, cam, rpb, n_shards, shard, spp_begin, spp_end, seed, ctx->d_rows, ctx->stream,
                                &ctl, rows);
    hipError_t e = hipMemcpyAsync(tile, ctx->d_rows, nb, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return rtw_hip_fail(e, "rtw_render_rows copy back");
    ctx->last_stream = nullptr;  // synchronised
    return rc;
}

int rtw_texture_from_accum(const float* accum, uint32_t n, uint8_t* out) {
#pragma STDC FP_CONTRACT OFF
    if (!accum || !out) return fail(RTW_E_INVALID, "null buffer");
    for (uint32_t i = 0; i < n; i++) {
        const float* px = accum + 4 * (size_t)i;
        const float scale = 1.0f / px[3];
        for (int k = 0; k < 3; k++) {
            float x = std::sqrt(px[k] * scale);
            if (x < 0.0f) x = 0.0f;
            if (x > 0.999f) x = 0.999f;
            out[4 * (size_t)i + k] = (x == x) ? (uint8_t)(256 * x) : 0;  // NaN (UB in the reference): 0
        }
        out[4 * (size_t)i + 3] = 255;
    }
    return RTW_OK;
}

int rtw_debug_rng(rtw_ctx* ctx, uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, float* out) {
    if (!ctx || !out || n > 64) return fail(RTW_E_INVALID, "bad debug_rng args (n <= 64)");
    if (ctx->device == RTW_DEVICE_CPU) return fail(RTW_E_INVALID, "host context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = stream_enter(ctx, ctx->stream)) return rc;
    ctx->last_stream = nullptr;  // synchronised below
    rtw_launch_debug_rng(seed, pixel, sample, n, ctx->d_dbg, ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctx->d_dbg, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RTW_OK;
}

int rtw_debug_sample(rtw_ctx* ctx, const rtw_camera* cam, uint64_t seed, uint32_t pixel, uint32_t sample,
                     float out[3]) {
    if (!ctx || !out) return fail(RTW_E_INVALID, "null args");
    if (ctx->device == RTW_DEVICE_CPU) return fail(RTW_E_INVALID, "host context");
    if (int rc = rtw_validate_cam(cam)) return rc;
    if (pixel >= cam->size) return fail(RTW_E_INVALID, "pixel out of range");
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = stream_enter(ctx, ctx->stream)) return rc;
    ctx->last_stream = nullptr;  // synchronised below
    rtw_launch L = make_launch(ctx, cam, seed);
    rtw_launch_debug_sample(L, pixel, sample, ctx->d_dbg, ctx->stream);
    HIP_TRY(hipGetLastError());
    float tmp[32];
    HIP_TRY(hipMemcpyAsync(tmp, ctx->d_dbg, sizeof tmp, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    out[0] = tmp[0];
    out[1] = tmp[1];
    out[2] = tmp[2];
    return RTW_OK;
}

int rtw_debug_stripe_counters(rtw_ctx* ctx, uint32_t* stripe_cap, uint32_t* counters) {
    if (!ctx || !stripe_cap || !counters) return fail(RTW_E_INVALID, "null args");
    if (ctx->device == RTW_DEVICE_CPU) return fail(RTW_E_INVALID, "host context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->wf_len || !ctx->d_wf) return fail(RTW_E_INVALID, "no wavefront render yet");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    // (the three sets are consecutive 256-B-aligned takes of run_wavefront's layout)
    std::vector<uint32_t> raw(3u * RTW_WF_STRIPES * RTW_WF_LEN_STRIDE);
    HIP_TRY(hipMemcpy(raw.data(), ctx->wf_len, raw.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < 3u * RTW_WF_STRIPES; k++) counters[k] = raw[(size_t)k * RTW_WF_LEN_STRIDE];
    *stripe_cap = ctx->wf_stripe_cap;
    return RTW_OK;
}

int rtw_debug_tile_lists(rtw_ctx* ctx, const rtw_camera* cam, uint32_t pix_begin, uint32_t pix_end, uint32_t builder,
                         uint32_t cap, uint32_t* n_tiles, uint32_t* n_tx, uint32_t* row0, uint32_t* counts,
                         uint32_t* entries, uint32_t tiles_cap) {
    if (!ctx || !n_tiles || !n_tx || !row0) return fail(RTW_E_INVALID, "null args");
    if (ctx->device == RTW_DEVICE_CPU) return fail(RTW_E_INVALID, "host context");
    if (int rc = rtw_validate_cam(cam)) return rc;
    if (pix_end > cam->size || pix_begin >= pix_end) return fail(RTW_E_INVALID, "pixel range empty or out of image");
    if (builder > 2 || (cap && (cap < 2 || cap > RTW_TL_MAX)))
        return fail(RTW_E_INVALID, "rtw_debug_tile_lists: builder is 0..2, cap 0 or 2..128");
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (int rc = stream_enter(ctx, s)) return rc;
    ctx->last_stream = nullptr;  // synchronised below
    // the launch and the batch's tiles as rtw_render_device makes them
    rtw_launch L = make_launch(ctx, cam, 0);
    set_plain_range(L, pix_begin, pix_end);
    rtw_wf W{};
    const uint64_t n_pix = wf_tile_grid(L, W);
    const uint64_t tiles = n_pix / 64;
    W.n_pix = (uint32_t)n_pix;
    *n_tiles = (uint32_t)tiles;
    *n_tx = W.n_tx;
    *row0 = L.row0;
    wf_tile_buffer(ctx, L, W, n_pix, s);
    if (!W.tl_count) return fail(RTW_E_INVALID, "rtw_debug_tile_lists: the context renders without tile lists");
    if (tiles > tiles_cap || !counts || !entries) return fail(RTW_E_INVALID, "rtw_debug_tile_lists: tiles_cap too small");
    if (cap) L.tile_lists = cap;
    // a slot no builder wrote reads back as id 0xFFFFFFFF
    HIP_TRY(hipMemsetAsync(ctx->d_tl, 0xFF, tiles * RTW_TL_BYTES, s));
    if (!rtw_wavefront_tile_lists(L, W, s, builder))
        return fail(RTW_E_INVALID, "rtw_debug_tile_lists: the scene class renders without tile lists");
    HIP_TRY(hipGetLastError());
    const size_t row = (size_t)L.tile_lists * 32;
    HIP_TRY(hipMemcpyAsync(counts, W.tl_count, tiles * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpy2DAsync(entries, row, W.tl, (size_t)RTW_TL_MAX * 32, row, tiles, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RTW_OK;
}

}  // extern "C"
