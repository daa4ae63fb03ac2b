// rtw_query.hip -- ray queries (include/rtw_gpu.h, DESIGN.md §Ray queries): the closest hit, or whether anything is
// hit, for rays the caller supplies.  Kernels of their own: no render kernel, class table or launch is touched.
//
// One RTW_DHD function per query, run by a gfx950 kernel (one lane per ray, blocks of 256; a ray is two 16-B loads, a
// hit four 16-B stores, an occlusion flag one byte) and by the host backend's threads -- the walk (order_of,
// order_base, ray_trav, trav_step<FEAT>) and the hit record (hit_prep<FEAT>) of every render's first bounce, the same
// fp32 operations in the same order, so a GPU context and a host context agree bit for bit.
//
// What differs from traverse<FEAT>:
//   * `closest` starts at the ray's tmax.  Quad.hit's interval is closed (a quad at t == closest is accepted, as in
//     the reference), so a hit that is not < tmax is dropped again: the caller's interval is open at tmax for every
//     primitive.  A dropped hit leaves closest at tmax, so nothing it could have hidden is lost.
//   * the FMA slab test (fast_box) is conservative for origins with |o| <= 7 extent only.  A render decides that per
//     camera (make_launch); a query decides it per ray: a lane whose origin lies further out (or is NaN) walks with
//     the launch's copy Lx, fast_box = 0 -- aabb.zig's box arithmetic, no instance-box cull.  Both walks find the
//     same closest hit.  The copy is wave-uniform (SGPRs).  In the source the two walks are two calls of query_walk;
//     what the compiler makes of them (one loop with a per-lane select of the box test, at the time of writing) is
//     its business: profiles/queries/.
//   * the any-hit walk stops at the first accepted hit and builds no record.
// The compact 16-B walk is not used: it has no tmax form, and the classes here (every feature but the media) never
// take it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtw_device.h"

namespace {

// (the query classes: RtwFirstHitClasses, rtw_internal.h)
// rtw_ray as two float4: (origin, tmax), (dir, time)
RTW_DHD Ray query_ray(float4 a, float4 b) {
    Ray r;
    r.o = mk(a.x, a.y, a.z);
    r.d = mk(b.x, b.y, b.z);
    r.time = b.w;
    return r;
}
// does the origin lie where the FMA slab test is conservative?  (false for a NaN component)
RTW_DHD bool query_near(const Ray& r, float reach) {
    const float om = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(r.o.x), __builtin_fabsf(r.o.y)), __builtin_fabsf(r.o.z));
    return om <= reach && r.o.x == r.o.x && r.o.y == r.o.y && r.o.z == r.o.z;
}

// traverse<FEAT>'s non-compact form on (0.001, tmax); ANY: stops at the first accepted hit
template <uint32_t FEAT, bool ANY>
RTW_DHD int query_walk(const rtw_launch& L, const Ray& r, float tmax, float& t_out) {
    const uint32_t oct = order_of(L, r);
    const float4* nodes = order_base(L.nodes, L, oct);
    const RayTrav rt = ray_trav(r, L.fast_box != 0);
    float closest = tmax;
    int hit = -1;
    uint32_t i = 0;
    const uint32_t n = L.n_nodes;
    Counters cnt;
    if constexpr (ANY) {
        while (i < n && hit < 0) {
            i = trav_step<FEAT>(nodes, L, r, rt, i, closest, hit, cnt, 0);
            if (hit >= 0 && !(closest < tmax)) hit = -1;  // a quad at t == tmax (closest is still tmax)
        }
    } else {
        while (i < n) i = trav_step<FEAT>(nodes, L, r, rt, i, closest, hit, cnt, 0);
        if (hit >= 0 && !(closest < tmax)) hit = -1;
    }
    t_out = closest;
    return hit_with_order(hit, oct);
}

// the walk of one ray with the per-ray choice of the box test; -1: a miss
template <uint32_t FEAT, bool ANY>
RTW_DHD int query_hit(const rtw_launch& L, const rtw_launch& Lx, float reach, const Ray& r, float tmax, float& t) {
    if (!(tmax > kTmin)) return -1;  // an empty interval; a NaN tmax
    if (L.fast_box && !query_near(r, reach)) return query_walk<FEAT, ANY>(Lx, r, tmax, t);
    return query_walk<FEAT, ANY>(L, r, tmax, t);
}

// rtw_hit as four float4
struct QueryHit {
    float4 w[4];
};
RTW_DHD float4 f4u(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return make_float4(ubits(a), ubits(b), ubits(c), ubits(d)); }

template <uint32_t FEAT>
RTW_DHD QueryHit query_closest(const rtw_launch& L, const rtw_launch& Lx, float reach, float4 ra, float4 rb) {
    const Ray r = query_ray(ra, rb);
    float t;
    const int hit = query_hit<FEAT, false>(L, Lx, reach, r, ra.w, t);
    QueryHit q;
    if (hit < 0) {
        q.w[0] = f4u(fbits(kInf), RTW_HIT_NONE, RTW_HIT_NONE, RTW_HIT_NONE);
        q.w[1] = q.w[2] = f4u(0, 0, 0, 0);
        q.w[3] = f4u(0, 0, RTW_HIT_NONE, RTW_HIT_NONE);
        return q;
    }
    // the leaf of the hit id (hit_prep's decoding) names the object; an instance's member names the primitive
    const float4* nodes = L.nodes;
    uint32_t id = (uint32_t)hit;
    if (L.n_orders > 1) {
        nodes = order_base(nodes, L, id >> RTW_HIT_NODE_BITS);
        id &= (1u << RTW_HIT_NODE_BITS) - 1u;
    }
    const uint32_t nbits = hit_node_bits<FEAT>(L);
    const uint32_t node = id & ((1u << nbits) - 1u), sub = id >> nbits;
    const float4 B = nodes[2 * node + 1];
    const uint32_t kind = RTW_LEAF_KIND(fbits(B.w)), index = fbits(B.z);
    uint32_t member = RTW_HIT_NONE, prim_kind = kind, prim_index = index, mat = fbits(B.y);
    if (kind == RTW_OBJ_INSTANCE) {
        const uint32_t ref = L.members[L.insts[index].first + sub];
        member = sub;
        prim_kind = RTW_REF_KIND(ref);
        prim_index = RTW_REF_INDEX(ref);
        mat = prim_kind == RTW_OBJ_SPHERE ? L.sph[prim_index].mat : RTW_QUAD_MAT(L.quads[prim_index].mat);
    }
    const HitPrep h = hit_prep<FEAT>(L.nodes, L, r, hit, t);
    float u = h.uv.u, v = h.uv.v;
    if (!h.uv.set) sphere_uv(h.uv.outward, u, v);  // a top-level sphere: the render computes it lazily
    q.w[0] = make_float4(t, ubits(kind), ubits(index), ubits(member));
    q.w[1] = make_float4(h.p.x, h.p.y, h.p.z, ubits(mat));
    q.w[2] = make_float4(h.normal.x, h.normal.y, h.normal.z, ubits(h.front ? 1u : 0u));
    q.w[3] = make_float4(u, v, ubits(prim_kind), ubits(prim_index));
    return q;
}

template <uint32_t FEAT>
RTW_DHD uint8_t query_any(const rtw_launch& L, const rtw_launch& Lx, float reach, float4 ra, float4 rb) {
    float t;
    return query_hit<FEAT, true>(L, Lx, reach, query_ray(ra, rb), ra.w, t) >= 0 ? 1 : 0;
}

// the launch's copy with the exact box arithmetic
RTW_DHD rtw_launch exact_box(const rtw_launch& L) {
    rtw_launch Lx = L;
    Lx.fast_box = 0;
    return Lx;
}

// one lane per ray; n <= 2^32 - 1, so the index is formed in 64 bits (the last block may start at 2^32 - 256)
template <uint32_t FEAT>
__global__ __launch_bounds__(256) void query_closest_kernel(rtw_launch L, float reach, uint64_t n, const float4* rays,
                                                            float4* hits) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const rtw_launch Lx = exact_box(L);
    const QueryHit q = query_closest<FEAT>(L, Lx, reach, rays[2 * i], rays[2 * i + 1]);
    hits[4 * i] = q.w[0];
    hits[4 * i + 1] = q.w[1];
    hits[4 * i + 2] = q.w[2];
    hits[4 * i + 3] = q.w[3];
}

template <uint32_t FEAT>
__global__ __launch_bounds__(256) void query_any_kernel(rtw_launch L, float reach, uint64_t n, const float4* rays,
                                                        uint8_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const rtw_launch Lx = exact_box(L);
    out[i] = query_any<FEAT>(L, Lx, reach, rays[2 * i], rays[2 * i + 1]);
}

// the scene's launch without a camera, and the reach of the FMA slab test
rtw_launch query_launch(const rtw_ctx* ctx, float& reach) {
    rtw_launch L = ctx->base;
    L.counters = nullptr;
    reach = 7.0f * ctx->extent;
    return L;
}

// 0: go on; 1: nothing to do (n == 0); else the refusal
int check_args(const char* what, const rtw_ctx* ctx, uint64_t n, const void* rays, const void* out) {
    char msg[128];
    if (!ctx) {
        std::snprintf(msg, sizeof msg, "%s: null ctx", what);
        return rtw_invalid(msg);
    }
    if (n > 0xFFFFFFFFull) {
        std::snprintf(msg, sizeof msg, "%s: more than 2^32 - 1 rays", what);
        return rtw_invalid(msg);
    }
    if (n == 0) return 1;
    if (!rays || !out) {
        std::snprintf(msg, sizeof msg, "%s: null rays / output", what);
        return rtw_invalid(msg);
    }
    return RTW_OK;
}

// both device entry points: ANY picks the kernel and the output's element
template <bool ANY>
int query_device(const char* what, rtw_ctx* ctx, uint64_t n, const rtw_ray* d_rays, void* d_out, void* stream,
                 uint32_t flags) {
    if (ctx && ctx->device == RTW_DEVICE_CPU) return rtw_invalid("host context: use the host-buffer entry point");
    if (flags & ~(uint32_t)RTW_RENDER_NO_SYNC) return rtw_invalid("ray query: unknown flag bits");
    if (const int rc = check_args(what, ctx, n, d_rays, d_out)) return rc == 1 ? RTW_OK : rc;
    // the kernels read rays and write hits as float4 (the occlusion flags are bytes)
    if (((uintptr_t)d_rays | (ANY ? 0 : (uintptr_t)d_out)) & 15) return rtw_invalid("ray query: device rays / hits not 16-byte aligned");
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (int rc = rtw_stream_enter(ctx, s)) return rc;
    float reach;
    const rtw_launch L = query_launch(ctx, reach);
    const dim3 grid((uint32_t)((n + 255) / 256));
    const float4* rays = reinterpret_cast<const float4*>(d_rays);
    RtwFirstHitClasses::visit(rtw_first_hit_class(L), [&](auto c) {
        if constexpr (ANY)
            hipLaunchKernelGGL(query_any_kernel<decltype(c)::value>, grid, dim3(256), 0, s, L, reach, n, rays,
                               static_cast<uint8_t*>(d_out));
        else
            hipLaunchKernelGGL(query_closest_kernel<decltype(c)::value>, grid, dim3(256), 0, s, L, reach, n, rays,
                               static_cast<float4*>(d_out));
    });
    HIP_TRY(hipGetLastError());
    if (int rc = rtw_stream_leave(ctx, s)) return rc;
    if (!(flags & RTW_RENDER_NO_SYNC)) HIP_TRY(hipStreamSynchronize(s));
    return RTW_OK;
}

// both host-buffer entry points
template <bool ANY>
int query_host(const char* what, rtw_ctx* ctx, uint64_t n, const rtw_ray* rays, void* out) {
    if (const int rc = check_args(what, ctx, n, rays, out)) return rc == 1 ? RTW_OK : rc;
    if (ctx->device == RTW_DEVICE_CPU) {
        // a host caller's records need only the alignment of their floats: they are copied to and from float4
        // the lock is held for the whole batch, as rtw_render_guides holds it: the registrations take it too
        std::lock_guard<std::mutex> lock(ctx->mu);
        float reach;
        const rtw_launch L = query_launch(ctx, reach);
        const rtw_launch Lx = exact_box(L);
        RtwFirstHitClasses::visit(rtw_first_hit_class(L), [&](auto c) {
            constexpr uint32_t FEAT = decltype(c)::value;
            rtw_host_ranges(n, ctx->cpu_threads, 64, [&](uint64_t i0, uint64_t i1) {  // chunks of at least 64 rays
                for (uint64_t i = i0; i < i1; i++) {
                    float4 r[2];
                    std::memcpy(r, rays + i, sizeof r);
                    if constexpr (ANY) {
                        static_cast<uint8_t*>(out)[i] = query_any<FEAT>(L, Lx, reach, r[0], r[1]);
                    } else {
                        const QueryHit q = query_closest<FEAT>(L, Lx, reach, r[0], r[1]);
                        std::memcpy(static_cast<rtw_hit*>(out) + i, q.w, sizeof q.w);
                    }
                }
            });
        });
        return RTW_OK;
    }
    // GPU context: rays and results through a device staging block of this call's
    const size_t in_bytes = (size_t)n * sizeof(rtw_ray), out_bytes = (size_t)n * (ANY ? 1 : sizeof(rtw_hit));
    char* d = nullptr;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), in_bytes + out_bytes));
    }
    hipError_t e = hipMemcpy(d, rays, in_bytes, hipMemcpyHostToDevice);
    int rc = RTW_OK;
    if (e == hipSuccess) rc = query_device<ANY>(what, ctx, n, reinterpret_cast<const rtw_ray*>(d), d + in_bytes, nullptr, 0);
    if (e == hipSuccess && rc == RTW_OK) e = hipMemcpy(out, d + in_bytes, out_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return rtw_hip_fail(e, "ray query staging");
    return rc;
}

}  // namespace

static_assert(sizeof(rtw_ray) == 32 && sizeof(rtw_hit) == 64, "rtw_ray / rtw_hit are two / four 16-B words");

extern "C" {

int rtw_trace_rays(rtw_ctx* ctx, uint64_t n, const rtw_ray* rays, rtw_hit* hits) {
    return query_host<false>("rtw_trace_rays", ctx, n, rays, hits);
}
int rtw_trace_rays_device(rtw_ctx* ctx, uint64_t n, const rtw_ray* d_rays, rtw_hit* d_hits, void* stream, uint32_t flags) {
    return query_device<false>("rtw_trace_rays_device", ctx, n, d_rays, d_hits, stream, flags);
}
int rtw_occluded(rtw_ctx* ctx, uint64_t n, const rtw_ray* rays, uint8_t* out) {
    return query_host<true>("rtw_occluded", ctx, n, rays, out);
}
int rtw_occluded_device(rtw_ctx* ctx, uint64_t n, const rtw_ray* d_rays, uint8_t* d_out, void* stream, uint32_t flags) {
    return query_device<true>("rtw_occluded_device", ctx, n, d_rays, d_out, stream, flags);
}

}  // extern "C"
