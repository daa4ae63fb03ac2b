// rtw_cpu.hip -- the host backend of the C ABI (rtw_scene_create(desc, RTW_DEVICE_CPU, ...)):
// Camera.render (src/camera.zig:93-116) on host threads, for machines without a GPU and for the
// reference's own CPU configuration (BASELINE config 1: 400x225, 10 spp, the 8-thread path of
// src/main.zig:314-326).
//
// Not a fallback: a context is a host context only when the caller asks for one, and a GPU
// context never runs here.  Each sample is sample_radiance() of rtw_device.h -- the very
// function the GPU's v0 kernel runs per lane, compiled for the host -- so a host render is
// bit-identical to the GPU's (same fp32 operations: correctly rounded division and sqrt, the
// restated pow / acos / atan2 / sin / log, the counter-based RNG; a host context walks the
// exact aabb.zig slab test and the IEEE sphere test, which the GPU's fast paths reproduce
// bit for bit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtw_device.h"
#include "rtw_wavefront.h"

namespace {
// Pixels [a, b) of a chunk with the sample loop of class F (rtw_with_class: the instantiation the GPU kernels run)
template <uint32_t F>
void cpu_pixels(const rtw_launch& L, uint32_t a, uint32_t b, float* out, const rtw_render_opts* stop,
                std::atomic<bool>& stopped) {
    Counters cnt;
    for (uint32_t i = a; i < b; i++) {
        if (rtw_stop_requested(stop)) {  // polled per pixel, as Camera.render polls `running` (camera.zig:107)
            stopped = true;
            return;
        }
        const uint32_t x = i % L.W;
        uint32_t y = i / L.W;
        if (L.n_shards && !map_row(L, y, y)) continue;  // a shard's logical row -> image row (rows past H: none)
        if (y >= L.H) continue;
        const uint32_t pixel = y * L.W + x;
        float* px = out + 4 * (size_t)i;
        float r = px[0], g = px[1], bl = px[2];
        for (uint32_t s = L.s0; s < L.s1; s++) {
            const f3 c = sample_radiance<F>(L.nodes, L, pixel, x + L.pixel_offset, y + L.pixel_offset, s, cnt);
            r += c.x;
            g += c.y;
            bl += c.z;
        }
        px[0] = r;
        px[1] = g;
        px[2] = bl;
        px[3] = (float)L.s1;  // writeColor: number_of_samples (camera.zig:56)
    }
}
}  // namespace

int rtw_cpu_render(const rtw_launch& L, uint32_t begin, uint32_t end, float* out, uint32_t threads,
                   const rtw_render_opts* stop) {
    std::atomic<bool> stopped{false};
    // the class once per call: instance trees, registered lights (the mixture-density instantiations) and vertex
    // attributes (always with the trees') select it as they do on the GPU
    decltype(&cpu_pixels<RTW_F_ALL>) pixels = nullptr;
    rtw_with_class<false>(rtw_feat_of(L), [&](auto c) { pixels = cpu_pixels<decltype(c)::value>; });
    // contiguous chunks, as startRender's Tasks (main.zig:318-324); samples in order per pixel
    rtw_host_ranges(end - begin, threads, 1, [&](uint64_t a, uint64_t b) {
        pixels(L, begin + (uint32_t)a, begin + (uint32_t)b, out, stop, stopped);
    });
    return stopped ? RTW_E_CANCELLED : RTW_OK;
}

// Host-only test hook (include/rtw_gpu.h), and the symbol a caller detects stratified pixel samples by: get_ray --
// the device's code, the same fp32 operations, the path's own RNG stream -- for n (pixel, sample) pairs
namespace {
Ray debug_get_ray(const rtw_launch& L, uint32_t pixel, uint32_t s, float* jit) {
    rtw_rng rng;
    rng.s = rtw_mix64(L.key0 ^ (((uint64_t)pixel << 32) | (uint64_t)s));  // sample_radiance's stream
    return get_ray(L, pixel % L.W + L.pixel_offset, pixel / L.W + L.pixel_offset, stratum_of(L.strata, s), rng, jit);
}
}  // namespace
extern "C" int rtw_debug_camera_ray(const rtw_camera* cam, uint64_t seed, uint32_t n, const uint32_t* pixels,
                                    const uint32_t* samples, float* origin, float* dir, float* time, float* jitter) {
    if (int rc = rtw_validate_cam(cam)) return rc;
    if (n && (!pixels || !samples)) {
        rtw_set_error("rtw_debug_camera_ray: null pixels / samples");
        return RTW_E_INVALID;
    }
    rtw_launch L{};
    rtw_launch_camera(L, cam, seed);
    for (uint32_t i = 0; i < n; i++) {
        if (pixels[i] >= cam->size) {
            char msg[96];
            std::snprintf(msg, sizeof msg, "rtw_debug_camera_ray: pair %u: pixel %u out of range", i, pixels[i]);
            rtw_set_error(msg);
            return RTW_E_INVALID;
        }
        float jit[2];
        const Ray r = debug_get_ray(L, pixels[i], samples[i], jit);
        const float o[3] = {r.o.x, r.o.y, r.o.z}, d[3] = {r.d.x, r.d.y, r.d.z};
        for (int k = 0; k < 3; k++) {
            if (origin) origin[3 * (size_t)i + k] = o[k];
            if (dir) dir[3 * (size_t)i + k] = d[k];
        }
        if (time) time[i] = r.time;
        if (jitter) {
            jitter[2 * (size_t)i] = jit[0];
            jitter[2 * (size_t)i + 1] = jit[1];
        }
    }
    return RTW_OK;
}

// ABI 6 test hook (include/rtw_gpu.h): the walk's sphere fast-reject against Sphere.hit's exact accept, on
// the host -- sphere_may_hit is the device's code (rtw_device.h), the same fp32 operations
extern "C" int rtw_debug_sphere_filter(uint32_t n, const float* a, const float* half_b, const float* c,
                                       const float* closest, uint8_t* may_hit, uint8_t* accept) {
    if (n && (!a || !half_b || !c || !closest || !may_hit || !accept)) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        // the ray constants as ray_trav derives them from a (fast_reject on)
        const float aa = a[i], hb = half_b[i];
        const bool in_range = aa >= 0x1p-40f && aa <= 0x1p40f;
        const float tk = aa * 0.001f, ktk = tk * 9.5367432e-07f, gk = in_range ? 0.99999905f : 0.0f;
        const float disc = hb * hb - aa * c[i];
        may_hit[i] = sphere_may_hit(hb, disc, aa, closest[i], tk, ktk, gk) ? 1 : 0;
        // Sphere.hit (objects.zig:127-136): nearest root in the open interval (0.001, closest)
        bool ok = false;
        if (disc >= 0) {
            const float sq = std::sqrt(disc);
            float root = (-hb - sq) / aa;
            ok = 0.001f < root && root < closest[i];
            if (!ok) {
                root = (-hb + sq) / aa;
                ok = 0.001f < root && root < closest[i];
            }
        }
        accept[i] = ok ? 1 : 0;
    }
    return RTW_OK;
}

// Host-only test hook (include/rtw_gpu.h), and the symbol a caller detects triangles by: Quad.init's derivation
// (rtw_quad_init, the scene builder's) and quad_t / quad_prep -- the device's code, the same fp32 operations --
// for n (record, ray) pairs
namespace {
// (inside the namespace of rtw_device.h: at file scope its quad_t meets <sys/types.h>'s)
bool debug_quad_t(const rtw_dev_quad& q, const Ray& r, float tmin, float tmax, float& t) {
    return quad_t(q, r, tmin, tmax, t);
}
}  // namespace
extern "C" int rtw_debug_quad_hit(uint32_t n, const rtw_quad* quads, const float* origins, const float* dirs,
                                  const float* tmin, const float* tmax, uint8_t* hit, float* t, float* alpha_beta) {
    if (n && (!quads || !origins || !dirs || !tmin || !tmax || !hit || !t || !alpha_beta)) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        if (quads[i].shape > RTW_QUAD_TRIANGLE) {
            char msg[96];
            std::snprintf(msg, sizeof msg, "rtw_debug_quad_hit: quad %u: unknown shape %u", i, quads[i].shape);
            rtw_set_error(msg);
            return RTW_E_INVALID;
        }
        rtw_dev_quad q;
        rtw_quad_init(quads[i], q);
        Ray r;
        r.o = ld3(origins + 3 * (size_t)i);
        r.d = ld3(dirs + 3 * (size_t)i);
        r.time = 0.0f;
        float tt;
        hit[i] = debug_quad_t(q, r, tmin[i], tmax[i], tt) ? 1 : 0;
        if (hit[i]) {
            HitPrep h;
            quad_prep(q, r, tt, h);
            t[i] = tt;
            alpha_beta[2 * (size_t)i] = h.uv.u;
            alpha_beta[2 * (size_t)i + 1] = h.uv.v;
        }
    }
    return RTW_OK;
}

// Host-only test hook (include/rtw_gpu.h), and the symbol a caller detects vertex attributes by: the hit record of
// (record, attribute, ray, t) -- rtw_quad_init, quad_prep and quad_attr, the device's code, the same fp32 operations
extern "C" int rtw_debug_quad_shade(uint32_t n, const rtw_quad* quads, const rtw_vertex_attr* attrs,
                                    const float* origins, const float* dirs, const float* t, float* normal, float* uv,
                                    uint8_t* front) {
    if (n && (!quads || !attrs || !origins || !dirs || !t || !normal || !uv || !front)) return RTW_E_INVALID;
    char msg[96];
    for (uint32_t i = 0; i < n; i++) {
        if (quads[i].shape > RTW_QUAD_TRIANGLE) {
            std::snprintf(msg, sizeof msg, "rtw_debug_quad_shade: quad %u: unknown shape %u", i, quads[i].shape);
            rtw_set_error(msg);
            return RTW_E_INVALID;
        }
        if (attrs[i].flags & ~(uint32_t)(RTW_ATTR_NORMALS | RTW_ATTR_UVS)) {
            std::snprintf(msg, sizeof msg, "rtw_debug_quad_shade: attribute %u: unknown flag bits 0x%x", i,
                          attrs[i].flags);
            rtw_set_error(msg);
            return RTW_E_INVALID;
        }
        rtw_dev_quad q;
        rtw_quad_init(quads[i], q);
        rtw_vertex_attr a = attrs[i];
        if ((a.flags & RTW_ATTR_NORMALS) && !rtw_vattr_normalise(attrs[i], a)) {
            std::snprintf(msg, sizeof msg, "rtw_debug_quad_shade: attribute %u: a normal is not finite or has zero "
                          "length", i);
            rtw_set_error(msg);
            return RTW_E_INVALID;
        }
        rtw_dev_vattr va;
        std::memcpy(&va, &a, sizeof va);
        Ray r;
        r.o = ld3(origins + 3 * (size_t)i);
        r.d = ld3(dirs + 3 * (size_t)i);
        r.time = 0.0f;
        HitPrep h;
        quad_prep(q, r, t[i], h);
        quad_attr(&va, h);
        normal[3 * (size_t)i] = h.normal.x;
        normal[3 * (size_t)i + 1] = h.normal.y;
        normal[3 * (size_t)i + 2] = h.normal.z;
        uv[2 * (size_t)i] = h.uv.u;
        uv[2 * (size_t)i + 1] = h.uv.v;
        front[i] = h.front ? 1 : 0;
    }
    return RTW_OK;
}

// Host-only test hook (include/rtw_gpu.h), and a symbol a caller detects environment maps by: env_texel,
// env_radiance, env_pdf and env_sample -- the device's code, the same fp32 operations -- on the context's host copy
// of the registered block (a GPU context keeps one too)
extern "C" int rtw_debug_environment(rtw_ctx* ctx, uint32_t n, const float* dirs, const float* draws, float* radiance,
                                     float* pdf, float* sampled_dir, uint32_t* texel) {
    if (!ctx) {
        rtw_set_error("null ctx");
        return RTW_E_INVALID;
    }
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (ctx->env_block.empty()) {
        rtw_set_error("rtw_debug_environment: no environment is registered");
        return RTW_E_INVALID;
    }
    const rtw_dev_env& e = *reinterpret_cast<const rtw_dev_env*>(ctx->env_block.data());
    for (uint32_t i = 0; i < n; i++) {
        if (dirs) {
            const f3 d = ld3(dirs + 3 * (size_t)i);
            float st;
            const uint32_t t = env_texel(e, d, st);
            if (texel) texel[i] = t;
            if (radiance) {
                const f3 c = env_radiance(e, d);
                radiance[3 * (size_t)i] = c.x;
                radiance[3 * (size_t)i + 1] = c.y;
                radiance[3 * (size_t)i + 2] = c.z;
            }
            if (pdf) pdf[i] = e.sampled ? env_pdf(e, d) : 0.0f;
        }
        if (draws && sampled_dir) {
            f3 s = mk(0, 0, 0);
            if (e.sampled) s = env_sample(e, draws[2 * (size_t)i], draws[2 * (size_t)i + 1]);
            sampled_dir[3 * (size_t)i] = s.x;
            sampled_dir[3 * (size_t)i + 1] = s.y;
            sampled_dir[3 * (size_t)i + 2] = s.z;
        }
    }
    return RTW_OK;
}

// Host-only test hook (include/rtw_gpu.h): the slot arithmetic of the bucketed push's LDS cursors
// (rtw_wavefront.h wf_cursor_*, the device's code) for n pushing lanes
extern "C" int rtw_debug_push_cursor(uint32_t n, const uint32_t* blk, const uint32_t* old, const uint32_t* fresh,
                                     uint32_t* slot, uint32_t* over, uint32_t* rebase) {
    if (n && (!blk || !old || !fresh || !slot || !over || !rebase)) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        over[i] = wf_cursor_over(blk[i], old[i]);
        slot[i] = wf_cursor_slot(blk[i], old[i], fresh[i]);
        rebase[i] = wf_cursor_rebase(blk[i], fresh[i]);
    }
    return RTW_OK;
}
