// rtw_denoise.hip -- denoised previews (include/rtw_gpu.h, DESIGN.md §Denoised previews): first-hit guide buffers
// (albedo, normal + depth) and the edge-avoiding a-trous wavelet filter of Dammertz et al. 2010 over the
// accumulator's mean radiance.  Kernels of their own: no render kernel, class table or launch is touched.
//
// One RTW_DHD function per step, run by a gfx950 kernel (one lane per pixel, blocks of 32 x 8 pixels: a wave row
// reads 32 x 16 B = 512 contiguous bytes per tap row) and by the host backend's threads -- the same fp32
// operations in the same order (-ffp-contract=off, correctly rounded division, rtw_expneg of rtw_libm.h), so a GPU
// context and a host context agree bit for bit.
//
// The filter's association (the header states it for callers):
//   pre-pass   inv = 1 / w;  c = (r inv, g inv, b inv);  demodulated: c.k = c.k / a.k, a.k = albedo.k > 2^-8 ?
//              albedo.k : 2^-8.  The plane keeps w in its fourth channel.
//   pass i     taps dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = p + 2^i (dx, dy); skipped off the image, where
//              c_q is not finite, where (depth_q > 0) != (depth_p > 0);
//                tc = kc > 0 ? ((dr dr + dg dg) + db db) kc : 0      (kc = 0 where c_p is not finite)
//                tn = kn > 0 ? ((dx dx + dy dy) + dz dz) kn : 0      (d = n_q - n_p)
//                tz = kz > 0 ? ((z_q - z_p) (z_q - z_p)) kz : 0      (kz = 1 / (sd2 (z_p z_p)), hit centre, sd2 > 0)
//                wgt = (h[dx] h[dy]) e((tc + tn) + tz);  sum.k += wgt c_q.k;  wsum += wgt
//              c' = wsum > 0 ? sum.k / wsum : c_p
//              kc = 1 / (sc sc), sc = sigma_color 2^-i;  kn = 1 / (sn sn);  sd2 = sd sd: once per pass on the host.
//   last pass  c'.k = c'.k a.k (demodulated);  out = (c'.r w, c'.g w, c'.b w, w)
// A pass reads two 16-B planes and writes one, and the planes of a frame sit in the Infinity Cache.  The passes
// with spacing 1 and 2 take their taps from an LDS tile (below), the wider ones through L1 / L2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtw_device.h"

namespace {

// ---------------------------------------------------------------------------
// Guides
// ---------------------------------------------------------------------------
// (the guide classes: RtwFirstHitClasses and, with an environment registered, RtwGuideEnvClasses, rtw_internal.h)
// The guides of pixel (x, y): Camera.getRay's pixel centre (pixel_center) without the jitter, from the
// camera centre, time 0; traverse / hit_prep as every render's first bounce
template <uint32_t FEAT>
RTW_DHD void guide_pixel(const rtw_launch& L, uint32_t x, uint32_t y, float4& albedo, float4& nd) {
    Ray r;
    r.o = ld3(L.center);
    r.d = pixel_center(L, x + L.pixel_offset, y + L.pixel_offset) - r.o;
    r.time = 0.0f;
    Counters cnt;
    float t;
    const int hit = traverse<FEAT>(L.nodes, L, r, t, cnt, 0);
    if (hit < 0) {
        const f3 bg = background<FEAT>(L, r);
        albedo = make_float4(bg.x, bg.y, bg.z, 0.0f);
        nd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const HitPrep h = hit_prep<FEAT>(L.nodes, L, r, hit, t);
    f3 a;
    switch (h.m.kind) {
    case RTW_MAT_METAL: a = ld3(h.m.albedo); break;
    case RTW_MAT_DIELECTRIC: a = mk(1, 1, 1); break;
    default: a = texture_value<FEAT>(L, h.m.texture, h.uv, h.p); break;  // Lambertian, DiffuseLight (Isotropic)
    }
    albedo = make_float4(a.x, a.y, a.z, 1.0f);
    nd = make_float4(h.normal.x, h.normal.y, h.normal.z, t * __builtin_sqrtf(length_squared(r.d)));
}

template <uint32_t FEAT>
__global__ __launch_bounds__(256) void guides_kernel(rtw_launch L, float4* albedo, float4* nd) {
    const uint32_t x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= L.W || y >= L.H) return;
    float4 a, n;
    guide_pixel<FEAT>(L, x, y, a, n);
    const size_t p = (size_t)y * L.W + x;
    albedo[p] = a;
    nd[p] = n;
}

template <uint32_t FEAT>
void guides_rows(const rtw_launch& L, uint32_t y0, uint32_t y1, float4* albedo, float4* nd) {
    for (uint32_t y = y0; y < y1; y++)
        for (uint32_t x = 0; x < L.W; x++) {
            const size_t p = (size_t)y * L.W + x;
            guide_pixel<FEAT>(L, x, y, albedo[p], nd[p]);
        }
}

dim3 pixel_grid(uint32_t W, uint32_t H) { return dim3((W + 31) / 32, (H + 7) / 8); }

// ---------------------------------------------------------------------------
// Filter
// ---------------------------------------------------------------------------
struct DnPass {
    const float4* src;     // the pass's input plane (c.rgb, w)
    const float4* nd;      // normal + depth
    const float4* albedo;  // null unless demodulating
    float4* dst;           // the other plane, or `out` in the last pass
    uint32_t W, H;
    int32_t s;             // tap spacing 2^i
    float kc, kn, sd2;     // 0: term off
    uint32_t last, demod;
};

RTW_DHD bool dn_finite3(float4 c) {
    return (fbits(c.x) & 0x7F800000u) != 0x7F800000u && (fbits(c.y) & 0x7F800000u) != 0x7F800000u &&
           (fbits(c.z) & 0x7F800000u) != 0x7F800000u;
}
RTW_DHD float dn_floor(float a) { return a > 0x1p-8f ? a : 0x1p-8f; }  // max(albedo, 2^-8); a NaN: 2^-8

RTW_DHD float4 dn_prepass(float4 a, const float4* albedo, size_t p) {
    const float inv = 1.0f / a.w;
    float4 c = make_float4(a.x * inv, a.y * inv, a.z * inv, a.w);
    if (albedo) {
        const float4 al = albedo[p];
        c.x = c.x / dn_floor(al.x);
        c.y = c.y / dn_floor(al.y);
        c.z = c.z / dn_floor(al.z);
    }
    return c;
}

// where a pass's taps come from: the planes through L1 / L2
struct DnGlobalTaps {
    const float4 *src, *nd;
    uint32_t W;
    RTW_DHD void operator()(int64_t qx, int64_t qy, float4& c, float4& n) const {
        const size_t q = (size_t)qy * W + (size_t)qx;
        c = src[q];
        n = nd[q];
    }
};

template <typename Taps>
RTW_DHD float4 dn_filter_pixel(const DnPass& P, const Taps& taps, uint32_t x, uint32_t y) {
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const size_t p = (size_t)y * P.W + x;
    float4 cp, np;
    taps((int64_t)x, (int64_t)y, cp, np);
    const bool hit_p = np.w > 0.0f;
    const float kc = dn_finite3(cp) ? P.kc : 0.0f;
    const float kn = P.kn;
    const float kz = (hit_p && P.sd2 > 0.0f) ? 1.0f / (P.sd2 * (np.w * np.w)) : 0.0f;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, wsum = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)P.s * dy;
        if (qy < 0 || qy >= (int64_t)P.H) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = (int64_t)x + (int64_t)P.s * dx;
            if (qx < 0 || qx >= (int64_t)P.W) continue;
            float4 cq, nq;
            taps(qx, qy, cq, nq);
            if (!dn_finite3(cq) || (nq.w > 0.0f) != hit_p) continue;
            float tc = 0.0f, tn = 0.0f, tz = 0.0f;
            if (kc > 0.0f) {
                const float dr = cq.x - cp.x, dg = cq.y - cp.y, db = cq.z - cp.z;
                tc = ((dr * dr + dg * dg) + db * db) * kc;
            }
            if (kn > 0.0f) {
                const float ex = nq.x - np.x, ey = nq.y - np.y, ez = nq.z - np.z;
                tn = ((ex * ex + ey * ey) + ez * ez) * kn;
            }
            if (kz > 0.0f) {
                const float dz = nq.w - np.w;
                tz = (dz * dz) * kz;
            }
            const float wgt = (h[dx + 2] * h[dy + 2]) * rtw_expneg((tc + tn) + tz);
            sr += wgt * cq.x;
            sg += wgt * cq.y;
            sb += wgt * cq.z;
            wsum += wgt;
        }
    }
    float4 o = cp;
    if (wsum > 0.0f) {
        o.x = sr / wsum;
        o.y = sg / wsum;
        o.z = sb / wsum;
    }
    if (P.last) {
        if (P.demod) {
            const float4 al = P.albedo[p];
            o.x = o.x * dn_floor(al.x);
            o.y = o.y * dn_floor(al.y);
            o.z = o.z * dn_floor(al.z);
        }
        o.x = o.x * o.w;
        o.y = o.y * o.w;
        o.z = o.z * o.w;
    }
    return o;
}

__global__ __launch_bounds__(256) void denoise_prepass_kernel(const float4* accum, const float4* albedo, float4* dst,
                                                              uint32_t W, uint32_t H) {
    const uint32_t x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    dst[p] = dn_prepass(accum[p], albedo, p);
}

__global__ __launch_bounds__(256) void denoise_pass_kernel(DnPass P) {
    const uint32_t x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= P.W || y >= P.H) return;
    P.dst[(size_t)y * P.W + x] = dn_filter_pixel(P, DnGlobalTaps{P.src, P.nd, P.W}, x, y);
}

#if !defined(RTW_DENOISE_NO_LDS)
// The passes with spacing S = 1 and 2 stage the block's 32 x 8 tile and its halo of 2 S pixels -- both planes, 13.5
// and 20 KiB -- in LDS and take their taps from there: 10 % (1200 x 800) to 17 % (3840 x 2160) off the whole call
// against taps through L1 / L2, five alternating pairs, spread 2 % (profiles/denoise/LDS_AB.md; the A side is the
// build with -DRTW_DENOISE_NO_LDS).  The arithmetic and its order are dn_filter_pixel's: the bits do not change.
template <int S>
struct DnLdsTaps {
    static constexpr int TW = 32 + 4 * S, TH = 8 + 4 * S;
    const float4 *c, *n;
    int64_t bx, by;
    __device__ __forceinline__ void operator()(int64_t qx, int64_t qy, float4& cq, float4& nq) const {
        const int k = (int)(qy - by) * TW + (int)(qx - bx);
        cq = c[k];
        nq = n[k];
    }
};
template <int S>
__global__ __launch_bounds__(256) void denoise_pass_lds_kernel(DnPass P) {
    using T = DnLdsTaps<S>;
    __shared__ float4 sc[T::TH * T::TW], sn[T::TH * T::TW];
    const int64_t bx = (int64_t)blockIdx.x * 32 - 2 * S, by = (int64_t)blockIdx.y * 8 - 2 * S;
    for (int k = threadIdx.x; k < T::TH * T::TW; k += 256) {
        const int64_t gx = bx + k % T::TW, gy = by + k / T::TW;
        if (gx >= 0 && gx < (int64_t)P.W && gy >= 0 && gy < (int64_t)P.H) {  // (taps off the image are never read)
            const size_t q = (size_t)gy * P.W + (size_t)gx;
            sc[k] = P.src[q];
            sn[k] = P.nd[q];
        }
    }
    __syncthreads();
    const uint32_t x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= P.W || y >= P.H) return;
    P.dst[(size_t)y * P.W + x] = dn_filter_pixel(P, T{sc, sn, bx, by}, x, y);
}
#endif

bool sigma_ok(float s) { return s >= 0.0f && s <= 3.4028234e38f; }

int check_params(const rtw_ctx* ctx, uint32_t W, uint32_t H, const void* accum, const void* albedo, const void* nd,
                 const rtw_denoise_params* p, const void* out) {
    if (!ctx || !p || !accum || !nd || !out) return rtw_invalid("rtw_denoise: null ctx / params / accum / normal_depth / out");
    if (p->passes < 1 || p->passes > RTW_DENOISE_MAX_PASSES) return rtw_invalid("rtw_denoise: passes outside 1..8");
    if (p->flags & ~(uint32_t)RTW_DENOISE_DEMODULATE) return rtw_invalid("rtw_denoise: unknown flag bits");
    if (!sigma_ok(p->sigma_color) || !sigma_ok(p->sigma_normal) || !sigma_ok(p->sigma_depth))
        return rtw_invalid("rtw_denoise: a sigma is negative or not finite");
    if (W == 0 || H == 0) return rtw_invalid("rtw_denoise: width * height == 0");
    if ((uint64_t)W * H > 0xFFFFFFFFull) return rtw_invalid("rtw_denoise: image too large");
    if ((p->flags & RTW_DENOISE_DEMODULATE) && !albedo) return rtw_invalid("rtw_denoise: RTW_DENOISE_DEMODULATE without albedo");
    return RTW_OK;
}

// pass i of the call: planes[i & 1] -> planes[~i & 1], the last one into `out`
DnPass make_pass(uint32_t W, uint32_t H, const rtw_denoise_params& p, uint32_t i, float4* const planes[2],
                 const float4* albedo, const float4* nd, float4* out) {
    DnPass P{};
    P.src = planes[i & 1];
    P.nd = nd;
    P.demod = (p.flags & RTW_DENOISE_DEMODULATE) ? 1u : 0u;
    P.albedo = P.demod ? albedo : nullptr;
    P.last = i + 1 == p.passes ? 1u : 0u;
    P.dst = P.last ? out : planes[(i & 1) ^ 1];
    P.W = W;
    P.H = H;
    P.s = 1 << i;
    const float sc = p.sigma_color * ubits((127u - i) << 23);  // sigma_color 2^-i
    P.kc = p.sigma_color > 0.0f ? 1.0f / (sc * sc) : 0.0f;
    P.kn = p.sigma_normal > 0.0f ? 1.0f / (p.sigma_normal * p.sigma_normal) : 0.0f;
    P.sd2 = p.sigma_depth * p.sigma_depth;
    return P;
}

// the context's planes, >= n pixels each (the caller holds ctx->mu and has entered stream s)
int ensure_planes(rtw_ctx* ctx, uint64_t n, hipStream_t s) {
    if (ctx->dn_cap >= n) return RTW_OK;
    uint64_t cap = 0;
    ctx->dn_cap = 0;
    for (int k = 0; k < 2; k++) HIP_TRY(rtw_device_grow(&ctx->d_dn[k], &cap, n, (size_t)n * 16, s));
    ctx->dn_cap = n;
    return RTW_OK;
}

// Enqueue the whole filter on s (device pointers; the caller holds ctx->mu and has entered s)
int enqueue_filter(rtw_ctx* ctx, uint32_t W, uint32_t H, const float4* accum, const float4* albedo, const float4* nd,
                   const rtw_denoise_params& p, float4* out, hipStream_t s) {
    if (int rc = ensure_planes(ctx, (uint64_t)W * H, s)) return rc;
    const dim3 g = pixel_grid(W, H);
    const bool demod = (p.flags & RTW_DENOISE_DEMODULATE) != 0;
    hipLaunchKernelGGL(denoise_prepass_kernel, g, dim3(256), 0, s, accum, demod ? albedo : nullptr, ctx->d_dn[0], W, H);
    for (uint32_t i = 0; i < p.passes; i++) {
        const DnPass P = make_pass(W, H, p, i, ctx->d_dn, albedo, nd, out);
#if !defined(RTW_DENOISE_NO_LDS)
        if (i == 0) {
            hipLaunchKernelGGL(denoise_pass_lds_kernel<1>, g, dim3(256), 0, s, P);
            continue;
        }
        if (i == 1) {
            hipLaunchKernelGGL(denoise_pass_lds_kernel<2>, g, dim3(256), 0, s, P);
            continue;
        }
#endif
        hipLaunchKernelGGL(denoise_pass_kernel, g, dim3(256), 0, s, P);
    }
    HIP_TRY(hipGetLastError());
    return RTW_OK;
}

void host_filter(rtw_ctx* ctx, uint32_t W, uint32_t H, const float4* accum, const float4* albedo, const float4* nd,
                 const rtw_denoise_params& p, float4* out) {
    const size_t n = (size_t)W * H;
    for (auto& v : ctx->dn_host)
        if (v.size() < n) v.resize(n);
    float4* planes[2] = {ctx->dn_host[0].data(), ctx->dn_host[1].data()};
    const bool demod = (p.flags & RTW_DENOISE_DEMODULATE) != 0;
    rtw_host_ranges(H, ctx->cpu_threads, 1, [&](uint32_t y0, uint32_t y1) {
        for (size_t q = (size_t)y0 * W; q < (size_t)y1 * W; q++) planes[0][q] = dn_prepass(accum[q], demod ? albedo : nullptr, q);
    });
    for (uint32_t i = 0; i < p.passes; i++) {
        const DnPass P = make_pass(W, H, p, i, planes, albedo, nd, out);
        rtw_host_ranges(H, ctx->cpu_threads, 1, [&](uint32_t y0, uint32_t y1) {
            for (uint32_t y = y0; y < y1; y++)
                for (uint32_t x = 0; x < W; x++)
                    P.dst[(size_t)y * W + x] = dn_filter_pixel(P, DnGlobalTaps{P.src, P.nd, P.W}, x, y);
        });
    }
}

}  // namespace

extern "C" {

void rtw_denoise_defaults(rtw_denoise_params* p) {
    if (!p) return;
    // profiles/denoise/defaults.json: the winner of the grid search (tools/denoise_defaults.py) -- 8 spp against
    // 2048 spp on Cornell, Book-1 and earth + Perlin at 64 x 64, mean RMSE ratio 0.79.  A wide colour term (the
    // guides do the edge stopping), no demodulation (a point-sampled albedo aliases against a 64 x 64 pixel's mean)
    *p = rtw_denoise_params{};
    p->passes = 3;
    p->flags = 0;
    p->sigma_color = 32.0f;
    p->sigma_normal = 0.1f;
    p->sigma_depth = 0.005f;
}

int rtw_render_guides_device(rtw_ctx* ctx, const rtw_camera* cam, float* d_albedo, float* d_normal_depth, void* stream,
                             uint32_t flags) {
    if (!ctx || !d_albedo || !d_normal_depth) return rtw_invalid("rtw_render_guides_device: null ctx / albedo / normal_depth");
    if (ctx->device == RTW_DEVICE_CPU) return rtw_invalid("host context: use rtw_render_guides");
    if (int rc = rtw_validate_cam(cam)) return rc;
    if (flags & ~(uint32_t)RTW_RENDER_NO_SYNC) return rtw_invalid("rtw_render_guides_device: unknown flag bits");
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (int rc = rtw_stream_enter(ctx, s)) return rc;
    rtw_launch L = rtw_make_launch(ctx, cam, 0);
    L.counters = nullptr;
    auto launch = [&](auto c) {
        hipLaunchKernelGGL(guides_kernel<decltype(c)::value>, pixel_grid(L.W, L.H), dim3(256), 0, s, L,
                           reinterpret_cast<float4*>(d_albedo), reinterpret_cast<float4*>(d_normal_depth));
    };
    if (!RtwFirstHitClasses::visit(rtw_guide_class(L), launch)) (void)RtwGuideEnvClasses::visit(rtw_guide_class(L), launch);
    HIP_TRY(hipGetLastError());
    if (int rc = rtw_stream_leave(ctx, s)) return rc;
    if (!(flags & RTW_RENDER_NO_SYNC)) HIP_TRY(hipStreamSynchronize(s));
    return RTW_OK;
}

int rtw_render_guides(rtw_ctx* ctx, const rtw_camera* cam, float* albedo, float* normal_depth) {
    if (!ctx || !albedo || !normal_depth) return rtw_invalid("rtw_render_guides: null ctx / albedo / normal_depth");
    if (int rc = rtw_validate_cam(cam)) return rc;
    if (ctx->device == RTW_DEVICE_CPU) {
        // the lock is held for the whole trace (a frame of single rays is short): the registrations
        // (rtw_scene_set_lights, rtw_scene_set_vertex_attrs) take it too, so none changes what the threads read
        std::lock_guard<std::mutex> lock(ctx->mu);
        rtw_launch L = rtw_make_launch(ctx, cam, 0);
        L.counters = nullptr;
        float4* a = reinterpret_cast<float4*>(albedo);
        float4* n = reinterpret_cast<float4*>(normal_depth);
        auto rows = [&](auto c) {
            rtw_host_ranges(L.H, ctx->cpu_threads, 1,
                            [&](uint32_t y0, uint32_t y1) { guides_rows<decltype(c)::value>(L, y0, y1, a, n); });
        };
        if (!RtwFirstHitClasses::visit(rtw_guide_class(L), rows)) (void)RtwGuideEnvClasses::visit(rtw_guide_class(L), rows);
        return RTW_OK;
    }
    // GPU context: the two guides through a device staging block of this call's
    const size_t nb = (size_t)cam->size * 16;
    float* d = nullptr;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), 2 * nb));
    }
    int rc = rtw_render_guides_device(ctx, cam, d, d + nb / 4, nullptr, 0);
    hipError_t e = hipSuccess;
    if (rc == RTW_OK) e = hipMemcpy(albedo, d, nb, hipMemcpyDeviceToHost);
    if (rc == RTW_OK && e == hipSuccess) e = hipMemcpy(normal_depth, d + nb / 4, nb, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return rtw_hip_fail(e, "rtw_render_guides copy back");
    return rc;
}

int rtw_denoise_device(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* d_accum, const float* d_albedo,
                       const float* d_normal_depth, const rtw_denoise_params* params, float* d_out, void* stream,
                       uint32_t flags) {
    if (int rc = check_params(ctx, width, height, d_accum, d_albedo, d_normal_depth, params, d_out)) return rc;
    if (ctx->device == RTW_DEVICE_CPU) return rtw_invalid("host context: use rtw_denoise");
    if (flags & ~(uint32_t)RTW_RENDER_NO_SYNC) return rtw_invalid("rtw_denoise_device: unknown flag bits");
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (int rc = rtw_stream_enter(ctx, s)) return rc;
    if (int rc = enqueue_filter(ctx, width, height, reinterpret_cast<const float4*>(d_accum),
                                reinterpret_cast<const float4*>(d_albedo), reinterpret_cast<const float4*>(d_normal_depth),
                                *params, reinterpret_cast<float4*>(d_out), s))
        return rc;
    if (int rc = rtw_stream_leave(ctx, s)) return rc;
    if (!(flags & RTW_RENDER_NO_SYNC)) HIP_TRY(hipStreamSynchronize(s));
    return RTW_OK;
}

int rtw_denoise(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* accum, const float* albedo,
                const float* normal_depth, const rtw_denoise_params* params, float* out) {
    if (int rc = check_params(ctx, width, height, accum, albedo, normal_depth, params, out)) return rc;
    if (ctx->device == RTW_DEVICE_CPU) {
        std::lock_guard<std::mutex> lock(ctx->mu);  // the planes are the context's
        host_filter(ctx, width, height, reinterpret_cast<const float4*>(accum), reinterpret_cast<const float4*>(albedo),
                    reinterpret_cast<const float4*>(normal_depth), *params, reinterpret_cast<float4*>(out));
        return RTW_OK;
    }
    // GPU context: accum (and the result, in place), albedo, normal_depth through a device staging block
    const size_t nb = (size_t)width * height * 16, nf = nb / 4;
    float* d = nullptr;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), 3 * nb));
    }
    hipError_t e = hipMemcpy(d, accum, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + nf, normal_depth, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess && albedo) e = hipMemcpy(d + 2 * nf, albedo, nb, hipMemcpyHostToDevice);
    int rc = RTW_OK;
    if (e == hipSuccess) rc = rtw_denoise_device(ctx, width, height, d, albedo ? d + 2 * nf : nullptr, d + nf, params, d, nullptr, 0);
    if (e == hipSuccess && rc == RTW_OK) e = hipMemcpy(out, d, nb, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return rtw_hip_fail(e, "rtw_denoise staging");
    return rc;
}

int rtw_debug_expneg(uint32_t n, const float* x, float* out) {
    if (n && (!x || !out)) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) out[i] = rtw_expneg(x[i]);
    return RTW_OK;
}

}  // extern "C"
