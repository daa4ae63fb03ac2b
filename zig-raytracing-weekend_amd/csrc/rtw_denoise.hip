// rtw_denoise.hip -- denoised previews (include/rtw_gpu.h, DESIGN.md §Denoised previews): first-hit guide buffers
// (albedo, normal + depth) and the edge-avoiding a-trous wavelet filter of Dammertz et al. 2010 over the
// accumulator's mean radiance; and the noise estimates and the variance-guided filter built on it (§Noise estimates and
// the guided filter; their sections below).  Kernels of their own: no render kernel, class table or launch is touched.
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
#include "rtw_moments.h"

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

// `who`: the entry point's family, "rtw_denoise" or "rtw_denoise_guided" (the message names the call refused)
int refuse(const char* who, const char* what) {
    char msg[128];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return rtw_invalid(msg);
}

int check_params(const char* who, const rtw_ctx* ctx, uint32_t W, uint32_t H, const void* accum, const void* albedo,
                 const void* nd, const rtw_denoise_params* p, const void* out) {
    if (!ctx || !p || !accum || !nd || !out) return refuse(who, "null ctx / params / accum / normal_depth / out");
    if (p->passes < 1 || p->passes > RTW_DENOISE_MAX_PASSES) return refuse(who, "passes outside 1..8");
    if (p->flags & ~(uint32_t)RTW_DENOISE_DEMODULATE) return refuse(who, "unknown flag bits");
    if (!sigma_ok(p->sigma_color) || !sigma_ok(p->sigma_normal) || !sigma_ok(p->sigma_depth))
        return refuse(who, "a sigma is negative or not finite");
    if (W == 0 || H == 0) return refuse(who, "width * height == 0");
    if ((uint64_t)W * H > 0xFFFFFFFFull) return refuse(who, "image too large");
    if ((p->flags & RTW_DENOISE_DEMODULATE) && !albedo) return refuse(who, "RTW_DENOISE_DEMODULATE without albedo");
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

// ---------------------------------------------------------------------------
// Noise estimates: running moments of the per-batch mean luminance (include/rtw_gpu.h, DESIGN.md §Noise estimates
// and the guided filter).  moments = two float4[W H] planes: the accumulator as of the last update, then
// (mean, M2, n, sw).  Every function below is one rounded fp32 operation per step in the association written.
// ---------------------------------------------------------------------------
// (dn_luma, dn_finite1 / dn_finite3 and West's update itself, mo_batch_luma and mo_west, are rtw_moments.h's: the
// temporal reprojection of rtw_temporal.hip runs them too)
// West's weighted update of one pixel by the batch a - p; false: neither plane changes
RTW_DHD bool mo_update(float4 a, float4& p, float4& m) {
    const float k = a.w - p.w;
    if (!(k > 0.0f)) return false;
    const float y = mo_batch_luma(a.x - p.x, a.y - p.y, a.z - p.z, k);
    p = a;
    if (!dn_finite1(y)) return true;
    mo_west(m, y, k);
    return true;
}
// The variance of the pixel's mean luminance, v = (M2 / (n - 1)) / sw; -1: unknown (n < 2).  What is not > 0 (a
// rounding residue below zero, a NaN of overflowed moments) is 0.
RTW_DHD float mo_variance(float4 m) {
    if (!(m.z >= 2.0f)) return -1.0f;
    const float v = (m.y / (m.z - 1.0f)) / m.w;
    return v > 0.0f ? v : 0.0f;
}
// sqrt(v) / (|mean| + floor); +inf where the variance is unknown, 0 where it is 0 (whatever the divisor)
RTW_DHD float mo_error(float4 m, float floor) {
    const float v = mo_variance(m);
    if (v < 0.0f) return __builtin_inff();
    const float sv = __builtin_sqrtf(v);
    if (!(sv > 0.0f)) return 0.0f;
    const float e = sv / (__builtin_fabsf(m.x) + floor);
    return e >= 0.0f ? e : __builtin_inff();
}

__global__ __launch_bounds__(256) void moments_kernel(const float4* accum, float4* mom, uint32_t W, uint32_t H) {
    const uint32_t x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x, n = (size_t)W * H;
    float4 p0 = mom[p], m = mom[n + p];
    if (mo_update(accum[p], p0, m)) {
        mom[p] = p0;
        mom[n + p] = m;
    }
}

void moments_rows(const float4* accum, float4* mom, size_t n, size_t q0, size_t q1) {
    for (size_t q = q0; q < q1; q++) (void)mo_update(accum[q], mom[q], mom[n + q]);
}

// One wave per 8 x 8 tile (lane = 8 ly + lx: a tile's row is one 128-B line of plane 1), the tiles dealt round robin
// to the waves of at most NOISE_BLOCKS blocks.  The errors are non-negative (or +inf), so their order is their bit
// patterns' as unsigned integers: every combination is an integer maximum or an integer count -- no floating-point
// sum, nothing whose order could show.  A tile's maximum is one wave's shuffles; a wave keeps its counts in
// registers over its tiles, the four waves meet in LDS once, and one lane per block adds to the summary with global
// atomics -- three per block, which is why the blocks are few and loop: a block per 32 x 8 pixels, the shape of the
// other streaming kernels here, would put 32 400 blocks on one cache line at 3840 x 2160
// (profiles/denoise_guided/NOTES.md).
constexpr uint32_t NOISE_BLOCKS = 1024;
__global__ __launch_bounds__(256) void noise_kernel(const float4* mom1, uint32_t W, uint32_t H, float floor,
                                                    float threshold, float* err, float* tile_max,
                                                    rtw_noise_summary* out) {
    __shared__ uint32_t s_max, s_over, s_known;
    if (threadIdx.x == 0) s_max = s_over = s_known = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, lx = lane & 7, ly = lane >> 3;
    const uint32_t tw = (W + 7) / 8, nt = tw * ((H + 7) / 8), nwaves = gridDim.x * 4;
    uint32_t f = 0, over = 0, known = 0;                       // the largest finite error and the counts, per lane
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < nt; t += nwaves) {   // (uniform in a wave)
        const uint32_t x = (t % tw) * 8 + lx, y = (t / tw) * 8 + ly;
        float e = 0.0f;
        if (x < W && y < H) {
            const size_t p = (size_t)y * W + x;
            const float4 m = mom1[p];
            e = mo_error(m, floor);
            over += e > threshold;
            known += m.z >= 2.0f;
            if (err) err[p] = e;
        }
        uint32_t b = fbits(e);                                 // the tile's maximum: +inf included
        f = max(f, b < 0x7F800000u ? b : 0u);
        for (int k = 1; k <= 32; k <<= 1) b = max(b, (uint32_t)__shfl_xor((int)b, k));
        if (tile_max && lane == 0) tile_max[t] = ubits(b);
    }
    for (int k = 1; k <= 32; k <<= 1) {
        f = max(f, (uint32_t)__shfl_xor((int)f, k));
        over += (uint32_t)__shfl_xor((int)over, k);
        known += (uint32_t)__shfl_xor((int)known, k);
    }
    if (lane == 0) {
        atomicMax(&s_max, f);
        atomicAdd(&s_over, over);
        atomicAdd(&s_known, known);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_over) atomicAdd(reinterpret_cast<unsigned long long*>(&out->over), (unsigned long long)s_over);
        if (s_known) atomicAdd(reinterpret_cast<unsigned long long*>(&out->known), (unsigned long long)s_known);
        if (s_max) atomicMax(reinterpret_cast<uint32_t*>(&out->max_err), s_max);
    }
}

void host_noise(const float4* mom1, uint32_t W, uint32_t H, float floor, float threshold, float* err, float* tile_max,
                rtw_noise_summary* out) {
    const uint32_t tw = (W + 7) / 8, th = (H + 7) / 8;
    rtw_noise_summary s{};
    if (tile_max) std::fill(tile_max, tile_max + (size_t)tw * th, 0.0f);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            const float e = mo_error(mom1[p], floor);
            if (err) err[p] = e;
            if (tile_max) {
                float& t = tile_max[(size_t)(y / 8) * tw + x / 8];
                t = e > t ? e : t;
            }
            s.over += e > threshold;
            s.known += mom1[p].z >= 2.0f;
            if (dn_finite1(e) && e > s.max_err) s.max_err = e;
        }
    *out = s;
}

int check_frame(const char* who, uint32_t W, uint32_t H) {
    if (W == 0 || H == 0 || (uint64_t)W * H > 0xFFFFFFFFull) return refuse(who, "width * height == 0 or too large");
    return RTW_OK;
}

// a device block of this call's (the host-buffer entry points of a GPU context stage through one)
struct DnStaging {
    float* d = nullptr;
    ~DnStaging() {
        if (d) (void)hipFree(d);
    }
    int alloc(rtw_ctx* ctx, size_t bytes) {
        std::lock_guard<std::mutex> lock(ctx->mu);
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), bytes));
        return RTW_OK;
    }
};

// ---------------------------------------------------------------------------
// The variance-guided filter: SVGF's spatial filter (Schied et al. 2017) -- dn_filter_pixel with the colour term
// measured in standard deviations of the locally filtered variance, and the variance carried through the passes.
//   pre-pass   the colour plane as above;  v = mo_variance (-1: unknown), demodulated: v / (la la), la = the
//              luminance of the floored albedo
//   pass i     vbar = (sum (g[dx] g[dy]) v_q) / (sum g[dx] g[dy]) over the 3 x 3 taps at spacing 1 (rows outer) that
//              are on the image, have the centre's hit state, a finite colour and v_q >= 0;  g = {1/4, 1/2, 1/4}
//              kl = 1 / (sl sqrt(vbar) + 2^-20)  (0: no such tap, sl = 0 or c_p not finite)
//              per tap  tl = |Y_q - Y_p| kl;  wgt = (h[dx] h[dy]) e((tl + tn) + tz);  vsum += (wgt wgt) max(v_q, 0)
//              v' = v_p < 0 ? -1 : wsum > 0 ? vsum / (wsum wsum) : v_p
//   last pass  out as above;  variance_out = v' (la la) demodulated, -1 where unknown
// sl = sigma_color, the same in every pass: the propagated variance shrinks instead.
// ---------------------------------------------------------------------------
struct DnGuidedPass {
    const float4 *src, *nd, *albedo;  // albedo: null unless demodulating
    const float* vsrc;                // the pass's input variance plane
    float4* dst;                      // the other colour plane, or `out` in the last pass
    float* vdst;                      // the other variance plane; variance_out (may be null) in the last pass
    uint32_t W, H;
    int32_t s;
    float sl, kn, sd2;
    uint32_t last, demod;
};

RTW_DHD float dn_albedo_luma(float4 al) { return dn_luma(dn_floor(al.x), dn_floor(al.y), dn_floor(al.z)); }

RTW_DHD float dn_guided_variance(float4 m, const float4* albedo, size_t p) {
    float v = mo_variance(m);
    if (albedo && v >= 0.0f) {
        const float la = dn_albedo_luma(albedo[p]);
        v = v / (la * la);
    }
    return v;
}

struct DnGuidedGlobalTaps {
    const float4 *src, *nd;
    const float* vsrc;
    uint32_t W;
    RTW_DHD void operator()(int64_t qx, int64_t qy, float4& c, float4& n, float& v) const {
        const size_t q = (size_t)qy * W + (size_t)qx;
        c = src[q];
        n = nd[q];
        v = vsrc[q];
    }
};

template <typename Taps>
RTW_DHD float4 dn_guided_pixel(const DnGuidedPass& P, const Taps& taps, uint32_t x, uint32_t y, float& vout) {
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float g[3] = {0.25f, 0.5f, 0.25f};
    const size_t p = (size_t)y * P.W + x;
    float4 cp, np;
    float vp;
    taps((int64_t)x, (int64_t)y, cp, np, vp);
    const bool hit_p = np.w > 0.0f;
    float kl = 0.0f;
    if (P.sl > 0.0f && dn_finite3(cp)) {
        float vs = 0.0f, gs = 0.0f;
        for (int dy = -1; dy <= 1; dy++) {
            const int64_t qy = (int64_t)y + dy;
            if (qy < 0 || qy >= (int64_t)P.H) continue;
            for (int dx = -1; dx <= 1; dx++) {
                const int64_t qx = (int64_t)x + dx;
                if (qx < 0 || qx >= (int64_t)P.W) continue;
                float4 cq, nq;
                float vq;
                taps(qx, qy, cq, nq, vq);
                if (!dn_finite3(cq) || (nq.w > 0.0f) != hit_p || !(vq >= 0.0f)) continue;
                const float gw = g[dx + 1] * g[dy + 1];
                vs += gw * vq;
                gs += gw;
            }
        }
        if (gs > 0.0f) kl = 1.0f / (P.sl * __builtin_sqrtf(vs / gs) + 0x1p-20f);
    }
    const float yp = dn_luma(cp.x, cp.y, cp.z);
    const float kn = P.kn;
    const float kz = (hit_p && P.sd2 > 0.0f) ? 1.0f / (P.sd2 * (np.w * np.w)) : 0.0f;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, wsum = 0.0f, vsum = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)P.s * dy;
        if (qy < 0 || qy >= (int64_t)P.H) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = (int64_t)x + (int64_t)P.s * dx;
            if (qx < 0 || qx >= (int64_t)P.W) continue;
            float4 cq, nq;
            float vq;
            taps(qx, qy, cq, nq, vq);
            if (!dn_finite3(cq) || (nq.w > 0.0f) != hit_p) continue;
            float tl = 0.0f, tn = 0.0f, tz = 0.0f;
            if (kl > 0.0f) tl = __builtin_fabsf(dn_luma(cq.x, cq.y, cq.z) - yp) * kl;
            if (kn > 0.0f) {
                const float ex = nq.x - np.x, ey = nq.y - np.y, ez = nq.z - np.z;
                tn = ((ex * ex + ey * ey) + ez * ez) * kn;
            }
            if (kz > 0.0f) {
                const float dz = nq.w - np.w;
                tz = (dz * dz) * kz;
            }
            const float wgt = (h[dx + 2] * h[dy + 2]) * rtw_expneg((tl + tn) + tz);
            sr += wgt * cq.x;
            sg += wgt * cq.y;
            sb += wgt * cq.z;
            wsum += wgt;
            vsum += (wgt * wgt) * (vq > 0.0f ? vq : 0.0f);
        }
    }
    float4 o = cp;
    vout = vp;
    if (wsum > 0.0f) {
        o.x = sr / wsum;
        o.y = sg / wsum;
        o.z = sb / wsum;
        vout = vsum / (wsum * wsum);
    }
    if (!(vp >= 0.0f)) vout = -1.0f;
    if (P.last) {
        if (P.demod) {
            const float4 al = P.albedo[p];
            o.x = o.x * dn_floor(al.x);
            o.y = o.y * dn_floor(al.y);
            o.z = o.z * dn_floor(al.z);
            if (vout >= 0.0f) {
                const float la = dn_albedo_luma(al);
                vout = vout * (la * la);
            }
        }
        o.x = o.x * o.w;
        o.y = o.y * o.w;
        o.z = o.z * o.w;
    }
    return o;
}

__global__ __launch_bounds__(256) void guided_prepass_kernel(const float4* accum, const float4* mom1,
                                                             const float4* albedo, float4* dst, float* vdst, uint32_t W,
                                                             uint32_t H) {
    const uint32_t x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    dst[p] = dn_prepass(accum[p], albedo, p);
    vdst[p] = dn_guided_variance(mom1[p], albedo, p);
}

__global__ __launch_bounds__(256) void guided_pass_kernel(DnGuidedPass P) {
    const uint32_t x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= P.W || y >= P.H) return;
    float v;
    P.dst[(size_t)y * P.W + x] = dn_guided_pixel(P, DnGuidedGlobalTaps{P.src, P.nd, P.vsrc, P.W}, x, y, v);
    if (P.vdst) P.vdst[(size_t)y * P.W + x] = v;
}

#if !defined(RTW_GUIDED_NO_LDS)
// The passes with spacing 1 and 2 from an LDS tile, as denoise_pass_lds_kernel: three planes, 15.2 and 22.5 KiB.
// Their halo of 2 S >= 2 pixels holds the 3 x 3 variance prefilter too.  The A/B against taps through L1 / L2
// (-DRTW_GUIDED_NO_LDS) is in profiles/denoise_guided/README.md.
template <int S>
struct DnGuidedLdsTaps {
    static constexpr int TW = 32 + 4 * S, TH = 8 + 4 * S;
    const float4 *c, *n;
    const float* v;
    int64_t bx, by;
    __device__ __forceinline__ void operator()(int64_t qx, int64_t qy, float4& cq, float4& nq, float& vq) const {
        const int k = (int)(qy - by) * TW + (int)(qx - bx);
        cq = c[k];
        nq = n[k];
        vq = v[k];
    }
};
template <int S>
__global__ __launch_bounds__(256) void guided_pass_lds_kernel(DnGuidedPass P) {
    using T = DnGuidedLdsTaps<S>;
    __shared__ float4 sc[T::TH * T::TW], sn[T::TH * T::TW];
    __shared__ float sv[T::TH * T::TW];
    const int64_t bx = (int64_t)blockIdx.x * 32 - 2 * S, by = (int64_t)blockIdx.y * 8 - 2 * S;
    for (int k = threadIdx.x; k < T::TH * T::TW; k += 256) {
        const int64_t gx = bx + k % T::TW, gy = by + k / T::TW;
        if (gx >= 0 && gx < (int64_t)P.W && gy >= 0 && gy < (int64_t)P.H) {  // (taps off the image are never read)
            const size_t q = (size_t)gy * P.W + (size_t)gx;
            sc[k] = P.src[q];
            sn[k] = P.nd[q];
            sv[k] = P.vsrc[q];
        }
    }
    __syncthreads();
    const uint32_t x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= P.W || y >= P.H) return;
    float v;
    P.dst[(size_t)y * P.W + x] = dn_guided_pixel(P, T{sc, sn, sv, bx, by}, x, y, v);
    if (P.vdst) P.vdst[(size_t)y * P.W + x] = v;
}
#endif

DnGuidedPass make_guided_pass(uint32_t W, uint32_t H, const rtw_denoise_params& p, uint32_t i, float4* const planes[2],
                              float* const vplanes[2], const float4* albedo, const float4* nd, float4* out,
                              float* variance_out) {
    DnGuidedPass P{};
    P.src = planes[i & 1];
    P.vsrc = vplanes[i & 1];
    P.nd = nd;
    P.demod = (p.flags & RTW_DENOISE_DEMODULATE) ? 1u : 0u;
    P.albedo = P.demod ? albedo : nullptr;
    P.last = i + 1 == p.passes ? 1u : 0u;
    P.dst = P.last ? out : planes[(i & 1) ^ 1];
    P.vdst = P.last ? variance_out : vplanes[(i & 1) ^ 1];
    P.W = W;
    P.H = H;
    P.s = 1 << i;
    P.sl = p.sigma_color;
    P.kn = p.sigma_normal > 0.0f ? 1.0f / (p.sigma_normal * p.sigma_normal) : 0.0f;
    P.sd2 = p.sigma_depth * p.sigma_depth;
    return P;
}

// the context's variance planes beside d_dn (the caller holds ctx->mu and has entered stream s)
int ensure_guided_planes(rtw_ctx* ctx, uint64_t n, hipStream_t s) {
    if (int rc = ensure_planes(ctx, n, s)) return rc;
    if (ctx->dnv_cap >= n) return RTW_OK;
    uint64_t cap = 0;
    ctx->dnv_cap = 0;
    for (int k = 0; k < 2; k++) HIP_TRY(rtw_device_grow(&ctx->d_dnv[k], &cap, n, (size_t)n * 4, s));
    ctx->dnv_cap = n;
    return RTW_OK;
}

int enqueue_guided(rtw_ctx* ctx, uint32_t W, uint32_t H, const float4* accum, const float4* mom1, const float4* albedo,
                   const float4* nd, const rtw_denoise_params& p, float4* out, float* variance_out, hipStream_t s) {
    if (int rc = ensure_guided_planes(ctx, (uint64_t)W * H, s)) return rc;
    const dim3 g = pixel_grid(W, H);
    const bool demod = (p.flags & RTW_DENOISE_DEMODULATE) != 0;
    hipLaunchKernelGGL(guided_prepass_kernel, g, dim3(256), 0, s, accum, mom1, demod ? albedo : nullptr, ctx->d_dn[0],
                       ctx->d_dnv[0], W, H);
    for (uint32_t i = 0; i < p.passes; i++) {
        const DnGuidedPass P = make_guided_pass(W, H, p, i, ctx->d_dn, ctx->d_dnv, albedo, nd, out, variance_out);
#if !defined(RTW_GUIDED_NO_LDS)
        if (i == 0) {
            hipLaunchKernelGGL(guided_pass_lds_kernel<1>, g, dim3(256), 0, s, P);
            continue;
        }
        if (i == 1) {
            hipLaunchKernelGGL(guided_pass_lds_kernel<2>, g, dim3(256), 0, s, P);
            continue;
        }
#endif
        hipLaunchKernelGGL(guided_pass_kernel, g, dim3(256), 0, s, P);
    }
    HIP_TRY(hipGetLastError());
    return RTW_OK;
}

void host_guided(rtw_ctx* ctx, uint32_t W, uint32_t H, const float4* accum, const float4* mom1, const float4* albedo,
                 const float4* nd, const rtw_denoise_params& p, float4* out, float* variance_out) {
    const size_t n = (size_t)W * H;
    for (auto& v : ctx->dn_host)
        if (v.size() < n) v.resize(n);
    for (auto& v : ctx->dnv_host)
        if (v.size() < n) v.resize(n);
    float4* planes[2] = {ctx->dn_host[0].data(), ctx->dn_host[1].data()};
    float* vplanes[2] = {ctx->dnv_host[0].data(), ctx->dnv_host[1].data()};
    const float4* al = (p.flags & RTW_DENOISE_DEMODULATE) ? albedo : nullptr;
    rtw_host_ranges(H, ctx->cpu_threads, 1, [&](uint32_t y0, uint32_t y1) {
        for (size_t q = (size_t)y0 * W; q < (size_t)y1 * W; q++) {
            planes[0][q] = dn_prepass(accum[q], al, q);
            vplanes[0][q] = dn_guided_variance(mom1[q], al, q);
        }
    });
    for (uint32_t i = 0; i < p.passes; i++) {
        const DnGuidedPass P = make_guided_pass(W, H, p, i, planes, vplanes, albedo, nd, out, variance_out);
        rtw_host_ranges(H, ctx->cpu_threads, 1, [&](uint32_t y0, uint32_t y1) {
            for (uint32_t y = y0; y < y1; y++)
                for (uint32_t x = 0; x < W; x++) {
                    float v;
                    P.dst[(size_t)y * W + x] = dn_guided_pixel(P, DnGuidedGlobalTaps{P.src, P.nd, P.vsrc, P.W}, x, y, v);
                    if (P.vdst) P.vdst[(size_t)y * W + x] = v;
                }
        });
    }
}

// the checks every entry point of a device form shares; on success the lock is the caller's to take
int check_device_form(const rtw_ctx* ctx, uint32_t flags, const char* host_form) {
    if (ctx->device == RTW_DEVICE_CPU) return rtw_invalid(host_form);
    if (flags & ~(uint32_t)RTW_RENDER_NO_SYNC) return rtw_invalid("unknown flag bits");
    return RTW_OK;
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
    if (int rc = check_params("rtw_denoise", ctx, width, height, d_accum, d_albedo, d_normal_depth, params, d_out)) return rc;
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
    if (int rc = check_params("rtw_denoise", ctx, width, height, accum, albedo, normal_depth, params, out)) return rc;
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

// ---- noise estimates and the guided filter
int rtw_moments_update_device(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* d_accum, float* d_moments,
                              void* stream, uint32_t flags) {
    if (!ctx || !d_accum || !d_moments) return rtw_invalid("rtw_moments_update: null ctx / accum / moments");
    if (int rc = check_frame("rtw_moments_update", width, height)) return rc;
    if (int rc = check_device_form(ctx, flags, "host context: use rtw_moments_update")) return rc;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (int rc = rtw_stream_enter(ctx, s)) return rc;
    hipLaunchKernelGGL(moments_kernel, pixel_grid(width, height), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(d_accum), reinterpret_cast<float4*>(d_moments), width, height);
    HIP_TRY(hipGetLastError());
    if (int rc = rtw_stream_leave(ctx, s)) return rc;
    if (!(flags & RTW_RENDER_NO_SYNC)) HIP_TRY(hipStreamSynchronize(s));
    return RTW_OK;
}

int rtw_moments_update(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* accum, float* moments) {
    if (!ctx || !accum || !moments) return rtw_invalid("rtw_moments_update: null ctx / accum / moments");
    if (int rc = check_frame("rtw_moments_update", width, height)) return rc;
    const size_t n = (size_t)width * height;
    if (ctx->device == RTW_DEVICE_CPU) {
        rtw_host_ranges(n, ctx->cpu_threads, 4096, [&](uint64_t q0, uint64_t q1) {
            moments_rows(reinterpret_cast<const float4*>(accum), reinterpret_cast<float4*>(moments), n, q0, q1);
        });
        return RTW_OK;
    }
    DnStaging st;  // accum, then the two planes
    if (int rc = st.alloc(ctx, 3 * n * 16)) return rc;
    hipError_t e = hipMemcpy(st.d, accum, n * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(st.d + 4 * n, moments, 2 * n * 16, hipMemcpyHostToDevice);
    int rc = RTW_OK;
    if (e == hipSuccess) rc = rtw_moments_update_device(ctx, width, height, st.d, st.d + 4 * n, nullptr, 0);
    if (e == hipSuccess && rc == RTW_OK) e = hipMemcpy(moments, st.d + 4 * n, 2 * n * 16, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return rtw_hip_fail(e, "rtw_moments_update staging");
    return rc;
}

int rtw_noise_estimate_device(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* d_moments, float floor,
                              float threshold, float* d_err, float* d_tile_max, rtw_noise_summary* d_out, void* stream,
                              uint32_t flags) {
    if (!ctx || !d_moments || !d_out) return rtw_invalid("rtw_noise_estimate: null ctx / moments / summary");
    if (int rc = check_frame("rtw_noise_estimate", width, height)) return rc;
    if (!sigma_ok(floor) || !sigma_ok(threshold)) return rtw_invalid("rtw_noise_estimate: floor or threshold is negative or not finite");
    if (int rc = check_device_form(ctx, flags, "host context: use rtw_noise_estimate")) return rc;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (int rc = rtw_stream_enter(ctx, s)) return rc;
    HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(rtw_noise_summary), s));
    const uint32_t tiles = ((width + 7) / 8) * ((height + 7) / 8);
    hipLaunchKernelGGL(noise_kernel, dim3(std::min((tiles + 3) / 4, NOISE_BLOCKS)), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(d_moments) + (size_t)width * height, width, height, floor,
                       threshold, d_err, d_tile_max, d_out);
    HIP_TRY(hipGetLastError());
    if (int rc = rtw_stream_leave(ctx, s)) return rc;
    if (!(flags & RTW_RENDER_NO_SYNC)) HIP_TRY(hipStreamSynchronize(s));
    return RTW_OK;
}

int rtw_noise_estimate(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* moments, float floor,
                       float threshold, float* err, float* tile_max, rtw_noise_summary* out) {
    if (!ctx || !moments || !out) return rtw_invalid("rtw_noise_estimate: null ctx / moments / summary");
    if (int rc = check_frame("rtw_noise_estimate", width, height)) return rc;
    if (!sigma_ok(floor) || !sigma_ok(threshold)) return rtw_invalid("rtw_noise_estimate: floor or threshold is negative or not finite");
    const size_t n = (size_t)width * height, nt = (size_t)((width + 7) / 8) * ((height + 7) / 8);
    if (ctx->device == RTW_DEVICE_CPU) {
        host_noise(reinterpret_cast<const float4*>(moments) + n, width, height, floor, threshold, err, tile_max, out);
        return RTW_OK;
    }
    DnStaging st;  // the two planes, err, tile_max, the summary (its 8-byte counts first: the planes keep it aligned)
    if (int rc = st.alloc(ctx, 2 * n * 16 + sizeof(rtw_noise_summary) + (n + nt) * 4)) return rc;
    float *d_sum = st.d + 8 * n, *d_err = d_sum + sizeof(rtw_noise_summary) / 4, *d_tile = d_err + n;
    hipError_t e = hipMemcpy(st.d, moments, 2 * n * 16, hipMemcpyHostToDevice);
    int rc = RTW_OK;
    if (e == hipSuccess)
        rc = rtw_noise_estimate_device(ctx, width, height, st.d, floor, threshold, err ? d_err : nullptr,
                                       tile_max ? d_tile : nullptr, reinterpret_cast<rtw_noise_summary*>(d_sum), nullptr, 0);
    if (e == hipSuccess && rc == RTW_OK && err) e = hipMemcpy(err, d_err, n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && rc == RTW_OK && tile_max) e = hipMemcpy(tile_max, d_tile, nt * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && rc == RTW_OK) e = hipMemcpy(out, d_sum, sizeof(rtw_noise_summary), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return rtw_hip_fail(e, "rtw_noise_estimate staging");
    return rc;
}

void rtw_denoise_guided_defaults(rtw_denoise_params* p) {
    if (!p) return;
    // profiles/denoise_guided/defaults.json: the winner of the grid search (tools/denoise_guided_defaults.py), in
    // the setting of rtw_denoise_defaults' search with the moments taken from 1-spp batches
    *p = rtw_denoise_params{};
    p->passes = 3;
    p->flags = 0;
    p->sigma_color = 4.0f;
    p->sigma_normal = 0.25f;
    p->sigma_depth = 0.02f;
}

// The device form's work once the arguments are checked: d_mom1 is the moments' second plane, the only one read
static int guided_on_device(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* d_accum, const float* d_mom1,
                            const float* d_albedo, const float* d_normal_depth, const rtw_denoise_params* params,
                            float* d_out, float* d_variance_out, void* stream, uint32_t flags) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (int rc = rtw_stream_enter(ctx, s)) return rc;
    if (int rc = enqueue_guided(ctx, width, height, reinterpret_cast<const float4*>(d_accum),
                                reinterpret_cast<const float4*>(d_mom1), reinterpret_cast<const float4*>(d_albedo),
                                reinterpret_cast<const float4*>(d_normal_depth), *params,
                                reinterpret_cast<float4*>(d_out), d_variance_out, s))
        return rc;
    if (int rc = rtw_stream_leave(ctx, s)) return rc;
    if (!(flags & RTW_RENDER_NO_SYNC)) HIP_TRY(hipStreamSynchronize(s));
    return RTW_OK;
}

int rtw_denoise_guided_device(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* d_accum,
                              const float* d_moments, const float* d_albedo, const float* d_normal_depth,
                              const rtw_denoise_params* params, float* d_out, float* d_variance_out, void* stream,
                              uint32_t flags) {
    if (int rc = check_params("rtw_denoise_guided", ctx, width, height, d_accum, d_albedo, d_normal_depth, params, d_out))
        return rc;
    if (!d_moments) return rtw_invalid("rtw_denoise_guided: null moments");
    if (int rc = check_device_form(ctx, flags, "host context: use rtw_denoise_guided")) return rc;
    return guided_on_device(ctx, width, height, d_accum, d_moments + 4 * (size_t)width * height, d_albedo, d_normal_depth,
                            params, d_out, d_variance_out, stream, flags);
}

int rtw_denoise_guided(rtw_ctx* ctx, uint32_t width, uint32_t height, const float* accum, const float* moments,
                       const float* albedo, const float* normal_depth, const rtw_denoise_params* params, float* out,
                       float* variance_out) {
    if (int rc = check_params("rtw_denoise_guided", ctx, width, height, accum, albedo, normal_depth, params, out)) return rc;
    if (!moments) return rtw_invalid("rtw_denoise_guided: null moments");
    const size_t n = (size_t)width * height;
    if (ctx->device == RTW_DEVICE_CPU) {
        std::lock_guard<std::mutex> lock(ctx->mu);  // the planes are the context's
        host_guided(ctx, width, height, reinterpret_cast<const float4*>(accum),
                    reinterpret_cast<const float4*>(moments) + n, reinterpret_cast<const float4*>(albedo),
                    reinterpret_cast<const float4*>(normal_depth), *params, reinterpret_cast<float4*>(out), variance_out);
        return RTW_OK;
    }
    // GPU context: accum (and the result, in place), normal_depth, the moments' second plane, albedo, the variance
    DnStaging st;
    if (int rc = st.alloc(ctx, 4 * n * 16 + n * 4)) return rc;
    const size_t nf = 4 * n;
    float *d_nd = st.d + nf, *d_m1 = st.d + 2 * nf, *d_al = st.d + 3 * nf, *d_var = st.d + 4 * nf;
    hipError_t e = hipMemcpy(st.d, accum, n * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_nd, normal_depth, n * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_m1, moments + nf, n * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess && albedo) e = hipMemcpy(d_al, albedo, n * 16, hipMemcpyHostToDevice);
    int rc = RTW_OK;
    if (e == hipSuccess)
        rc = guided_on_device(ctx, width, height, st.d, d_m1, albedo ? d_al : nullptr, d_nd, params, st.d,
                              variance_out ? d_var : nullptr, nullptr, 0);
    if (e == hipSuccess && rc == RTW_OK) e = hipMemcpy(out, st.d, n * 16, hipMemcpyDeviceToHost);
    if (e == hipSuccess && rc == RTW_OK && variance_out) e = hipMemcpy(variance_out, d_var, n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return rtw_hip_fail(e, "rtw_denoise_guided staging");
    return rc;
}

int rtw_debug_expneg(uint32_t n, const float* x, float* out) {
    if (n && (!x || !out)) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) out[i] = rtw_expneg(x[i]);
    return RTW_OK;
}

}  // extern "C"
