// rtw_temporal.hip -- temporal reprojection (include/rtw_gpu.h, DESIGN.md §Temporal reprojection): SVGF's temporal
// half (Schied et al. 2017).  When the camera moves, the accumulator and the luminance moments of the previous camera
// are carried onto the new one: each pixel's first hit, known from the guide buffers, is looked up where the previous
// camera saw it.  A kernel of its own: no render kernel, class table or launch is touched.
//
// One RTW_DHD function per pixel, run by a gfx950 kernel (one lane per pixel, blocks of 32 x 8 pixels as
// guides_kernel's) and by the host backend's threads -- the same fp32 operations in the same order
// (-ffp-contract=off, correctly rounded division and square root), so a GPU context and a host context agree bit for
// bit.  The taps are gathered through L1 / L2: neighbouring lanes reproject to neighbouring footprints and share
// their lines; nothing is staged in LDS (under a free camera a block's footprint is no fixed halo), no atomics, no
// scratch.
//
// The association (the header states it for callers), dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z:
//   look     d = ((pixel00 + du (x + off)) + dv (y + off)) - c_cur;  u = d / sqrt(dot(d, d)) per component
//            hit (depth > 0): p = c_cur + u depth;  e = p - c_prev;  dist = sqrt(dot(e, e))      miss: e = u
//   project  lambda = na / dot(n, e), n = cross(du', dv'), a = pixel00' - c_prev, na = dot(n, a) (the previous
//            camera's, once per call on the host);  no history unless 0 < lambda < inf
//            r = e lambda - a;  fx = dot(r, du') / dot(du', du') - off';  fy likewise with dv'
//   snap     rx = floor(fx + 1/2), ry likewise;  |fx - rx| <= S and |fy - ry| <= S: the one tap (rx, ry), weight 1
//   taps     else x0 = floor(fx), tx = fx - x0 (y likewise): (x0, y0) (1 - tx)(1 - ty), (x0 + 1, y0) tx (1 - ty),
//            (x0, y0 + 1) (1 - tx) ty, (x0 + 1, y0 + 1) tx ty, in this order; a tap of weight 0 is skipped
//   valid    on the image; accumulator finite, w > 0; (depth_q > 0) == hit; for hits
//            |depth_q - dist| <= tol dist and dot(n_cur, n_q) >= normal_cos
//   hidden   hit centre: an on-image tap of weight > 0 with 0 < depth_q and dist - depth_q > tol dist saw a nearer
//            surface -- the footprint straddles an occluder's silhouette -- and no tap is valid
//   blend    ws = sum of the valid weights;  g_q = weight_q / ws;  h_i = sum g_q w_q;
//            mean = sum g_q (rgb_q (1 / w_q));  h = min(h_i, max_history)
//            out = (mean h + cur.rgb, h + cur.w);  h = 0: out = cur;  cur not finite or w <= 0: out = (mean h, h)
//   moments  over the valid taps with n_q >= 1: g'_q = weight_q / (their sum);  m = sum g'_q m_q;
//            h_i > max_history: m.sw = m.sw (h / h_i);  then West's update by y = luma(cur.rgb (1 / cur.w)), k = cur.w
//            (mo_batch_luma, mo_west of rtw_moments.h) unless cur is not valid or y not finite
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "rtw_device.h"
#include "rtw_moments.h"

namespace {

constexpr float kSnap = RTW_TEMPORAL_SNAP;

// What reprojecting onto the previous camera reads of it: computed once per call on the host, passed by value
struct TpPrev {
    float c[3];        // its centre
    float n[3];        // cross(du, dv): the viewport plane's normal, towards the scene
    float a[3];        // pixel00 - c
    float na;          // dot(n, a) > 0
    float du[3], dv[3];
    float uu, vv;      // dot(du, du), dot(dv, dv)
    float off;         // pixel_offset
};
struct TpArgs {
    TpPrev prev;
    float c[3], pixel00[3], du[3], dv[3];  // the current camera
    uint32_t off;
    uint32_t W, H;
    float max_history, depth_tol, normal_cos;
    const float4 *cur, *cur_nd, *prev_acc, *prev_nd;
    const float4* prev_m1;  // plane 1 of the previous moments, or null
    float4* out;
    float4* out_m;          // both planes, or null
    float* hist;            // or null
};

TpPrev tp_prev(const rtw_camera& cam) {
    TpPrev P{};
    const f3 c = ld3(cam.center), du = ld3(cam.pixel_delta_u), dv = ld3(cam.pixel_delta_v);
    const f3 n = cross(du, dv), a = ld3(cam.pixel00_loc) - c;
    const float v[5][3] = {{c.x, c.y, c.z}, {n.x, n.y, n.z}, {a.x, a.y, a.z}, {du.x, du.y, du.z}, {dv.x, dv.y, dv.z}};
    memcpy(P.c, v[0], 12);
    memcpy(P.n, v[1], 12);
    memcpy(P.a, v[2], 12);
    memcpy(P.du, v[3], 12);
    memcpy(P.dv, v[4], 12);
    P.na = dot(n, a);
    P.uu = dot(du, du);
    P.vv = dot(dv, dv);
    P.off = (float)cam.pixel_offset;
    return P;
}

// Where the previous camera saw the point c_prev + e (any positive multiple of e): the fractional pixel coordinates
// of the line's intersection with its viewport plane.  False: behind the camera, parallel to the plane or not finite.
RTW_DHD bool tp_project(const TpPrev& P, f3 e, float& fx, float& fy) {
    const float lambda = P.na / dot(ld3(P.n), e);
    if (!(lambda > 0.0f) || !(lambda <= 3.4028234e38f)) return false;
    const f3 r = e * splat(lambda) - ld3(P.a);
    fx = dot(r, ld3(P.du)) / P.uu - P.off;
    fy = dot(r, ld3(P.dv)) / P.vv - P.off;
    return dn_finite1(fx) && dn_finite1(fy);
}

RTW_DHD bool tp_valid_accum(float4 a) { return dn_finite3(a) && dn_finite1(a.w) && a.w > 0.0f; }

RTW_DHD void tp_pixel(const TpArgs& A, uint32_t x, uint32_t y) {
    const size_t p = (size_t)y * A.W + x;
    const float4 cur = A.cur[p], nd = A.cur_nd[p];
    const bool hit = nd.w > 0.0f;
    // where the pixel looks
    const f3 cc = ld3(A.c);
    const f3 d = ((ld3(A.pixel00) + ld3(A.du) * splat((float)(x + A.off))) + ld3(A.dv) * splat((float)(y + A.off))) - cc;
    const float len = __builtin_sqrtf(dot(d, d));
    const f3 u = mk(d.x / len, d.y / len, d.z / len);
    f3 e = u;
    float dist = 0.0f;
    if (hit) {
        e = (cc + u * splat(nd.w)) - ld3(A.prev.c);
        dist = __builtin_sqrtf(dot(e, e));
    }
    // where the previous camera saw it: up to four taps (tap k at (qx + (k & 1), qy + (k >> 1)))
    float wg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int64_t qx = 0, qy = 0;
    float fx, fy;
    if (tp_project(A.prev, e, fx, fy) && fx > -1.0f && fx < (float)A.W && fy > -1.0f && fy < (float)A.H) {
        const float rx = __builtin_floorf(fx + 0.5f), ry = __builtin_floorf(fy + 0.5f);
        if (__builtin_fabsf(fx - rx) <= kSnap && __builtin_fabsf(fy - ry) <= kSnap) {
            qx = (int64_t)rx;
            qy = (int64_t)ry;
            wg[0] = 1.0f;
        } else {
            const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
            const float tx = fx - x0, ty = fy - y0;
            qx = (int64_t)x0;
            qy = (int64_t)y0;
            wg[0] = (1.0f - tx) * (1.0f - ty);
            wg[1] = tx * (1.0f - ty);
            wg[2] = (1.0f - tx) * ty;
            wg[3] = tx * ty;
        }
    }
    float4 ta[4];
    size_t tq[4];
    float ws = 0.0f;
    const float slack = A.depth_tol * dist;
    bool occluded = false;  // a tap of the footprint saw a nearer surface: the point may have been hidden
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int64_t tx = qx + (k & 1), ty = qy + (k >> 1);
        tq[k] = 0;
        ta[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool ok = wg[k] > 0.0f && tx >= 0 && tx < (int64_t)A.W && ty >= 0 && ty < (int64_t)A.H;
        if (ok) {
            tq[k] = (size_t)ty * A.W + (size_t)tx;
            ta[k] = A.prev_acc[tq[k]];
            const float4 tn = A.prev_nd[tq[k]];
            ok = tp_valid_accum(ta[k]) && (tn.w > 0.0f) == hit;
            if (hit && tn.w > 0.0f) {
                occluded = occluded || dist - tn.w > slack;
                ok = ok && __builtin_fabsf(tn.w - dist) <= slack &&
                     dot(mk(nd.x, nd.y, nd.z), mk(tn.x, tn.y, tn.z)) >= A.normal_cos;
            }
        }
        if (!ok) wg[k] = 0.0f;
        ws += wg[k];
    }
    if (occluded) {
        wg[0] = wg[1] = wg[2] = wg[3] = 0.0f;
        ws = 0.0f;
    }
    // blend
    float hi = 0.0f, mr = 0.0f, mg = 0.0f, mb = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (wg[k] > 0.0f) {
            const float g = wg[k] / ws, inv = 1.0f / ta[k].w;
            hi += g * ta[k].w;
            mr += g * (ta[k].x * inv);
            mg += g * (ta[k].y * inv);
            mb += g * (ta[k].z * inv);
        }
    const float h = hi < A.max_history ? hi : A.max_history;
    const bool cur_ok = tp_valid_accum(cur);
    float4 o;
    if (!(h > 0.0f)) o = cur_ok ? cur : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    else if (cur_ok) o = make_float4(mr * h + cur.x, mg * h + cur.y, mb * h + cur.z, h + cur.w);
    else o = make_float4(mr * h, mg * h, mb * h, h);
    A.out[p] = o;
    if (A.hist) A.hist[p] = h > 0.0f ? h : 0.0f;
    if (!A.out_m) return;
    // moments
    float4 tm[4];
    float wm = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        tm[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (wg[k] > 0.0f) {
            tm[k] = A.prev_m1[tq[k]];
            if (!(tm[k].z >= 1.0f)) wg[k] = 0.0f;
        }
        wm += wg[k];
    }
    float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (wg[k] > 0.0f) {
            const float g = wg[k] / wm;
            m.x += g * tm[k].x;
            m.y += g * tm[k].y;
            m.z += g * tm[k].z;
            m.w += g * tm[k].w;
        }
    if (hi > A.max_history) m.w = m.w * (h / hi);
    if (cur_ok) {
        const float yl = mo_batch_luma(cur.x, cur.y, cur.z, cur.w);
        if (dn_finite1(yl)) mo_west(m, yl, cur.w);
    }
    A.out_m[p] = o;
    A.out_m[(size_t)A.W * A.H + p] = m;
}

// Blocks of 32 x 8 pixels, as guides_kernel's.  -DRTW_TEMPORAL_BLOCK_W=64 builds the A/B's other side, 64 x 4 (a wave
// per row of 1 KiB; profiles/temporal/README.md).
#ifndef RTW_TEMPORAL_BLOCK_W
#define RTW_TEMPORAL_BLOCK_W 32
#endif
constexpr uint32_t kBlockW = RTW_TEMPORAL_BLOCK_W, kBlockH = 256 / kBlockW;
static_assert(kBlockW == 32 || kBlockW == 64, "blocks of 32 x 8 or 64 x 4 pixels");
__global__ __launch_bounds__(256) void temporal_kernel(TpArgs A) {
    const uint32_t x = blockIdx.x * kBlockW + (threadIdx.x & (kBlockW - 1)), y = blockIdx.y * kBlockH + threadIdx.x / kBlockW;
    if (x >= A.W || y >= A.H) return;
    tp_pixel(A, x, y);
}

int refuse(const char* what) {
    char msg[160];
    snprintf(msg, sizeof msg, "rtw_temporal_accumulate: %s", what);
    return rtw_invalid(msg);
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// every refusal of the two entry points but the kind of context; fills A on success
int check_and_fill(const rtw_ctx* ctx, const rtw_camera* cur_cam, const rtw_camera* prev_cam, const float* cur_accum,
                   const float* cur_nd, const float* prev_accum, const float* prev_nd, const float* prev_moments,
                   const rtw_temporal_params* p, float* out_accum, float* out_moments, float* history_out, TpArgs& A) {
    if (!ctx || !cur_cam || !prev_cam || !cur_accum || !cur_nd || !prev_accum || !prev_nd || !p || !out_accum)
        return refuse("null ctx / camera / accum / normal_depth / params / out_accum");
    if (int rc = rtw_validate_cam(cur_cam)) return rc;
    if (int rc = rtw_validate_cam(prev_cam)) return rc;
    const uint32_t W = cur_cam->image_width, H = cur_cam->image_height;
    if (W == 0 || H == 0 || (uint64_t)W * H > 0xFFFFFFFFull) return refuse("width * height == 0 or too large");
    if (prev_cam->image_width != W || prev_cam->image_height != H) return refuse("the cameras' images differ in size");
    if ((prev_moments == nullptr) != (out_moments == nullptr)) return refuse("prev_moments and out_moments go together");
    if (p->flags) return refuse("unknown flag bits");
    if (!(p->max_history > 0.0f) || !(p->max_history <= 3.4028234e38f)) return refuse("max_history is not > 0 and finite");
    if (!(p->depth_tolerance > 0.0f) || !(p->depth_tolerance <= 3.4028234e38f))
        return refuse("depth_tolerance is not > 0 and finite");
    if (!(p->normal_cos >= -1.0f) || !(p->normal_cos <= 1.0f)) return refuse("normal_cos outside [-1, 1]");
    const size_t n = (size_t)W * H;
    const void* gathered[3] = {prev_accum, prev_nd, prev_moments};
    const size_t gbytes[3] = {n * 16, n * 16, n * 32};
    const void* outs[3] = {out_accum, out_moments, history_out};
    const size_t obytes[3] = {n * 16, n * 32, n * 4};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            if (overlap(outs[i], obytes[i], gathered[j], gbytes[j])) return refuse("an output aliases a prev_* buffer");
    if (overlap(out_moments, n * 32, cur_accum, n * 16) || overlap(out_moments, n * 32, cur_nd, n * 16) ||
        overlap(out_moments, n * 32, out_accum, n * 16) || overlap(history_out, n * 4, out_accum, n * 16) ||
        overlap(history_out, n * 4, out_moments, n * 32) || overlap(history_out, n * 4, cur_accum, n * 16) ||
        overlap(history_out, n * 4, cur_nd, n * 16) || overlap(out_accum, n * 16, cur_nd, n * 16))
        return refuse("out_moments / history_out alias another buffer");
    if (out_accum != cur_accum && overlap(out_accum, n * 16, cur_accum, n * 16))
        return refuse("out_accum overlaps cur_accum without being it");
    A = TpArgs{};
    A.prev = tp_prev(*prev_cam);
    memcpy(A.c, cur_cam->center, 12);
    memcpy(A.pixel00, cur_cam->pixel00_loc, 12);
    memcpy(A.du, cur_cam->pixel_delta_u, 12);
    memcpy(A.dv, cur_cam->pixel_delta_v, 12);
    A.off = cur_cam->pixel_offset;
    A.W = W;
    A.H = H;
    A.max_history = p->max_history;
    A.depth_tol = p->depth_tolerance;
    A.normal_cos = p->normal_cos;
    A.cur = reinterpret_cast<const float4*>(cur_accum);
    A.cur_nd = reinterpret_cast<const float4*>(cur_nd);
    A.prev_acc = reinterpret_cast<const float4*>(prev_accum);
    A.prev_nd = reinterpret_cast<const float4*>(prev_nd);
    A.prev_m1 = prev_moments ? reinterpret_cast<const float4*>(prev_moments) + n : nullptr;
    A.out = reinterpret_cast<float4*>(out_accum);
    A.out_m = reinterpret_cast<float4*>(out_moments);
    A.hist = history_out;
    return RTW_OK;
}

// a device block of this call's (the host-buffer entry point of a GPU context stages through one)
struct TpStaging {
    float* d = nullptr;
    ~TpStaging() {
        if (d) (void)hipFree(d);
    }
    int alloc(rtw_ctx* ctx, size_t bytes) {
        std::lock_guard<std::mutex> lock(ctx->mu);
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), bytes));
        return RTW_OK;
    }
};

}  // namespace

extern "C" {

void rtw_temporal_defaults(rtw_temporal_params* p) {
    if (!p) return;
    // profiles/temporal/defaults.json: the winner of the grid search (tools/temporal_defaults.py) over Cornell orbits
    // at 2 spp per frame, scored 0.43 (the mean of RMSE ratios against starting over, raw and under the guided filter).
    // A loose depth test: on a wall seen at a grazing angle neighbouring pixels differ by several per cent in depth
    *p = rtw_temporal_params{};
    p->max_history = 32.0f;
    p->depth_tolerance = 0.2f;
    p->normal_cos = 0.9f;
    p->flags = 0;
}

int rtw_temporal_accumulate_device(rtw_ctx* ctx, const rtw_camera* cur_cam, const rtw_camera* prev_cam,
                                   const float* d_cur_accum, const float* d_cur_normal_depth, const float* d_prev_accum,
                                   const float* d_prev_normal_depth, const float* d_prev_moments,
                                   const rtw_temporal_params* params, float* d_out_accum, float* d_out_moments,
                                   float* d_history_out, void* stream, uint32_t flags) {
    TpArgs A;
    if (int rc = check_and_fill(ctx, cur_cam, prev_cam, d_cur_accum, d_cur_normal_depth, d_prev_accum, d_prev_normal_depth,
                                d_prev_moments, params, d_out_accum, d_out_moments, d_history_out, A))
        return rc;
    if (ctx->device == RTW_DEVICE_CPU) return rtw_invalid("host context: use rtw_temporal_accumulate");
    if (flags & ~(uint32_t)RTW_RENDER_NO_SYNC) return refuse("unknown flag bits");
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (int rc = rtw_stream_enter(ctx, s)) return rc;
    hipLaunchKernelGGL(temporal_kernel, dim3((A.W + kBlockW - 1) / kBlockW, (A.H + kBlockH - 1) / kBlockH), dim3(256), 0, s,
                       A);
    HIP_TRY(hipGetLastError());
    if (int rc = rtw_stream_leave(ctx, s)) return rc;
    if (!(flags & RTW_RENDER_NO_SYNC)) HIP_TRY(hipStreamSynchronize(s));
    return RTW_OK;
}

int rtw_temporal_accumulate(rtw_ctx* ctx, const rtw_camera* cur_cam, const rtw_camera* prev_cam, const float* cur_accum,
                            const float* cur_normal_depth, const float* prev_accum, const float* prev_normal_depth,
                            const float* prev_moments, const rtw_temporal_params* params, float* out_accum,
                            float* out_moments, float* history_out) {
    TpArgs A;
    if (int rc = check_and_fill(ctx, cur_cam, prev_cam, cur_accum, cur_normal_depth, prev_accum, prev_normal_depth,
                                prev_moments, params, out_accum, out_moments, history_out, A))
        return rc;
    if (ctx->device == RTW_DEVICE_CPU) {
        rtw_host_ranges(A.H, ctx->cpu_threads, 1, [&](uint32_t y0, uint32_t y1) {
            for (uint32_t y = y0; y < y1; y++)
                for (uint32_t x = 0; x < A.W; x++) tp_pixel(A, x, y);
        });
        return RTW_OK;
    }
    // GPU context: cur_accum (and out_accum, in place), the three other frames, plane 1 of the previous moments where
    // the device form reads it, the two planes of out_moments, the history
    const size_t n = (size_t)A.W * A.H, nf = 4 * n;
    TpStaging st;
    if (int rc = st.alloc(ctx, (4 * nf + (prev_moments ? 4 * nf : 0) + n) * 4)) return rc;
    float *d_cur = st.d, *d_cnd = st.d + nf, *d_prev = st.d + 2 * nf, *d_pnd = st.d + 3 * nf, *d_hist = st.d + 4 * nf;
    float *d_pm = prev_moments ? d_hist + n : nullptr, *d_om = prev_moments ? d_pm + 2 * nf : nullptr;
    hipError_t e = hipMemcpy(d_cur, cur_accum, nf * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_cnd, cur_normal_depth, nf * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_prev, prev_accum, nf * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_pnd, prev_normal_depth, nf * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && prev_moments) e = hipMemcpy(d_pm + nf, prev_moments + nf, nf * 4, hipMemcpyHostToDevice);
    int rc = RTW_OK;
    if (e == hipSuccess)
        rc = rtw_temporal_accumulate_device(ctx, cur_cam, prev_cam, d_cur, d_cnd, d_prev, d_pnd, d_pm, params, d_cur, d_om,
                                            history_out ? d_hist : nullptr, nullptr, 0);
    if (e == hipSuccess && rc == RTW_OK) e = hipMemcpy(out_accum, d_cur, nf * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && rc == RTW_OK && out_moments) e = hipMemcpy(out_moments, d_om, 2 * nf * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && rc == RTW_OK && history_out) e = hipMemcpy(history_out, d_hist, n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return rtw_hip_fail(e, "rtw_temporal_accumulate staging");
    return rc;
}

int rtw_debug_reproject(const rtw_camera* prev_cam, uint32_t n, const float* points, const float* dirs, float* xy,
                        uint8_t* ok) {
    if (int rc = rtw_validate_cam(prev_cam)) return rc;
    if ((points == nullptr) == (dirs == nullptr)) return rtw_invalid("rtw_debug_reproject: give points or dirs, not both");
    if (n && (!xy || !ok)) return rtw_invalid("rtw_debug_reproject: null xy / ok");
    const TpPrev P = tp_prev(*prev_cam);
    for (uint32_t i = 0; i < n; i++) {
        const f3 e = points ? ld3(points + 3 * (size_t)i) - ld3(P.c) : ld3(dirs + 3 * (size_t)i);
        float fx = 0.0f, fy = 0.0f;
        ok[i] = tp_project(P, e, fx, fy) ? 1 : 0;
        xy[2 * (size_t)i] = ok[i] ? fx : 0.0f;
        xy[2 * (size_t)i + 1] = ok[i] ? fy : 0.0f;
    }
    return RTW_OK;
}

}  // extern "C"
