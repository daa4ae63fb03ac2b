// rtw_moments.h -- what the filters of rtw_denoise.hip and the temporal reprojection of rtw_temporal.hip share, one
// definition each: the luminance, the finiteness tests on the bit patterns and West's weighted update of a pixel's
// running moments (include/rtw_gpu.h, "Noise estimates and the variance-guided filter").  Every function is one
// rounded fp32 operation per step in the association written, on the host and on the device.
#pragma once
#include "rtw_device.h"

namespace {

RTW_DHD bool dn_finite1(float v) { return (fbits(v) & 0x7F800000u) != 0x7F800000u; }
RTW_DHD bool dn_finite3(float4 c) {
    return (fbits(c.x) & 0x7F800000u) != 0x7F800000u && (fbits(c.y) & 0x7F800000u) != 0x7F800000u &&
           (fbits(c.z) & 0x7F800000u) != 0x7F800000u;
}
RTW_DHD float dn_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the mean luminance of a batch of k > 0 samples whose radiance sums to (r, g, b)
RTW_DHD float mo_batch_luma(float r, float g, float b, float k) {
    const float inv = 1.0f / k;
    return dn_luma(r * inv, g * inv, b * inv);
}
// West's weighted update of m = (mean, M2, n, sw) by one batch of weight k > 0 and finite mean luminance y
RTW_DHD void mo_west(float4& m, float y, float k) {
    const float sw = m.w + k, e = y - m.x;
    const float mean = m.x + e * (k / sw);
    m = make_float4(mean, m.y + (k * e) * (y - mean), m.z + 1.0f, sw);
}

}  // namespace
