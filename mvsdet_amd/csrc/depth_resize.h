// What the depth diagnostics (backproject.hip) and the depth losses (depthloss.hip) share: ATen's bilinear resize of the
// ground-truth depth in ATen's own op order.
#pragma once
#include "common.h"

namespace mvsdet {

// at::native::compute_source_index_and_lambda (UpSample.h) in fp32.  The source index is ONE fused multiply-add, as the
// CPU build of ATen contracts `scale * (dst + 0.5f) - 0.5f`.
__device__ __forceinline__ void resize_taps(int dst, float scale, int in, int out, int& i0, int& i1, float& l0, float& l1) {
    if (in == out) {
        i0 = i1 = dst;
        l0 = 1.0f;
        l1 = 0.0f;
        return;
    }
    float src = fmaf(scale, (float)dst + 0.5f, -0.5f);
    if (src < 0.0f) src = 0.0f;
    i0 = min((int)floorf(src), in - 1);
    l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l0 = 1.0f - l1;
}

// Pixel (y, x) of view `src` (Hg x Wg, element strides s1, s2) resized to (h, w): upsample_bilinear2d(align_corners=False).
__device__ __forceinline__ float resized_at(const float* __restrict__ src, int64_t s1, int64_t s2, int y, int x, int h, int w, int Hg,
                                            int Wg, float scale_y, float scale_x) {
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    resize_taps(y, scale_y, Hg, h, y0, y1, ly0, ly1);
    resize_taps(x, scale_x, Wg, w, x0, x1, lx0, lx1);
    const float a = src[(int64_t)y0 * s1 + (int64_t)x0 * s2], b = src[(int64_t)y0 * s1 + (int64_t)x1 * s2];
    const float c = src[(int64_t)y1 * s1 + (int64_t)x0 * s2], d = src[(int64_t)y1 * s1 + (int64_t)x1 * s2];
    return ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d);
}

}  // namespace mvsdet
