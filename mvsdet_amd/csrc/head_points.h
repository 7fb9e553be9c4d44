// What the detection decode (detect.hip) and the target assignment / losses (assign.hip) share of the head's geometry: the
// upsampled valid mask, get_points of a voxel, and the radix select of the k-th largest value by its float bits.
#pragma once
#include "common.h"

namespace mvsdet {

// aten/src/ATen/native/UpSample.h: area_pixel_compute_source_index + guard_index_and_lambda (align_corners = False)
__device__ __forceinline__ void linear_taps(float scale, int d, int in, int& i0, int& i1, float& l0, float& l1) {
    float r = scale * ((float)d + 0.5f) - 0.5f;
    if (r < 0.f) r = 0.f;
    const int i = min((int)floorf(r), in - 1);
    const float lam = fminf(fmaxf(r - (float)i, 0.f), 1.f);
    i0 = i;
    i1 = i + (i < in - 1 ? 1 : 0);
    l1 = lam;
    l0 = 1.f - lam;
}

// nn.Upsample(trilinear)(valid).round().bool() at voxel (x, y, z) of a level, as 0 / 1.  valid: one scene's (VX, VY, VZ) view
// counts; (sx, sy, sz) the trilinear scales (float)in / out of the level
__device__ __forceinline__ float upsampled_valid(const float* valid, int VX, int VY, int VZ, float sx, float sy, float sz, int x, int y,
                                                 int z) {
    int x0, x1, y0, y1, z0, z1;
    float ax0, ax1, ay0, ay1, az0, az1;
    linear_taps(sx, x, VX, x0, x1, ax0, ax1);
    linear_taps(sy, y, VY, y0, y1, ay0, ay1);
    linear_taps(sz, z, VZ, z0, z1, az0, az1);
    auto at = [&](int xi, int yi, int zi) { return valid[((size_t)xi * VY + yi) * VZ + zi]; };
    auto zl = [&](int xi, int yi) { float t = at(xi, yi, z0) * az0; t += at(xi, yi, z1) * az1; return t; };
    auto yl = [&](int xi) { float t = zl(xi, y0) * ay0; t += zl(xi, y1) * ay1; return t; };
    float v = yl(x0) * ax0;
    v += yl(x1) * ax1;
    return rintf(v) != 0.f ? 1.f : 0.f;
}

// get_points of voxel (x, y, z): voxel * voxel size + new origin (g: voxel size, new origin -- a row of the (B, L, 6) geometry)
__device__ __forceinline__ void grid_point(const float* g, int x, int y, int z, float& px, float& py, float& pz) {
    px = (float)x * g[0], py = (float)y * g[1], pz = (float)z * g[2];
    px = px + g[3];
    py = py + g[4];
    pz = pz + g[5];
}

// The k-th largest (k >= 1) of the values whose bits bits_of(i, u) hands out (returning false leaves element i out), i < n, by
// the whole workgroup, 8 bits a pass.  The values are >= +0, so their bits order like the values.  At least k elements must take
// part.  Returns the bits T of that value; need_eq = how many elements with bits == T belong to the k largest.
// hist: 256 ints of LDS, sel: 2.
template <class BitsOf>
__device__ __forceinline__ unsigned radix_select_kth(int* hist, int* sel, int n, int k, int& need_eq, BitsOf bits_of) {
    const int tid = threadIdx.x, nt = blockDim.x;
    unsigned prefix = 0, pmask = 0;
    int kk = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int d = tid; d < 256; d += nt) hist[d] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += nt) {
            unsigned u;
            if (bits_of(i, u) && (u & pmask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int acc = 0, d = 255;
            for (; d > 0; --d) {
                if (acc + hist[d] >= kk) break;
                acc += hist[d];
            }
            sel[0] = d;
            sel[1] = kk - acc;
        }
        __syncthreads();
        prefix |= (unsigned)sel[0] << shift;
        pmask |= 255u << shift;
        kk = sel[1];
        __syncthreads();
    }
    need_eq = kk;
    return prefix;
}

}  // namespace mvsdet
