// Clipping of a rectangle's edges against another rectangle, shared by RotatedIoU3DLoss (assign.hip: rotated_iou_loss, which also
// needs the clipped lengths for its gradient) and the evaluator's IoU (evalmap.hip).  Method and conventions at degenerate pairs:
// the header of assign.hip.
#pragma once
#include "common.h"

namespace mvsdet {

// The part [t0, t1] of the segment m + tau * t, |tau| <= half, inside one axis of an axis-aligned rectangle (|coordinate| <= w).
// m, t, n: that coordinate of the segment's midpoint, direction and outward normal.  A segment along the axis' boundary (t == 0,
// |m| == w) counts where on_edge and the two outward normals agree (file header).
__device__ __forceinline__ void clip_axis(float m, float t, float n, float w, bool on_edge, float& t0, float& t1) {
    if (t == 0.f) {
        const bool in = fabsf(m) < w || (on_edge && fabsf(m) == w && m * n > 0.f);
        if (!in) t1 = t0;
    } else {
        const float a = (-w - m) / t, b = (w - m) / t;
        t0 = fmaxf(t0, fminf(a, b));
        t1 = fminf(t1, fmaxf(a, b));
    }
}

// Edge k (0..3, counter-clockwise: normals +x, +y, -x, -y of its own frame) of a rectangle with half sizes (hw, hl), centre
// (rx, ry) and axes rotated by (c, s) in the frame of an axis-aligned rectangle with half sizes (ow, ol): its inside part
// [t0, t1] along the edge from its midpoint (t1 <= t0: none), and tx, ty its direction there
template <int k>
__device__ __forceinline__ void clip_edge(float rx, float ry, float c, float s, float hw, float hl, float ow, float ol, bool on_edge,
                                          float& t0, float& t1, float& tx, float& ty) {
    constexpr float nxl = k == 0 ? 1.f : k == 2 ? -1.f : 0.f, nyl = k == 1 ? 1.f : k == 3 ? -1.f : 0.f;
    const float nx = nxl * c - nyl * s, ny = nxl * s + nyl * c;
    const float h = (k & 1) ? hl : hw, half = (k & 1) ? hw : hl;
    tx = -ny, ty = nx;
    t0 = -half, t1 = half;
    clip_axis(rx + h * nx, tx, nx, ow, on_edge, t0, t1);
    clip_axis(ry + h * ny, ty, ny, ol, on_edge, t0, t1);
    t1 = fmaxf(t1, t0);
}

// Area of the intersection of rectangle A (centre, sizes aw x al, heading ya) with rectangle B: the forward value of
// rotated_iou_loss' footprint term, by the same sums in the same order (A's edges clipped in B's frame, B's in A's, Green's sum;
// parallel axes: the product of the two overlaps along B's axes).
__device__ __forceinline__ float rect_intersection_area(float ax, float ay, float aw, float al, float ya, float bx, float by, float bw,
                                                        float bl, float yb) {
    const float hw = aw / 2.f, hl = al / 2.f, ow = bw / 2.f, ol = bl / 2.f;
    const float cb = cosf(yb), sb = sinf(yb);
    const float ex = ax - bx, ey = ay - by;
    const float rx = ex * cb + ey * sb, ry = ey * cb - ex * sb;
    const float theta = ya - yb;
    float c = cosf(theta), s = sinf(theta);
    if (fabsf(s) < 1e-6f) {
        s = 0.f;
        c = c < 0.f ? -1.f : 1.f;
    } else if (fabsf(c) < 1e-6f) {
        c = 0.f;
        s = s < 0.f ? -1.f : 1.f;
    }
    float twice = 0.f;
    if (s == 0.f || c == 0.f) {
        const float hx = s == 0.f ? hw : hl, hy = s == 0.f ? hl : hw;
        const float ox = fminf(rx + hx, ow) - fmaxf(rx - hx, -ow), oy = fminf(ry + hy, ol) - fmaxf(ry - hy, -ol);
        twice = 2.f * fmaxf(ox, 0.f) * fmaxf(oy, 0.f);
    } else {
        const float qx = -(rx * c + ry * s), qy = -(ry * c - rx * s);
        float t0, t1, tx, ty;
        clip_edge<0>(rx, ry, c, s, hw, hl, ow, ol, true, t0, t1, tx, ty);
        twice += (rx * ty - ry * tx + hw) * (t1 - t0);
        clip_edge<1>(rx, ry, c, s, hw, hl, ow, ol, true, t0, t1, tx, ty);
        twice += (rx * ty - ry * tx + hl) * (t1 - t0);
        clip_edge<2>(rx, ry, c, s, hw, hl, ow, ol, true, t0, t1, tx, ty);
        twice += (rx * ty - ry * tx + hw) * (t1 - t0);
        clip_edge<3>(rx, ry, c, s, hw, hl, ow, ol, true, t0, t1, tx, ty);
        twice += (rx * ty - ry * tx + hl) * (t1 - t0);
        clip_edge<0>(qx, qy, c, -s, ow, ol, hw, hl, false, t0, t1, tx, ty);
        twice += ow * (t1 - t0);
        clip_edge<1>(qx, qy, c, -s, ow, ol, hw, hl, false, t0, t1, tx, ty);
        twice += ol * (t1 - t0);
        clip_edge<2>(qx, qy, c, -s, ow, ol, hw, hl, false, t0, t1, tx, ty);
        twice += ow * (t1 - t0);
        clip_edge<3>(qx, qy, c, -s, ow, ol, hw, hl, false, t0, t1, tx, ty);
        twice += ol * (t1 - t0);
    }
    return fmaxf(twice / 2.f, 0.f);
}

}  // namespace mvsdet
