// Training of the ScanNet head: target assignment (NerfDetHead._get_targets, projects/NeRF-Det/nerfdet/nerfdet_head.py:473-562)
// and its three losses (_loss_by_feat_single, :206-257) on the caller's stream, no host round trip, no float atomics.
//
//   assign_count_kernel        grid (box, level, scene): n[l, g] = points of level l inside box g (integer workgroup reduction)
//   assign_select_kernel       one workgroup per (scene, box): best[g] from n[:, g]; centerness of the best level's inside points;
//                              t[g] = the (pts_center_threshold + 1)-th largest by a radix select on the float bits (-1: too few)
//   assign_pick_kernel         one thread per point, the scene's boxes staged in LDS: inside, best level, centerness > t[g]; the
//                              least volume wins, equal volumes the lowest box index; label, box index, centerness and box targets
//   head_loss_kernel           one thread per point, the maps read in place in their (B, c, X, Y, Z) layout: focal / BCE / IoU terms,
//                              a workgroup's sums in a fixed tree
//   head_loss_finish_kernel    one workgroup per scene: the workgroups' partials in index order -> the scene's sums and counts
//   head_loss_backward_kernel  the same walk: d center, d bbox, d cls dense in the maps' layout, scaled by per-scene device scalars
//
// The first two visit only the sub-block of the grid that can hold a box's points (two voxels of margin; the whole level for boxes
// with non-finite or huge coordinates); the inside test itself is the reference's expression on every visited point.  No
// intermediate of size points x boxes exists.  All arithmetic that decides or produces a target is the reference's ATen expression,
// op for op, under -ffp-contract=off with IEEE division and square root.
#include "common.h"
#include "head_points.h"

#include <algorithm>

namespace mvsdet {
namespace {

constexpr int kMaxL = MVSDET_DETECT_MAX_LEVELS;
constexpr int kMaxBoxes = MVSDET_ASSIGN_MAX_BOXES;
constexpr int kCountThreads = 256;
constexpr int kSelThreads = 256;
constexpr int kPointThreads = 256;
constexpr float kFloatMax = 1e8f;   // _get_targets' float_max

struct GridLevel {
    int X, Y, Z;
    int pt_off;            // offset of the level's points in a scene's point list
};

struct AssignParams {
    GridLevel lv[kMaxL];
    const float* geom;     // (B, L, 6): voxel size, new origin
    const float* boxes;    // (B, G, 6): gravity centre, size
    const float* volumes;  // (B, G)
    const long long* labels;   // (B, G)
    const int* counts;     // (B): boxes of the scene
    int L, G, P;
    int assign_thr, center_thr;
    int* n_inside;         // (B, G, kMaxL) workspace
    int* best;             // (B, G)
    float* thr;            // (B, G)
};

struct LossLevel {
    const float* center;   // (B,1,X,Y,Z)
    const float* bbox;     // (B,6,X,Y,Z)
    const float* cls;      // (B,C,X,Y,Z)
    float* d_center;       // gradients in the same layouts (backward only)
    float* d_bbox;
    float* d_cls;
    float sx, sy, sz;      // trilinear scales of the valid upsampling
};

struct LossParams {
    GridLevel lv[kMaxL];
    LossLevel lm[kMaxL];
    const float* valid;    // (B,1,VX,VY,VZ)
    const float* geom;     // (B, L, 6)
    const long long* labels;   // (B, P) of the assignment, -1 = background
    const float* center_t;     // (B, P)
    const float* bbox_t;       // (B, P, 6)
    int L, C, P, VX, VY, VZ;
    float gamma, alpha;
};

// _get_face_distances of point (px, py, pz) to box b = (cx, cy, cz, dx, dy, dz), in the reference's operand order
__device__ __forceinline__ void face_distances(float px, float py, float pz, const float* b, float* d) {
    d[0] = (px - b[0]) + b[3] / 2.f;
    d[1] = (b[0] + b[3] / 2.f) - px;
    d[2] = (py - b[1]) + b[4] / 2.f;
    d[3] = (b[1] + b[4] / 2.f) - py;
    d[4] = (pz - b[2]) + b[5] / 2.f;
    d[5] = (b[2] + b[5] / 2.f) - pz;
}

// bbox_targets[..., :6].min(-1)[0] > 0
__device__ __forceinline__ bool inside_box(const float* d) {
    return fminf(fminf(fminf(d[0], d[1]), fminf(d[2], d[3])), fminf(d[4], d[5])) > 0.f;
}

// _get_centerness: sqrt(xmin / xmax * ymin / ymax * zmin / zmax), left to right
__device__ __forceinline__ float centerness(const float* d) {
    float c = fminf(d[0], d[1]) / fmaxf(d[0], d[1]);
    c = c * fminf(d[2], d[3]);
    c = c / fmaxf(d[2], d[3]);
    c = c * fminf(d[4], d[5]);
    c = c / fmaxf(d[4], d[5]);
    return sqrtf(c);
}

// Voxel indices [a, b) of one axis that can lie strictly inside (c - d / 2, c + d / 2): two voxels of margin on either side, the
// whole axis where the bounds are not finite or too large for the margin to cover the rounding of the point coordinates
__device__ __forceinline__ void axis_range(float c, float d, float vs, float o, int n, int& a, int& b) {
    const float lo = (c - d / 2.f - o) / vs, hi = (c + d / 2.f - o) / vs;
    a = 0;
    b = n;
    if (!(fabsf(lo) < 1e5f && fabsf(hi) < 1e5f)) return;
    a = max(0, (int)floorf(lo) - 2);
    b = min(n, (int)ceilf(hi) + 3);
    if (b < a) b = a;
}

struct SubBlock {
    int x0, y0, z0, nx, ny, nz;
    __device__ __forceinline__ int size() const { return nx * ny * nz; }
    __device__ __forceinline__ void at(int j, int& x, int& y, int& z) const {
        x = x0 + j / (ny * nz), y = y0 + (j / nz) % ny, z = z0 + j % nz;
    }
};

__device__ __forceinline__ SubBlock box_sub_block(const float* b, const float* g, const GridLevel& lv) {
    SubBlock s;
    int e;
    axis_range(b[0], b[3], g[0], g[3], lv.X, s.x0, e);
    s.nx = e - s.x0;
    axis_range(b[1], b[4], g[1], g[4], lv.Y, s.y0, e);
    s.ny = e - s.y0;
    axis_range(b[2], b[5], g[2], g[5], lv.Z, s.z0, e);
    s.nz = e - s.z0;
    return s;
}

// sum of v over the workgroup in a fixed tree (lanes by shuffles, then the waves in order); valid in thread 0
template <class T>
__device__ __forceinline__ T block_sum(T v, T* wave_part) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) wave_part[wave] = v;
    __syncthreads();
    T s = wave_part[0];
    for (int w = 1; w < nw; ++w) s += wave_part[w];
    return s;
}

__global__ __launch_bounds__(kCountThreads) void assign_count_kernel(AssignParams p) {
    __shared__ int part[kCountThreads / 64];
    const int g = blockIdx.x, l = blockIdx.y, b = blockIdx.z;
    if (g >= p.counts[b]) return;
    const GridLevel lv = p.lv[l];
    const float* gp = p.geom + ((size_t)b * p.L + l) * 6;
    const float geo[6] = {gp[0], gp[1], gp[2], gp[3], gp[4], gp[5]};
    const float* bp = p.boxes + ((size_t)b * p.G + g) * 6;
    const float box[6] = {bp[0], bp[1], bp[2], bp[3], bp[4], bp[5]};
    const SubBlock sb = box_sub_block(box, geo, lv);
    int n = 0;
    for (int j = threadIdx.x; j < sb.size(); j += kCountThreads) {
        int x, y, z;
        float px, py, pz, d[6];
        sb.at(j, x, y, z);
        grid_point(geo, x, y, z, px, py, pz);
        face_distances(px, py, pz, box, d);
        n += inside_box(d) ? 1 : 0;
    }
    n = block_sum(n, part);
    if (threadIdx.x == 0) p.n_inside[((size_t)b * p.G + g) * kMaxL + l] = n;
}

__global__ __launch_bounds__(kSelThreads) void assign_select_kernel(AssignParams p) {
    __shared__ int hist[256];
    __shared__ int sel[2];
    const int g = blockIdx.x, b = blockIdx.y;
    if (g >= p.counts[b]) return;
    // best scale (:509-529): the first level with fewer inside points than pts_assign_threshold, minus one, at least 0; the last
    // level where none is below
    const int* n = p.n_inside + ((size_t)b * p.G + g) * kMaxL;
    int best = p.L - 1;
    for (int l = 0; l < p.L; ++l) {
        if (n[l] < p.assign_thr) {
            best = max(l - 1, 0);
            break;
        }
    }
    const GridLevel lv = p.lv[best];
    const float* gp = p.geom + ((size_t)b * p.L + best) * 6;
    const float geo[6] = {gp[0], gp[1], gp[2], gp[3], gp[4], gp[5]};
    const float* bp = p.boxes + ((size_t)b * p.G + g) * 6;
    const float box[6] = {bp[0], bp[1], bp[2], bp[3], bp[4], bp[5]};
    const SubBlock sb = box_sub_block(box, geo, lv);
    // the candidates' centerness bits (an inside point's ratios are positive: bits order like values)
    auto bits_of = [&](int j, unsigned& u) {
        int x, y, z;
        float px, py, pz, d[6];
        sb.at(j, x, y, z);
        grid_point(geo, x, y, z, px, py, pz);
        face_distances(px, py, pz, box, d);
        if (!inside_box(d)) return false;
        u = __float_as_uint(centerness(d));
        return true;
    };
    const int k = p.center_thr + 1;
    float t = -1.f;   // at most pts_center_threshold candidates: the (k+1)-th largest is a -1 of the masked points
    if (n[best] >= k) {   // uniform over the workgroup
        int need_eq;
        t = __uint_as_float(radix_select_kth(hist, sel, sb.size(), k, need_eq, bits_of));
    }
    if (threadIdx.x == 0) {
        p.best[(size_t)b * p.G + g] = best;
        p.thr[(size_t)b * p.G + g] = t;
    }
}

struct StagedBox {
    float b[6];
    float volume, thr;
    int best;
};

__global__ __launch_bounds__(kPointThreads) void assign_pick_kernel(AssignParams p, long long* out_labels, int* out_box,
                                                                    float* out_center, float* out_bbox) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    StagedBox* sb = reinterpret_cast<StagedBox*>(smem);
    const int b = blockIdx.y;
    const int G = min(p.counts[b], p.G);
    for (int g = threadIdx.x; g < G; g += kPointThreads) {
        const size_t r = (size_t)b * p.G + g;
        for (int q = 0; q < 6; ++q) sb[g].b[q] = p.boxes[r * 6 + q];
        sb[g].volume = p.volumes[r];
        sb[g].thr = p.thr[r];
        sb[g].best = p.best[r];
    }
    __syncthreads();
    const int i = blockIdx.x * kPointThreads + threadIdx.x;
    if (i >= p.P) return;
    int l = 0;
    while (l + 1 < p.L && i >= p.lv[l + 1].pt_off) ++l;
    const GridLevel lv = p.lv[l];
    const int v = i - lv.pt_off;
    const int x = v / (lv.Y * lv.Z), y = (v / lv.Z) % lv.Y, z = v % lv.Z;
    const float* gp = p.geom + ((size_t)b * p.L + l) * 6;
    float px, py, pz;
    grid_point(gp, x, y, z, px, py, pz);
    // the least volume among the boxes with inside, best level and top centerness; volumes.min(dim=1) over the masked (1e8)
    // volumes: a volume has to be below 1e8 to win, equal volumes keep the lowest box index
    float vmin = kFloatMax;
    int arg = -1;
    for (int g = 0; g < G; ++g) {
        if (sb[g].best != l) continue;
        float d[6];
        face_distances(px, py, pz, sb[g].b, d);
        if (!inside_box(d)) continue;
        if (!(centerness(d) > sb[g].thr)) continue;
        if (sb[g].volume < vmin) {
            vmin = sb[g].volume;
            arg = g;
        }
    }
    const size_t o = (size_t)b * p.P + i;
    float ct = 0.f, bt[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    long long label = -1;
    if (arg >= 0) {
        float d[6];
        face_distances(px, py, pz, sb[arg].b, d);
        ct = centerness(d);
        bt[0] = px - d[0];
        bt[1] = py - d[2];
        bt[2] = pz - d[4];
        bt[3] = px + d[1];
        bt[4] = py + d[3];
        bt[5] = pz + d[5];
        label = p.labels[(size_t)b * p.G + arg];
    }
    out_labels[o] = label;
    out_box[o] = arg;
    out_center[o] = ct;
    for (int q = 0; q < 6; ++q) out_bbox[o * 6 + q] = bt[q];
}

// ---------------------------------------------------------------------------------------------------------------- losses
struct PointTerms {        // what one point adds to a scene's sums
    float center, bbox, cls, w;
    int pos, valid;
};

struct PointRef {
    int l, v, N;           // level, voxel, voxels of the level
    float px, py, pz;
    bool valid;
    long long label;
};

__device__ __forceinline__ PointRef locate(const LossParams& p, int b, int i) {
    PointRef r;
    r.l = 0;
    while (r.l + 1 < p.L && i >= p.lv[r.l + 1].pt_off) ++r.l;
    const GridLevel lv = p.lv[r.l];
    const LossLevel& lm = p.lm[r.l];
    r.v = i - lv.pt_off;
    r.N = lv.X * lv.Y * lv.Z;
    const int x = r.v / (lv.Y * lv.Z), y = (r.v / lv.Z) % lv.Y, z = r.v % lv.Z;
    grid_point(p.geom + ((size_t)b * p.L + r.l) * 6, x, y, z, r.px, r.py, r.pz);
    r.valid = upsampled_valid(p.valid + (size_t)b * p.VX * p.VY * p.VZ, p.VX, p.VY, p.VZ, lm.sx, lm.sy, lm.sz, x, y, z) != 0.f;
    r.label = p.labels[(size_t)b * p.P + i];
    return r;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// mmcv's sigmoid focal loss of one (point, class) logit: the positive term where the point's label is the class, else the
// negative one (a label of -1 is background in every class)
__device__ __forceinline__ float focal_term(float x, bool positive, float gamma, float alpha) {
    const float pr = sigmoidf_(x);
    if (positive) return -alpha * powf(1.f - pr, gamma) * logf(fmaxf(pr, 1.17549435e-38f));
    return -(1.f - alpha) * powf(pr, gamma) * logf(fmaxf(1.f - pr, 1.17549435e-38f));
}

__device__ __forceinline__ float focal_grad(float x, bool positive, float gamma, float alpha) {
    const float pr = sigmoidf_(x);
    if (positive) return -alpha * powf(1.f - pr, gamma) * (1.f - pr - gamma * pr * logf(fmaxf(pr, 1.17549435e-38f)));
    return -(1.f - alpha) * powf(pr, gamma) * (gamma * (1.f - pr) * logf(fmaxf(1.f - pr, 1.17549435e-38f)) - pr);
}

// _bbox_pred_to_bbox of the point and its six distances d, against the target box t: 1 - IoU of
// axis_aligned_bbox_overlaps_3d(is_aligned=True) (iou3d_calculator.py:281-323), and where gd != nullptr its gradient by d
__device__ __forceinline__ float iou_loss(float px, float py, float pz, const float* d, const float* t, float* gd) {
    const float a[6] = {px - d[0], py - d[2], pz - d[4], px + d[1], py + d[3], pz + d[5]};
    float e[3], wh[3], ga[6];
    bool lt_a[3], rb_a[3];
    for (int q = 0; q < 3; ++q) {
        e[q] = a[q + 3] - a[q];
        const float lt = fmaxf(a[q], t[q]), rb = fminf(a[q + 3], t[q + 3]);
        lt_a[q] = a[q] > t[q];
        rb_a[q] = a[q + 3] < t[q + 3];
        wh[q] = fmaxf(rb - lt, 0.f);
    }
    const float area1 = e[0] * e[1] * e[2];
    const float area2 = (t[3] - t[0]) * (t[4] - t[1]) * (t[5] - t[2]);
    const float ov = wh[0] * wh[1] * wh[2];
    const float un0 = area1 + area2 - ov;
    const float un = fmaxf(un0, 1e-6f);
    const float iou = ov / un;
    if (gd) {
        // d iou = d ov / un - ov / un^2 * d un, d un = d area1 - d ov where the union is above its floor
        const float k_ov = 1.f / un + (un0 > 1e-6f ? ov / (un * un) : 0.f);
        const float k_ar = un0 > 1e-6f ? -ov / (un * un) : 0.f;
        for (int q = 0; q < 3; ++q) {
            const float oth_e = e[(q + 1) % 3] * e[(q + 2) % 3];
            const float oth_w = wh[q] > 0.f ? wh[(q + 1) % 3] * wh[(q + 2) % 3] : 0.f;
            // lower corner a[q]: area1 falls with it; the overlap falls with it where it is the larger lower corner
            ga[q] = k_ar * -oth_e + (lt_a[q] ? k_ov * -oth_w : 0.f);
            ga[q + 3] = k_ar * oth_e + (rb_a[q] ? k_ov * oth_w : 0.f);
        }
        // loss = 1 - iou; a = (p - d0, p - d2, p - d4, p + d1, p + d3, p + d5)
        gd[0] = ga[0];
        gd[2] = ga[1];
        gd[4] = ga[2];
        gd[1] = -ga[3];
        gd[3] = -ga[4];
        gd[5] = -ga[5];
    }
    return 1.f - iou;
}

// binary_cross_entropy_with_logits(x, t): (1 - t) x + max(-x, 0) + log(exp(-max(-x, 0)) + exp(-x - max(-x, 0)))
__device__ __forceinline__ float bce_logits(float x, float t) {
    const float m = fmaxf(-x, 0.f);
    return (1.f - t) * x + m + logf(expf(-m) + expf(-x - m));
}

__global__ __launch_bounds__(kPointThreads) void head_loss_kernel(LossParams p, float* part_f, int* part_i) {
    __shared__ float fpart[kPointThreads / 64];
    __shared__ int ipart[kPointThreads / 64];
    const int b = blockIdx.y, i = blockIdx.x * kPointThreads + threadIdx.x;
    PointTerms s{0.f, 0.f, 0.f, 0.f, 0, 0};
    if (i < p.P) {
        const PointRef r = locate(p, b, i);
        const LossLevel& lm = p.lm[r.l];
        if (r.valid) {
            s.valid = 1;
            const float* cls = lm.cls + (size_t)b * p.C * r.N + r.v;
            for (int c = 0; c < p.C; ++c) s.cls += focal_term(cls[(size_t)c * r.N], r.label == c, p.gamma, p.alpha);
            if (r.label >= 0) {
                s.pos = 1;
                const size_t o = (size_t)b * p.P + i;
                const float ct = p.center_t[o];
                s.center = bce_logits(lm.center[(size_t)b * r.N + r.v], ct);
                float d[6];
                for (int q = 0; q < 6; ++q) d[q] = lm.bbox[((size_t)b * 6 + q) * r.N + r.v];
                s.w = ct;
                s.bbox = iou_loss(r.px, r.py, r.pz, d, p.bbox_t + o * 6, nullptr) * ct;
            }
        }
    }
    const float f0 = block_sum(s.center, fpart), f1 = block_sum(s.bbox, fpart), f2 = block_sum(s.cls, fpart), f3 = block_sum(s.w, fpart);
    const int i0 = block_sum(s.pos, ipart), i1 = block_sum(s.valid, ipart);
    if (threadIdx.x == 0) {
        const size_t o = (size_t)b * gridDim.x + blockIdx.x;
        part_f[o * 4 + 0] = f0;
        part_f[o * 4 + 1] = f1;
        part_f[o * 4 + 2] = f2;
        part_f[o * 4 + 3] = f3;
        part_i[o * 2 + 0] = i0;
        part_i[o * 2 + 1] = i1;
    }
}

// one workgroup of 64 threads per scene: lane q < 4 sums float column q, lanes 4 and 5 the counts, over the workgroups in order
__global__ void head_loss_finish_kernel(const float* part_f, const int* part_i, int nblk, float* out_sums, int* out_counts) {
    const int b = blockIdx.x, q = threadIdx.x;
    if (q < 4) {
        float s = 0.f;
        for (int k = 0; k < nblk; ++k) s += part_f[((size_t)b * nblk + k) * 4 + q];
        out_sums[b * 4 + q] = s;
    } else if (q < 6) {
        int s = 0;
        for (int k = 0; k < nblk; ++k) s += part_i[((size_t)b * nblk + k) * 2 + (q - 4)];
        out_counts[b * 2 + (q - 4)] = s;
    }
}

// coef (B, 3): what a unit of the scene's center / bbox / cls sum is worth (incoming gradient / normaliser), on the device
__global__ __launch_bounds__(kPointThreads) void head_loss_backward_kernel(LossParams p, const float* coef) {
    const int b = blockIdx.y, i = blockIdx.x * kPointThreads + threadIdx.x;
    if (i >= p.P) return;
    const PointRef r = locate(p, b, i);
    const LossLevel& lm = p.lm[r.l];
    const float k_center = coef[b * 3], k_bbox = coef[b * 3 + 1], k_cls = coef[b * 3 + 2];
    const float* cls = lm.cls + (size_t)b * p.C * r.N + r.v;
    float* d_cls = lm.d_cls + (size_t)b * p.C * r.N + r.v;
    for (int c = 0; c < p.C; ++c)
        d_cls[(size_t)c * r.N] = r.valid ? k_cls * focal_grad(cls[(size_t)c * r.N], r.label == c, p.gamma, p.alpha) : 0.f;
    float gc = 0.f, gd[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r.valid && r.label >= 0) {
        const size_t o = (size_t)b * p.P + i;
        const float ct = p.center_t[o];
        gc = k_center * (sigmoidf_(lm.center[(size_t)b * r.N + r.v]) - ct);
        float d[6];
        for (int q = 0; q < 6; ++q) d[q] = lm.bbox[((size_t)b * 6 + q) * r.N + r.v];
        iou_loss(r.px, r.py, r.pz, d, p.bbox_t + o * 6, gd);
        for (int q = 0; q < 6; ++q) gd[q] *= k_bbox * ct;
    }
    lm.d_center[(size_t)b * r.N + r.v] = gc;
    for (int q = 0; q < 6; ++q) lm.d_bbox[((size_t)b * 6 + q) * r.N + r.v] = gd[q];
}

int plan_levels(const char* name, const int* level_dims, int B, int L, GridLevel* lv, long long* points) {
    MVS_REQUIRE(level_dims, "%s: NULL pointer", name);
    MVS_REQUIRE(B >= 1 && B <= 65535, "%s: bad shape B=%d", name, B);
    MVS_REQUIRE(L >= 1 && L <= kMaxL, "%s: bad shape L=%d (1..%d levels)", name, L, kMaxL);
    *points = 0;
    for (int l = 0; l < L; ++l) {
        const int X = level_dims[3 * l], Y = level_dims[3 * l + 1], Z = level_dims[3 * l + 2];
        MVS_REQUIRE(X > 0 && Y > 0 && Z > 0 && (long long)X * Y * Z < (1 << 24), "%s: bad shape level %d: %dx%dx%d", name, l, X, Y, Z);
        lv[l] = GridLevel{X, Y, Z, (int)*points};
        *points += (long long)X * Y * Z;
    }
    MVS_REQUIRE((long long)B * *points * 6 < (1ll << 31), "%s: bad shape: %d scenes x %lld points", name, B, *points);
    return MVSDET_OK;
}

int plan_loss(const char* name, const float* const* center, const float* const* bbox, const float* const* cls, float* const* d_center,
              float* const* d_bbox, float* const* d_cls, bool backward, const int* level_dims, const float* valid,
              const float* level_geom, const int64_t* labels, const float* center_t, const float* bbox_t, int B, int L, int C, int VX,
              int VY, int VZ, float gamma, float alpha, LossParams* p) {
    MVS_REQUIRE(center && bbox && cls && valid && level_geom && labels && center_t && bbox_t, "%s: NULL pointer", name);
    MVS_REQUIRE(!backward || (d_center && d_bbox && d_cls), "%s: NULL pointer", name);
    *p = LossParams{};
    long long points;
    if (const int rc = plan_levels(name, level_dims, B, L, p->lv, &points)) return rc;
    MVS_REQUIRE(C >= 1 && C <= 1024, "%s: bad shape n_classes=%d (1..1024)", name, C);
    MVS_REQUIRE(VX > 0 && VY > 0 && VZ > 0 && (long long)VX * VY * VZ < (1 << 26), "%s: bad shape valid %dx%dx%d", name, VX, VY, VZ);
    MVS_REQUIRE(gamma >= 0.f && alpha >= 0.f && alpha <= 1.f, "%s: gamma=%g, alpha=%g", name, (double)gamma, (double)alpha);
    for (int l = 0; l < L; ++l) {
        MVS_REQUIRE(center[l] && bbox[l] && cls[l], "%s: NULL pointer (level %d)", name, l);
        MVS_REQUIRE(!backward || (d_center[l] && d_bbox[l] && d_cls[l]), "%s: NULL pointer (level %d)", name, l);
        LossLevel& m = p->lm[l];
        m.center = center[l];
        m.bbox = bbox[l];
        m.cls = cls[l];
        if (backward) {
            m.d_center = d_center[l];
            m.d_bbox = d_bbox[l];
            m.d_cls = d_cls[l];
        }
        m.sx = (float)VX / (float)p->lv[l].X;
        m.sy = (float)VY / (float)p->lv[l].Y;
        m.sz = (float)VZ / (float)p->lv[l].Z;
    }
    p->valid = valid;
    p->geom = level_geom;
    p->labels = reinterpret_cast<const long long*>(labels);
    p->center_t = center_t;
    p->bbox_t = bbox_t;
    p->L = L;
    p->C = C;
    p->P = (int)points;
    p->VX = VX;
    p->VY = VY;
    p->VZ = VZ;
    p->gamma = gamma;
    p->alpha = alpha;
    return MVSDET_OK;
}

int need_workspace(const char* name, const void* workspace, size_t bytes, size_t need, const char* query) {
    if (need == 0 || (workspace && bytes >= need)) return MVSDET_OK;
    set_error("%s: workspace of %zu bytes, %zu needed (%s)", name, bytes, need, query);
    return MVSDET_ERR_WORKSPACE;
}

inline int point_blocks(long long points) { return (int)((points + kPointThreads - 1) / kPointThreads); }

}  // namespace
}  // namespace mvsdet

using namespace mvsdet;

extern "C" size_t mvsdet_head_targets_workspace_bytes(int B, int G) {
    if (B <= 0 || G <= 0) return 0;
    return (size_t)B * G * (kMaxL + 2) * 4;
}

extern "C" int mvsdet_head_targets_f32(const int* level_dims, const float* level_geom, int B, int L, const float* gt_boxes,
                                       const float* gt_volumes, const int64_t* gt_labels, const int* gt_counts, int G,
                                       int pts_assign_threshold, int pts_center_threshold, int64_t* out_labels, int* out_box_index,
                                       float* out_center_targets, float* out_bbox_targets, void* workspace, size_t workspace_bytes,
                                       mvsdet_stream_t stream) {
    const char* name = "head_targets";
    AssignParams p{};
    long long points;
    if (const int rc = plan_levels(name, level_dims, B, L, p.lv, &points)) return rc;
    MVS_REQUIRE(level_geom && gt_counts && out_labels && out_box_index && out_center_targets && out_bbox_targets, "%s: NULL pointer", name);
    MVS_REQUIRE(G >= 0 && G <= kMaxBoxes, "%s: G=%d boxes per scene above the limit MVSDET_ASSIGN_MAX_BOXES=%d", name, G, kMaxBoxes);
    MVS_REQUIRE(G == 0 || (gt_boxes && gt_volumes && gt_labels), "%s: NULL pointer", name);
    MVS_REQUIRE(pts_assign_threshold >= 0 && pts_center_threshold >= 0, "%s: pts_assign_threshold=%d, pts_center_threshold=%d", name,
                pts_assign_threshold, pts_center_threshold);
    if (const int rc = need_workspace(name, workspace, workspace_bytes, mvsdet_head_targets_workspace_bytes(B, G),
                                      "mvsdet_head_targets_workspace_bytes"))
        return rc;
    p.geom = level_geom;
    p.boxes = gt_boxes;
    p.volumes = gt_volumes;
    p.labels = reinterpret_cast<const long long*>(gt_labels);
    p.counts = gt_counts;
    p.L = L;
    p.G = G;
    p.P = (int)points;
    p.assign_thr = pts_assign_threshold;
    p.center_thr = pts_center_threshold;
    p.n_inside = static_cast<int*>(workspace);
    p.best = p.n_inside + (size_t)B * G * kMaxL;
    p.thr = reinterpret_cast<float*>(p.best + (size_t)B * G);
    hipStream_t s = (hipStream_t)stream;
    if (G > 0) {
        hipLaunchKernelGGL(assign_count_kernel, dim3(G, L, B), dim3(kCountThreads), 0, s, p);
        hipLaunchKernelGGL(assign_select_kernel, dim3(G, B), dim3(kSelThreads), 0, s, p);
    }
    hipLaunchKernelGGL(assign_pick_kernel, dim3(point_blocks(points), B), dim3(kPointThreads), (size_t)std::max(G, 1) * sizeof(StagedBox),
                       s, p, reinterpret_cast<long long*>(out_labels), out_box_index, out_center_targets, out_bbox_targets);
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}

extern "C" size_t mvsdet_head_loss_workspace_bytes(int B, int points) {
    if (B <= 0 || points <= 0) return 0;
    return (size_t)B * point_blocks(points) * 6 * 4;
}

extern "C" int mvsdet_head_loss_f32(const float* const* center, const float* const* bbox, const float* const* cls, const int* level_dims,
                                    const float* valid, const float* level_geom, int B, int L, int n_classes, int VX, int VY, int VZ,
                                    const int64_t* labels, const float* center_targets, const float* bbox_targets, float gamma,
                                    float alpha, float* out_sums, int* out_counts, void* workspace, size_t workspace_bytes,
                                    mvsdet_stream_t stream) {
    const char* name = "head_loss";
    LossParams p;
    if (const int rc = plan_loss(name, center, bbox, cls, nullptr, nullptr, nullptr, false, level_dims, valid, level_geom, labels,
                                 center_targets, bbox_targets, B, L, n_classes, VX, VY, VZ, gamma, alpha, &p))
        return rc;
    MVS_REQUIRE(out_sums && out_counts, "%s: NULL pointer", name);
    if (const int rc = need_workspace(name, workspace, workspace_bytes, mvsdet_head_loss_workspace_bytes(B, p.P),
                                      "mvsdet_head_loss_workspace_bytes"))
        return rc;
    const int nblk = point_blocks(p.P);
    float* part_f = static_cast<float*>(workspace);
    int* part_i = reinterpret_cast<int*>(part_f + (size_t)B * nblk * 4);
    hipLaunchKernelGGL(head_loss_kernel, dim3(nblk, B), dim3(kPointThreads), 0, (hipStream_t)stream, p, part_f, part_i);
    hipLaunchKernelGGL(head_loss_finish_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, part_f, part_i, nblk, out_sums, out_counts);
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}

extern "C" int mvsdet_head_loss_backward_f32(const float* const* center, const float* const* bbox, const float* const* cls,
                                             const int* level_dims, const float* valid, const float* level_geom, int B, int L,
                                             int n_classes, int VX, int VY, int VZ, const int64_t* labels, const float* center_targets,
                                             const float* bbox_targets, float gamma, float alpha, const float* coef,
                                             float* const* d_center, float* const* d_bbox, float* const* d_cls, mvsdet_stream_t stream) {
    const char* name = "head_loss_backward";
    LossParams p;
    if (const int rc = plan_loss(name, center, bbox, cls, d_center, d_bbox, d_cls, true, level_dims, valid, level_geom, labels,
                                 center_targets, bbox_targets, B, L, n_classes, VX, VY, VZ, gamma, alpha, &p))
        return rc;
    MVS_REQUIRE(coef, "%s: NULL pointer", name);
    hipLaunchKernelGGL(head_loss_backward_kernel, dim3(point_blocks(p.P), B), dim3(kPointThreads), 0, (hipStream_t)stream, p, coef);
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}
