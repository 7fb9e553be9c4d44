// Training of the detection head on the caller's stream, no host round trip, no float atomics.  Two routes share every kernel
// (templates on the box record and on the box loss):
//   ScanNet head  NerfDetHead._get_targets (projects/NeRF-Det/nerfdet/nerfdet_head.py:473-562), _loss_by_feat_single (:206-257):
//                 6-value boxes, targets rebuilt from the face distances, AxisAlignedIoULoss
//   ARKit head    ImVoxelHead_ARKit._get_targets (:1107-1185), _loss_by_feat_single (:779-846): 7-value boxes with heading, face
//                 distances in the box's own frame (:1058-1084), the ground-truth box itself as target, RotatedIoU3DLoss
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
// op for op, under -ffp-contract=off with IEEE division and square root.  The rotated route takes cos(yaw) and sin(yaw) of every
// ground-truth box as inputs (torch.cos / torch.sin of the caller, as rotation_3d_in_axis computes them): no transcendental lies on
// the path to a label.  The sub-block of a rotated box is that of the axis-aligned hull of its footprint.
//
// RotatedIoU3DLoss (rotated_iou_loss below), one thread per positive point, forward and backward, no vertex list and no sort:
// the boundary of the intersection of two convex regions is the pieces of A's edges inside B plus the pieces of B's edges inside
// A.  Each of the eight edges is clipped by parameter interval (Liang-Barsky) against the other rectangle in that rectangle's own
// frame, where it is axis-aligned; the area is Green's sum 1/2 (c x t + h) * length over the pieces (c: the rectangle's centre
// seen from B's centre, t: the edge's direction, h: its distance from c).  The gradient is the boundary integral over the pieces
// of the predicted rectangle A: d area / d centre = sum of normal * length, / d size = half the lengths of the two edges across,
// / d yaw = - integral of tau d tau (tau: the position along the edge from its midpoint).  That is the derivative of the area
// itself, which is what autograd through mmcv's vertex gather yields away from degenerate pairs.
// Convention at degenerate pairs: a relative angle within 1e-6 rad of a multiple of pi/2 is taken as that multiple (float pi and
// pi/2 are not exact).  An edge of A that lies ON a parallel edge of B counts in full where both outward normals agree, and not
// at all where they oppose (boxes touching from outside); an edge of B that lies on an edge of A never counts (A against closed
// B, B against open A), so a shared edge is counted once.  With parallel axes the area is the product of the two overlaps along
// B's axes, taken from the same sums that place A's edges: two roundings of one shared edge cannot count it twice.  Left open: a
// relative angle between 1e-6 and about 1e-4 rad off a multiple of pi/2 together with two edges less than about 1e-7 m apart,
// where the crossing of the two nearly coincident edges is ill-conditioned in float32 and the area can be off by a share of that
// edge's strip (still finite; a set of vanishing measure that no test here reaches).  The area is clamped to >= 0, the union is never zero for
// a predicted box (its sizes are sums of two exponentials); a ground-truth box of zero size gives IoU 0.  All of it is finite.
//
// Ties of the axis-aligned IoU (iou_loss) and of the z faces of the rotated one follow ATen's autograd, which is what the reference
// trains with: torch.max / torch.min of two tensors give each operand half the gradient where the two are equal, and
// clamp(min=0) passes the gradient on where its argument is >= 0, at 0 itself too.  So a predicted corner (a z face) that equals
// the target's takes half the overlap's gradient, and boxes that touch (rb - lt == 0 on an axis, z ranges end to end) keep the
// overlap's gradient on that axis: identical boxes do not lose half their pull and touching boxes are still drawn together.  The
// forward values do not depend on any of this.  Left as it is: the exact tie un0 == 1e-6 of the axis-aligned union with its floor,
// where the floor's side is taken (no gradient through the union; ATen would halve it).  The BEV conventions above are unchanged.
#include "block_reduce.h"
#include "head_points.h"
#include "rect_clip.h"

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
    const float* boxes;    // (B, G, 6): gravity centre, size; rotated route (B, G, 7): and yaw
    const float* rot;      // rotated route: (B, G, 2) cos(yaw), sin(yaw)
    const float* volumes;  // (B, G)
    const long long* labels;   // (B, G)
    const int* counts;     // (B): boxes of the scene
    int L, G, P;
    int assign_thr, center_k;
    int* n_inside;         // (B, G, kMaxL) workspace
    int* best;             // (B, G)
    float* thr;            // (B, G)
};

struct LossLevel {
    const float* center;   // (B,1,X,Y,Z)
    const float* bbox;     // (B,6,X,Y,Z); rotated route (B,7,X,Y,Z)
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
    const float* bbox_t;       // (B, P, 6); rotated route (B, P, 7)
    int L, C, P, VX, VY, VZ;
    float gamma, alpha;
};

// The two box records.  kBox: values of a ground-truth row, kReg: channels of the bbox map and values of a target row
struct AlignedBox {
    static constexpr int kBox = 6, kReg = 6;
    float b[6];            // gravity centre, size
};
struct RotatedBox {
    static constexpr int kBox = 7, kReg = 7;
    float b[6];
    float yaw, c, s;       // heading, its cosine and sine as the caller computed them
};

__device__ __forceinline__ void load_box(const AssignParams& p, size_t r, AlignedBox& g) {
    for (int q = 0; q < 6; ++q) g.b[q] = p.boxes[r * 6 + q];
}
__device__ __forceinline__ void load_box(const AssignParams& p, size_t r, RotatedBox& g) {
    for (int q = 0; q < 6; ++q) g.b[q] = p.boxes[r * 7 + q];
    g.yaw = p.boxes[r * 7 + 6];
    g.c = p.rot[r * 2];
    g.s = p.rot[r * 2 + 1];
}

// _get_face_distances of point (px, py, pz) to box b = (cx, cy, cz, dx, dy, dz), in the reference's operand order
__device__ __forceinline__ void face_distances(float px, float py, float pz, const float* b, float* d) {
    d[0] = (px - b[0]) + b[3] / 2.f;
    d[1] = (b[0] + b[3] / 2.f) - px;
    d[2] = (py - b[1]) + b[4] / 2.f;
    d[3] = (b[1] + b[4] / 2.f) - py;
    d[4] = (pz - b[2]) + b[5] / 2.f;
    d[5] = (b[2] + b[5] / 2.f) - pz;
}
__device__ __forceinline__ void face_distances(float px, float py, float pz, const AlignedBox& g, float* d) {
    face_distances(px, py, pz, g.b, d);
}
// ImVoxelHead_ARKit._get_face_distances (:1070-1084): point - centre rotated by -yaw about z (rotation_3d_in_axis: the row
// vector times [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]] of the angle -yaw), added to the centre again, then the six distances
__device__ __forceinline__ void face_distances(float px, float py, float pz, const RotatedBox& g, float* d) {
    const float sx = px - g.b[0], sy = py - g.b[1], sz = pz - g.b[2];
    const float rs = -g.s;                                   // sin(-yaw)
    const float cx = g.b[0] + (sx * g.c + sy * -rs);
    const float cy = g.b[1] + (sx * rs + sy * g.c);
    const float cz = g.b[2] + sz;
    face_distances(cx, cy, cz, g.b, d);
}

// the extents along x and y of what bounds the box's footprint: its sizes, or the axis-aligned hull of the rotated rectangle
__device__ __forceinline__ void footprint(const AlignedBox& g, float& ex, float& ey) { ex = g.b[3], ey = g.b[4]; }
__device__ __forceinline__ void footprint(const RotatedBox& g, float& ex, float& ey) {
    ex = fabsf(g.c) * g.b[3] + fabsf(g.s) * g.b[4];
    ey = fabsf(g.s) * g.b[3] + fabsf(g.c) * g.b[4];
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

template <class Box>
__device__ __forceinline__ SubBlock box_sub_block(const Box& box, const float* g, const GridLevel& lv) {
    SubBlock s;
    int e;
    float ex, ey;
    footprint(box, ex, ey);
    const float* b = box.b;
    axis_range(b[0], ex, g[0], g[3], lv.X, s.x0, e);
    s.nx = e - s.x0;
    axis_range(b[1], ey, g[1], g[4], lv.Y, s.y0, e);
    s.ny = e - s.y0;
    axis_range(b[2], b[5], g[2], g[5], lv.Z, s.z0, e);
    s.nz = e - s.z0;
    return s;
}

template <class Box>
__global__ __launch_bounds__(kCountThreads) void assign_count_kernel(AssignParams p) {
    const int g = blockIdx.x, l = blockIdx.y, b = blockIdx.z;
    if (g >= p.counts[b]) return;
    const GridLevel lv = p.lv[l];
    const float* gp = p.geom + ((size_t)b * p.L + l) * 6;
    const float geo[6] = {gp[0], gp[1], gp[2], gp[3], gp[4], gp[5]};
    Box box;
    load_box(p, (size_t)b * p.G + g, box);
    const SubBlock sb = box_sub_block(box, geo, lv);
    int n[1] = {0};
    for (int j = threadIdx.x; j < sb.size(); j += kCountThreads) {
        int x, y, z;
        float px, py, pz, d[6];
        sb.at(j, x, y, z);
        grid_point(geo, x, y, z, px, py, pz);
        face_distances(px, py, pz, box, d);
        n[0] += inside_box(d) ? 1 : 0;
    }
    if (block_sums<kCountThreads>(n)) p.n_inside[((size_t)b * p.G + g) * kMaxL + l] = n[0];
}

template <class Box>
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
    Box box;
    load_box(p, (size_t)b * p.G + g, box);
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
    const int k = p.center_k;   // pts_center_threshold + 1; the ARKit head: at most all points (:1167-1170)
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

template <class Box>
struct StagedBox {
    Box box;
    float volume, thr;
    int best;
};

// the targets of a point at its chosen box: the ScanNet head rebuilds the box from the face distances (:556-561), the ARKit head
// hands out the ground-truth row itself (:1180)
__device__ __forceinline__ void box_target(const AlignedBox&, float px, float py, float pz, const float* d, float* bt) {
    bt[0] = px - d[0];
    bt[1] = py - d[2];
    bt[2] = pz - d[4];
    bt[3] = px + d[1];
    bt[4] = py + d[3];
    bt[5] = pz + d[5];
}
__device__ __forceinline__ void box_target(const RotatedBox& g, float, float, float, const float*, float* bt) {
    for (int q = 0; q < 6; ++q) bt[q] = g.b[q];
    bt[6] = g.yaw;
}

// none_center: the centerness target of a point without a box (0 for the ScanNet head, the masked -1 for the ARKit head)
template <class Box>
__global__ __launch_bounds__(kPointThreads) void assign_pick_kernel(AssignParams p, float none_center, long long* out_labels,
                                                                    int* out_box, float* out_center, float* out_bbox) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    StagedBox<Box>* sb = reinterpret_cast<StagedBox<Box>*>(smem);
    const int b = blockIdx.y;
    const int G = min(p.counts[b], p.G);
    for (int g = threadIdx.x; g < G; g += kPointThreads) {
        const size_t r = (size_t)b * p.G + g;
        load_box(p, r, sb[g].box);
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
        face_distances(px, py, pz, sb[g].box, d);
        if (!inside_box(d)) continue;
        if (!(centerness(d) > sb[g].thr)) continue;
        if (sb[g].volume < vmin) {
            vmin = sb[g].volume;
            arg = g;
        }
    }
    const size_t o = (size_t)b * p.P + i;
    float ct = none_center, bt[Box::kReg];
    for (int q = 0; q < Box::kReg; ++q) bt[q] = 0.f;
    long long label = -1;
    if (arg >= 0) {
        float d[6];
        face_distances(px, py, pz, sb[arg].box, d);
        ct = centerness(d);
        box_target(sb[arg].box, px, py, pz, d, bt);
        label = p.labels[(size_t)b * p.G + arg];
    }
    out_labels[o] = label;
    out_box[o] = arg;
    out_center[o] = ct;
    for (int q = 0; q < Box::kReg; ++q) out_bbox[o * Box::kReg + q] = bt[q];
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

// the floor under the focal loss' logarithms as torch's clamp(min=FLT_MIN) sets it: a NaN stays a NaN (fmaxf would drop it, and with
// gamma = 0, where pow(NaN, 0) = 1, a NaN logit would come out as a finite term)
__device__ __forceinline__ float log_floor(float v) { return v < 1.17549435e-38f ? 1.17549435e-38f : v; }

// mmcv's sigmoid focal loss of one (point, class) logit: the positive term where the point's label is the class, else the
// negative one (a label of -1 is background in every class)
__device__ __forceinline__ float focal_term(float x, bool positive, float gamma, float alpha) {
    const float pr = sigmoidf_(x);
    if (positive) return -alpha * powf(1.f - pr, gamma) * logf(log_floor(pr));
    return -(1.f - alpha) * powf(pr, gamma) * logf(log_floor(1.f - pr));
}

__device__ __forceinline__ float focal_grad(float x, bool positive, float gamma, float alpha) {
    const float pr = sigmoidf_(x);
    if (positive) return -alpha * powf(1.f - pr, gamma) * (1.f - pr - gamma * pr * logf(log_floor(pr)));
    return -(1.f - alpha) * powf(pr, gamma) * (gamma * (1.f - pr) * logf(log_floor(1.f - pr)) - pr);
}

// the first operand's share of the gradient of torch.max / torch.min of two tensors: all of it where it is the chosen one, half at
// an exact tie, none otherwise (file header: ties)
__device__ __forceinline__ float tie_share(bool chosen, bool tie) { return chosen ? 1.f : tie ? 0.5f : 0.f; }

// _bbox_pred_to_bbox of the point and its six distances d, against the target box t: 1 - IoU of
// axis_aligned_bbox_overlaps_3d(is_aligned=True) (iou3d_calculator.py:281-323), and where gd != nullptr its gradient by d.
// Ties and touches as ATen's autograd routes them (file header); the forward value does not depend on them.
__device__ __forceinline__ float iou_loss(float px, float py, float pz, const float* d, const float* t, float* gd) {
    const float a[6] = {px - d[0], py - d[2], pz - d[4], px + d[1], py + d[3], pz + d[5]};
    float e[3], wh[3], ga[6];
    float lt_a[3], rb_a[3];   // the predicted corner's share of d max / d min: all, half at an exact tie (ATen), none
    bool open[3];             // clamp(min=0) passes the gradient on where its argument is >= 0, at 0 itself too (ATen)
    for (int q = 0; q < 3; ++q) {
        e[q] = a[q + 3] - a[q];
        const float lt = fmaxf(a[q], t[q]), rb = fminf(a[q + 3], t[q + 3]);
        lt_a[q] = tie_share(a[q] > t[q], a[q] == t[q]);
        rb_a[q] = tie_share(a[q + 3] < t[q + 3], a[q + 3] == t[q + 3]);
        open[q] = rb - lt >= 0.f;
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
            const float oth_w = open[q] ? wh[(q + 1) % 3] * wh[(q + 2) % 3] : 0.f;
            // lower corner a[q]: area1 falls with it; the overlap falls with it where it is the larger lower corner
            ga[q] = k_ar * -oth_e + lt_a[q] * (k_ov * -oth_w);
            ga[q + 3] = k_ar * oth_e + rb_a[q] * (k_ov * oth_w);
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

__device__ __forceinline__ float box_loss(const AlignedBox&, float px, float py, float pz, const float* d, const float* t, float* gd) {
    return iou_loss(px, py, pz, d, t, gd);
}

// RotatedIoU3DLoss of one point: ImVoxelHead_ARKit._bbox_pred_to_bbox (:1045-1055) of the point and its seven channels d (six
// distances, heading) against the target box t = (centre, size, yaw); 1 - IoU3D, IoU3D = A_bev * z overlap / (V_pred + V_gt -
// A_bev * z overlap) as mmcv's diff_iou_rotated_3d composes it, and where gd != nullptr its gradient by d.  File header: method
// and the convention at degenerate pairs.
__device__ __forceinline__ float rotated_iou_loss(float px, float py, float pz, const float* d, const float* t, float* gd) {
    const float ca = cosf(d[6]), sa = sinf(d[6]);
    const float sx = (d[1] - d[0]) / 2.f, sy = (d[3] - d[2]) / 2.f, sz = (d[5] - d[4]) / 2.f;
    const float ax = px + (sx * ca - sy * sa), ay = py + (sx * sa + sy * ca), az = pz + sz;
    const float aw = d[0] + d[1], al = d[2] + d[3], ah = d[4] + d[5];
    const float hw = aw / 2.f, hl = al / 2.f, ow = t[3] / 2.f, ol = t[4] / 2.f;
    // A in B's frame: centre r, axes turned by theta = yaw_a - yaw_b (snapped at multiples of pi / 2)
    const float cb = cosf(t[6]), sb = sinf(t[6]);
    const float ex = ax - t[0], ey = ay - t[1];
    const float rx = ex * cb + ey * sb, ry = ey * cb - ex * sb;
    const float theta = d[6] - t[6];
    float c = cosf(theta), s = sinf(theta);
    if (fabsf(s) < 1e-6f) {
        s = 0.f;
        c = c < 0.f ? -1.f : 1.f;
    } else if (fabsf(c) < 1e-6f) {
        c = 0.f;
        s = s < 0.f ? -1.f : 1.f;
    }
    // B in A's frame
    const float qx = -(rx * c + ry * s), qy = -(ry * c - rx * s);
    float t0, t1, tx, ty, twice = 0.f, len[4], gyaw = 0.f;
    // A's edges against B: Green's term (r x t + h) * length, and what the gradient needs
    clip_edge<0>(rx, ry, c, s, hw, hl, ow, ol, true, t0, t1, tx, ty);
    len[0] = t1 - t0, twice += (rx * ty - ry * tx + hw) * len[0], gyaw -= (t1 * t1 - t0 * t0) / 2.f;
    clip_edge<1>(rx, ry, c, s, hw, hl, ow, ol, true, t0, t1, tx, ty);
    len[1] = t1 - t0, twice += (rx * ty - ry * tx + hl) * len[1], gyaw -= (t1 * t1 - t0 * t0) / 2.f;
    clip_edge<2>(rx, ry, c, s, hw, hl, ow, ol, true, t0, t1, tx, ty);
    len[2] = t1 - t0, twice += (rx * ty - ry * tx + hw) * len[2], gyaw -= (t1 * t1 - t0 * t0) / 2.f;
    clip_edge<3>(rx, ry, c, s, hw, hl, ow, ol, true, t0, t1, tx, ty);
    len[3] = t1 - t0, twice += (rx * ty - ry * tx + hl) * len[3], gyaw -= (t1 * t1 - t0 * t0) / 2.f;
    if (s == 0.f || c == 0.f) {
        // parallel axes: the product of the two overlaps along B's axes, from the very sums A's edges were placed with above, so
        // that an edge the two rectangles share (to the last bit or not) is never counted for both
        const float hx = s == 0.f ? hw : hl, hy = s == 0.f ? hl : hw;
        const float ox = fminf(rx + hx, ow) - fmaxf(rx - hx, -ow), oy = fminf(ry + hy, ol) - fmaxf(ry - hy, -ol);
        twice = 2.f * fmaxf(ox, 0.f) * fmaxf(oy, 0.f);
    } else {
        // B's edges against A (B's centre is the origin of Green's sum: h * length)
        clip_edge<0>(qx, qy, c, -s, ow, ol, hw, hl, false, t0, t1, tx, ty);
        twice += ow * (t1 - t0);
        clip_edge<1>(qx, qy, c, -s, ow, ol, hw, hl, false, t0, t1, tx, ty);
        twice += ol * (t1 - t0);
        clip_edge<2>(qx, qy, c, -s, ow, ol, hw, hl, false, t0, t1, tx, ty);
        twice += ow * (t1 - t0);
        clip_edge<3>(qx, qy, c, -s, ow, ol, hw, hl, false, t0, t1, tx, ty);
        twice += ol * (t1 - t0);
    }
    const float area0 = twice / 2.f;
    const float area = fmaxf(area0, 0.f);
    const float zhi_a = az + ah * 0.5f, zlo_a = az - ah * 0.5f, zhi_b = t[2] + t[5] * 0.5f, zlo_b = t[2] - t[5] * 0.5f;
    const float zo0 = fminf(zhi_a, zhi_b) - fmaxf(zlo_a, zlo_b);
    const float zo = fmaxf(zo0, 0.f);
    const float inter = area * zo;
    const float vol_a = aw * al * ah, vol_b = t[3] * t[4] * t[5];
    const float uni = vol_a + vol_b - inter;
    const bool ok = uni > 0.f;
    const float iou = ok ? inter / uni : 0.f;
    if (gd) {
        // d iou = k_i d inter + k_v d vol_a; d inter = zo d area + area d zo
        const float k_i = ok ? (uni + inter) / (uni * uni) : 0.f, k_v = ok ? -inter / (uni * uni) : 0.f;
        const float k_a = area0 > 0.f ? k_i * zo : 0.f, k_z = zo0 >= 0.f ? k_i * area : 0.f;
        // by the shift (A's own axes), the sizes and the heading; the centre turns with the heading about the point
        const float gxl = len[0] - len[2], gyl = len[1] - len[3];
        const float g_sx = k_a * gxl, g_sy = k_a * gyl;
        const float g_zhi = tie_share(zhi_a < zhi_b, zhi_a == zhi_b) * k_z, g_zlo = tie_share(zlo_a > zlo_b, zlo_a == zlo_b) * -k_z;
        const float g_sz = g_zhi + g_zlo;
        const float g_w = k_a * (len[0] + len[2]) / 2.f + k_v * al * ah;
        const float g_l = k_a * (len[1] + len[3]) / 2.f + k_v * aw * ah;
        const float g_h = (g_zhi - g_zlo) * 0.5f + k_v * aw * al;
        // loss = 1 - iou
        gd[0] = -(g_w - g_sx / 2.f);
        gd[1] = -(g_w + g_sx / 2.f);
        gd[2] = -(g_l - g_sy / 2.f);
        gd[3] = -(g_l + g_sy / 2.f);
        gd[4] = -(g_h - g_sz / 2.f);
        gd[5] = -(g_h + g_sz / 2.f);
        gd[6] = -(k_a * (gyaw + gyl * sx - gxl * sy));
    }
    return 1.f - iou;
}
__device__ __forceinline__ float box_loss(const RotatedBox&, float px, float py, float pz, const float* d, const float* t, float* gd) {
    return rotated_iou_loss(px, py, pz, d, t, gd);
}

// binary_cross_entropy_with_logits(x, t) as ATen evaluates it: (1 - t) x - log_sigmoid(x), log_sigmoid(x) = min(x, 0) -
// log1p(exp(-|x|)).  The log1p keeps the term of a confident logit (log(1 + exp(-30)) = 9.4e-14), which log(1 + ...) rounds to 0
__device__ __forceinline__ float bce_logits(float x, float t) {
    return (1.f - t) * x - (fminf(x, 0.f) - log1pf(expf(-fabsf(x))));
}

template <class Box>
__global__ __launch_bounds__(kPointThreads) void head_loss_kernel(LossParams p, float* part_f, int* part_i) {
    constexpr int R = Box::kReg;
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
                float d[R];
                for (int q = 0; q < R; ++q) d[q] = lm.bbox[((size_t)b * R + q) * r.N + r.v];
                s.w = ct;
                s.bbox = box_loss(Box{}, r.px, r.py, r.pz, d, p.bbox_t + o * R, nullptr) * ct;
            }
        }
    }
    float f[4] = {s.center, s.bbox, s.cls, s.w};
    int n[2] = {s.pos, s.valid};
    if (block_sums<kPointThreads>(f, n)) {   // block_reduce.h; the sign of a -0.f total ends at head_loss_finish_kernel's 0.f seed
        const size_t o = (size_t)b * gridDim.x + blockIdx.x;
        for (int q = 0; q < 4; ++q) part_f[o * 4 + q] = f[q];
        for (int q = 0; q < 2; ++q) part_i[o * 2 + q] = n[q];
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
template <class Box>
__global__ __launch_bounds__(kPointThreads) void head_loss_backward_kernel(LossParams p, const float* coef) {
    constexpr int R = Box::kReg;
    const int b = blockIdx.y, i = blockIdx.x * kPointThreads + threadIdx.x;
    if (i >= p.P) return;
    const PointRef r = locate(p, b, i);
    const LossLevel& lm = p.lm[r.l];
    const float k_center = coef[b * 3], k_bbox = coef[b * 3 + 1], k_cls = coef[b * 3 + 2];
    const float* cls = lm.cls + (size_t)b * p.C * r.N + r.v;
    float* d_cls = lm.d_cls + (size_t)b * p.C * r.N + r.v;
    for (int c = 0; c < p.C; ++c)
        d_cls[(size_t)c * r.N] = r.valid ? k_cls * focal_grad(cls[(size_t)c * r.N], r.label == c, p.gamma, p.alpha) : 0.f;
    float gc = 0.f, gd[R];
    for (int q = 0; q < R; ++q) gd[q] = 0.f;
    if (r.valid && r.label >= 0) {
        const size_t o = (size_t)b * p.P + i;
        const float ct = p.center_t[o];
        gc = k_center * (sigmoidf_(lm.center[(size_t)b * r.N + r.v]) - ct);
        float d[R];
        for (int q = 0; q < R; ++q) d[q] = lm.bbox[((size_t)b * R + q) * r.N + r.v];
        box_loss(Box{}, r.px, r.py, r.pz, d, p.bbox_t + o * R, gd);
        for (int q = 0; q < R; ++q) gd[q] *= k_bbox * ct;
    }
    lm.d_center[(size_t)b * r.N + r.v] = gc;
    for (int q = 0; q < R; ++q) lm.d_bbox[((size_t)b * R + q) * r.N + r.v] = gd[q];
}

int plan_levels(const char* name, const int* level_dims, int B, int L, int nreg, GridLevel* lv, long long* points) {
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
    MVS_REQUIRE((long long)B * *points * nreg < (1ll << 31), "%s: bad shape: %d scenes x %lld points", name, B, *points);
    return MVSDET_OK;
}

int plan_loss(const char* name, const float* const* center, const float* const* bbox, const float* const* cls, float* const* d_center,
              float* const* d_bbox, float* const* d_cls, bool backward, const int* level_dims, const float* valid,
              const float* level_geom, const int64_t* labels, const float* center_t, const float* bbox_t, int B, int L, int C, int VX,
              int VY, int VZ, float gamma, float alpha, int nreg, LossParams* p) {
    MVS_REQUIRE(center && bbox && cls && valid && level_geom && labels && center_t && bbox_t, "%s: NULL pointer", name);
    MVS_REQUIRE(!backward || (d_center && d_bbox && d_cls), "%s: NULL pointer", name);
    *p = LossParams{};
    long long points;
    if (const int rc = plan_levels(name, level_dims, B, L, nreg, p->lv, &points)) return rc;
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

// the three launches of the target assignment; rot == nullptr: the ScanNet route
template <class Box>
int launch_targets(const char* name, const int* level_dims, const float* level_geom, int B, int L, const float* gt_boxes,
                   const float* gt_rot, const float* gt_volumes, const int64_t* gt_labels, const int* gt_counts, int G,
                   int pts_assign_threshold, int pts_center_threshold, float none_center, int64_t* out_labels, int* out_box_index,
                   float* out_center_targets, float* out_bbox_targets, void* workspace, size_t workspace_bytes, size_t need,
                   mvsdet_stream_t stream) {
    constexpr bool rotated = Box::kBox == 7;
    AssignParams p{};
    long long points;
    if (const int rc = plan_levels(name, level_dims, B, L, Box::kReg, p.lv, &points)) return rc;
    MVS_REQUIRE(level_geom && gt_counts && out_labels && out_box_index && out_center_targets && out_bbox_targets, "%s: NULL pointer", name);
    MVS_REQUIRE(G >= 0 && G <= kMaxBoxes, "%s: G=%d boxes per scene above the limit MVSDET_ASSIGN_MAX_BOXES=%d", name, G, kMaxBoxes);
    MVS_REQUIRE(G == 0 || (gt_boxes && gt_volumes && gt_labels && (gt_rot || !rotated)), "%s: NULL pointer", name);
    MVS_REQUIRE(pts_assign_threshold >= 0 && pts_center_threshold >= 0, "%s: pts_assign_threshold=%d, pts_center_threshold=%d", name,
                pts_assign_threshold, pts_center_threshold);
    if (const int rc = need_workspace(name, workspace, workspace_bytes, need, "mvsdet_head_targets_workspace_bytes")) return rc;
    p.geom = level_geom;
    p.boxes = gt_boxes;
    p.rot = gt_rot;
    p.volumes = gt_volumes;
    p.labels = reinterpret_cast<const long long*>(gt_labels);
    p.counts = gt_counts;
    p.L = L;
    p.G = G;
    p.P = (int)points;
    p.assign_thr = pts_assign_threshold;
    // torch.topk(centerness, pts_center_threshold + 1); the ARKit head: min(pts_center_threshold + 1, points) (:1167-1170)
    p.center_k = rotated ? (int)std::min<long long>((long long)pts_center_threshold + 1, points) : pts_center_threshold + 1;
    p.n_inside = static_cast<int*>(workspace);
    p.best = p.n_inside + (size_t)B * G * kMaxL;
    p.thr = reinterpret_cast<float*>(p.best + (size_t)B * G);
    hipStream_t s = (hipStream_t)stream;
    if (G > 0) {
        hipLaunchKernelGGL(assign_count_kernel<Box>, dim3(G, L, B), dim3(kCountThreads), 0, s, p);
        hipLaunchKernelGGL(assign_select_kernel<Box>, dim3(G, B), dim3(kSelThreads), 0, s, p);
    }
    hipLaunchKernelGGL(assign_pick_kernel<Box>, dim3(point_blocks(points), B), dim3(kPointThreads),
                       (size_t)std::max(G, 1) * sizeof(StagedBox<Box>), s, p, none_center, reinterpret_cast<long long*>(out_labels),
                       out_box_index, out_center_targets, out_bbox_targets);
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}

template <class Box>
int launch_loss(const char* name, const float* const* center, const float* const* bbox, const float* const* cls, const int* level_dims,
                const float* valid, const float* level_geom, int B, int L, int n_classes, int VX, int VY, int VZ, const int64_t* labels,
                const float* center_targets, const float* bbox_targets, float gamma, float alpha, float* out_sums, int* out_counts,
                void* workspace, size_t workspace_bytes, mvsdet_stream_t stream) {
    LossParams p;
    if (const int rc = plan_loss(name, center, bbox, cls, nullptr, nullptr, nullptr, false, level_dims, valid, level_geom, labels,
                                 center_targets, bbox_targets, B, L, n_classes, VX, VY, VZ, gamma, alpha, Box::kReg, &p))
        return rc;
    MVS_REQUIRE(out_sums && out_counts, "%s: NULL pointer", name);
    const int nblk = point_blocks(p.P);
    if (const int rc = need_workspace(name, workspace, workspace_bytes, (size_t)B * nblk * 6 * 4, "mvsdet_head_loss_workspace_bytes"))
        return rc;
    float* part_f = static_cast<float*>(workspace);
    int* part_i = reinterpret_cast<int*>(part_f + (size_t)B * nblk * 4);
    hipLaunchKernelGGL(head_loss_kernel<Box>, dim3(nblk, B), dim3(kPointThreads), 0, (hipStream_t)stream, p, part_f, part_i);
    hipLaunchKernelGGL(head_loss_finish_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, part_f, part_i, nblk, out_sums, out_counts);
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}

template <class Box>
int launch_loss_backward(const char* name, const float* const* center, const float* const* bbox, const float* const* cls,
                         const int* level_dims, const float* valid, const float* level_geom, int B, int L, int n_classes, int VX, int VY,
                         int VZ, const int64_t* labels, const float* center_targets, const float* bbox_targets, float gamma, float alpha,
                         const float* coef, float* const* d_center, float* const* d_bbox, float* const* d_cls, mvsdet_stream_t stream) {
    LossParams p;
    if (const int rc = plan_loss(name, center, bbox, cls, d_center, d_bbox, d_cls, true, level_dims, valid, level_geom, labels,
                                 center_targets, bbox_targets, B, L, n_classes, VX, VY, VZ, gamma, alpha, Box::kReg, &p))
        return rc;
    MVS_REQUIRE(coef, "%s: NULL pointer", name);
    hipLaunchKernelGGL(head_loss_backward_kernel<Box>, dim3(point_blocks(p.P), B), dim3(kPointThreads), 0, (hipStream_t)stream, p, coef);
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}

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
    return launch_targets<AlignedBox>("head_targets", level_dims, level_geom, B, L, gt_boxes, nullptr, gt_volumes, gt_labels, gt_counts, G,
                                      pts_assign_threshold, pts_center_threshold, 0.f, out_labels, out_box_index, out_center_targets,
                                      out_bbox_targets, workspace, workspace_bytes, mvsdet_head_targets_workspace_bytes(B, G), stream);
}

extern "C" int mvsdet_head_targets_rotated_f32(const int* level_dims, const float* level_geom, int B, int L, const float* gt_boxes,
                                               const float* gt_rot, const float* gt_volumes, const int64_t* gt_labels,
                                               const int* gt_counts, int G, int pts_assign_threshold, int pts_center_threshold,
                                               int64_t* out_labels, int* out_box_index, float* out_center_targets,
                                               float* out_bbox_targets, void* workspace, size_t workspace_bytes, mvsdet_stream_t stream) {
    return launch_targets<RotatedBox>("head_targets_rotated", level_dims, level_geom, B, L, gt_boxes, gt_rot, gt_volumes, gt_labels,
                                      gt_counts, G, pts_assign_threshold, pts_center_threshold, -1.f, out_labels, out_box_index,
                                      out_center_targets, out_bbox_targets, workspace, workspace_bytes,
                                      mvsdet_head_targets_workspace_bytes(B, G), stream);
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
    return launch_loss<AlignedBox>("head_loss", center, bbox, cls, level_dims, valid, level_geom, B, L, n_classes, VX, VY, VZ, labels,
                                   center_targets, bbox_targets, gamma, alpha, out_sums, out_counts, workspace, workspace_bytes, stream);
}

extern "C" int mvsdet_head_loss_rotated_f32(const float* const* center, const float* const* bbox, const float* const* cls,
                                            const int* level_dims, const float* valid, const float* level_geom, int B, int L,
                                            int n_classes, int VX, int VY, int VZ, const int64_t* labels, const float* center_targets,
                                            const float* bbox_targets, float gamma, float alpha, float* out_sums, int* out_counts,
                                            void* workspace, size_t workspace_bytes, mvsdet_stream_t stream) {
    return launch_loss<RotatedBox>("head_loss_rotated", center, bbox, cls, level_dims, valid, level_geom, B, L, n_classes, VX, VY, VZ,
                                   labels, center_targets, bbox_targets, gamma, alpha, out_sums, out_counts, workspace, workspace_bytes,
                                   stream);
}

extern "C" int mvsdet_head_loss_backward_f32(const float* const* center, const float* const* bbox, const float* const* cls,
                                             const int* level_dims, const float* valid, const float* level_geom, int B, int L,
                                             int n_classes, int VX, int VY, int VZ, const int64_t* labels, const float* center_targets,
                                             const float* bbox_targets, float gamma, float alpha, const float* coef,
                                             float* const* d_center, float* const* d_bbox, float* const* d_cls, mvsdet_stream_t stream) {
    return launch_loss_backward<AlignedBox>("head_loss_backward", center, bbox, cls, level_dims, valid, level_geom, B, L, n_classes, VX,
                                            VY, VZ, labels, center_targets, bbox_targets, gamma, alpha, coef, d_center, d_bbox, d_cls,
                                            stream);
}

extern "C" int mvsdet_head_loss_rotated_backward_f32(const float* const* center, const float* const* bbox, const float* const* cls,
                                                     const int* level_dims, const float* valid, const float* level_geom, int B, int L,
                                                     int n_classes, int VX, int VY, int VZ, const int64_t* labels,
                                                     const float* center_targets, const float* bbox_targets, float gamma, float alpha,
                                                     const float* coef, float* const* d_center, float* const* d_bbox,
                                                     float* const* d_cls, mvsdet_stream_t stream) {
    return launch_loss_backward<RotatedBox>("head_loss_rotated_backward", center, bbox, cls, level_dims, valid, level_geom, B, L,
                                            n_classes, VX, VY, VZ, labels, center_targets, bbox_targets, gamma, alpha, coef, d_center,
                                            d_bbox, d_cls, stream);
}
