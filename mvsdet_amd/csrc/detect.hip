// Detection post-processing of the two heads: head maps -> kept boxes on the caller's stream, no host round trip.
//
// The stages, each written once:
//   detect_select_kernel<kRot>  one workgroup per (level, scene): upsampled valid mask, score = sigmoid(cls) * sigmoid(center) * valid,
//                               max over classes, top-nms_pre by a radix select on the score bits, decode into the candidate list
//   sort_keys                   one workgroup per list: bitonic sort in LDS of (score descending, NaN first, index ascending) keys
//   mask_tile                   64 rows x 64 columns: the suppression bit of every ordered pair (i, j > i), one 64-bit word per row
//   greedy_walk                 one workgroup per list: the walk 64 boxes at a time, kept rows handed to the route in pick order
//
// The ScanNet head (NerfDetHead.predict_by_feat -> _predict_by_feat_single -> _nms -> aligned_3d_nms,
// projects/NeRF-Det/nerfdet/nerfdet_head.py:301-420, 564-628; mvsdet_detect_head_f32), four launches: detect_select_kernel<false>
// keeps score > score_thr and appends the 6-DoF boxes in voxel order to the level's segment of the scene's list.
// detect_sort_kernel sorts one list per scene over the levels' segments.  detect_mask_kernel runs the class-aware axis-aligned IoU
// (NaN suppresses) on a (words, words, B) grid.  detect_scan_kernel writes the kept boxes converted, in pick order, then the padding.
//
// The ARKit head (ImVoxelHead_ARKit.predict_by_feat -> _single_scene_multiclass_nms -> mmcv's nms3d, nerfdet_head.py:902-1056,
// 1190-1243; mvsdet_detect_head_rotated_f32), a memset and five launches: detect_select_kernel<true> decodes every top-k point into
// a 7-DoF box and appends each of its classes above score_thr to the (scene, class) segment.  rot_sort_kernel sorts one list per
// segment and computes the IoU prepass of every box.  rot_mask_kernel runs mmcv's rotated BEV IoU (NaN does not suppress), its
// workgroups striding over a segment's tiles.  rot_scan_kernel records the kept rows; rot_gather_kernel writes them class-major.
//
// The standalone NMS replaces the first launch by a copy of the caller's boxes: mvsdet_aligned_3d_nms_f32 by detect_load_kernel,
// mvsdet_nms3d_f32 by rot_load_kernel.
//
// All arithmetic that decides or produces an output is written as the reference's ATen expression, op for op; the Makefile's
// -ffp-contract=off keeps every product and sum separately rounded, and fp32 division is IEEE-rounded (hipcc's default).
#include "common.h"
#include "head_points.h"

#include <algorithm>
#include <type_traits>

namespace mvsdet {
namespace {

constexpr int kSelThreads = 1024;
constexpr int kSortThreads = 1024;
constexpr int kScanThreads = 1024;
constexpr int kMaxL = MVSDET_DETECT_MAX_LEVELS;
constexpr int kLimit = MVSDET_DETECT_MAX_CANDIDATES;

struct DetLevel {
    const float* center;   // (B,1,X,Y,Z)
    const float* bbox;     // (B,6,X,Y,Z)
    const float* cls;      // (B,C,X,Y,Z)
    int X, Y, Z;
    int k;                 // top-k size, 0 = every point
    int seg_off;           // offset of this level's segment in a scene's candidate list
    int pt_off;            // offset of this level's points in a scene's score workspace
    float sx, sy, sz;      // trilinear scales of the valid upsampling: (float)in / out
};

struct WorkSizes {         // of either workspace; caps = min(ncap, kLimit) rows a sorted list can hold, words = ceil(caps / 64)
    int points, ncap, caps, words;
};

struct Work : WorkSizes {  // carved out of the caller's workspace (mvsdet_detect_workspace_bytes)
    int* seg_count;        // (B, kMaxL)
    int* n_sorted;         // (B): candidates of the scene, or -(survivors) above the limit
    float* pscore;         // (B, points) max score per point
    int* plabel;           // (B, points) its class
    float* cbox;           // (B, ncap, 6)
    float* cscore;         // (B, ncap)
    long long* clabel;     // (B, ncap)
    float* sbox;           // (B, caps, 6) sorted
    float* sscore;
    long long* slabel;
    int* sidx;             // candidate index (standalone NMS: the input index)
    unsigned long long* mask;  // (B, caps, words)
};

struct SelectParams {
    DetLevel lv[kMaxL];
    const float* valid;    // (B,1,VX,VY,VZ) view counts as float
    const float* geom;     // (B, L, 6): voxel size, new origin
    int L, C, VX, VY, VZ;
    float score_thr;
};

struct SortParams {
    int L;
    int seg_off[kMaxL];
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// torch.maximum / torch.minimum: NaN in, NaN out
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? __int_as_float(0x7fc00000) : (a > b ? a : b); }
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || b != b) ? __int_as_float(0x7fc00000) : (a < b ? a : b); }

// exclusive prefix of `flag` over the workgroup (in thread order) and the workgroup's total
__device__ __forceinline__ int block_scan(bool flag, int* wave_cnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        const int c = wave_cnt[w];
        base += w < wave ? c : 0;
        tot += c;
    }
    __syncthreads();
    total = tot;
    return base + pre;
}

// ---------------------------------------------------------------------------------------------------------------- rotated boxes
// ImVoxelHead_ARKit (nerfdet_head.py:902-1056, 1190-1243): one candidate list per scene as above, but every candidate carries all
// its class scores, and mmcv's nms3d runs per (scene, class) segment on (x, y, z, dx, dy, dz, heading) boxes.
constexpr int kRotMaxClasses = 256;

struct RotBox {            // what iou_bev reads of a box: centre and size in BEV, rotated corners, cos / sin of -heading
    float x, y, dx, dy;
    float px[4], py[4];
    float cn, sn;
};

struct RotWork : WorkSizes {   // carved out of the caller's workspace (mvsdet_detect_rotated_workspace_bytes)
    int* ccount;           // (B*C): pairs appended to a segment (may exceed caps: the overflow count)
    int* n_sorted;         // (B*C): boxes of the segment, or -(survivors) above the limit
    int* nkept;            // (B*C)
    float* pscore;         // (B, points) max score per point
    float* cbox;           // (B, ncap, 7) decoded candidates
    float* dscore;         // (B*C, ncap) a candidate's score in the segment's class
    int* eslot;            // (B*C, caps) candidates of the segment, in append order
    float* sbox;           // (B*C, caps, 7) sorted
    float* sscore;
    int* sidx;             // candidate index (standalone NMS: the input index)
    RotBox* sgeo;          // (B*C, caps) the IoU prepass of every sorted box
    int* kept;             // (B*C, caps) sorted rows kept, in pick order
    unsigned long long* mask;  // (B*C, caps, words)
    int C;
};

// _bbox_pred_to_bbox (nerfdet_head.py:1030-1056) of one point: shift = half-differences of the distances, turned about z by the
// angle as rotation_3d_in_axis(axis=2) writes it (einsum of the shift row with [[c, s, 0], [-s, c, 0], [0, 0, 1]], summed in j
// order); the box is (point + shift, the summed distances, the angle)
__device__ __forceinline__ void rotated_decode(float px, float py, float pz, const float* d, float* ob) {
    const float sx = (d[1] - d[0]) / 2.f, sy = (d[3] - d[2]) / 2.f, sz = (d[5] - d[4]) / 2.f;
    const float c = cosf(d[6]), s = sinf(d[6]);
    float rx = sx * c;
    rx = rx + sy * -s;
    rx = rx + sz * 0.f;
    float ry = sx * s;
    ry = ry + sy * c;
    ry = ry + sz * 0.f;
    float rz = sx * 0.f;
    rz = rz + sy * 0.f;
    rz = rz + sz * 1.f;
    ob[0] = px + rx;
    ob[1] = py + ry;
    ob[2] = pz + rz;
    ob[3] = d[0] + d[1];
    ob[4] = d[2] + d[3];
    ob[5] = d[4] + d[5];
    ob[6] = d[6];
}

// Appends (slot, score) to segment `seg` where `pass`; one global atomic per wave and segment.  Every lane of the wave calls it.
__device__ __forceinline__ void rotated_append(const RotWork& w, int seg, bool pass, int slot, float score) {
    const unsigned long long m = __ballot(pass);
    if (!m) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&w.ccount[seg], __popcll(m));
    base = __shfl(base, leader);
    if (pass) {
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        w.dscore[(size_t)seg * w.ncap + slot] = score;
        if (pos < w.caps) w.eslot[(size_t)seg * w.caps + pos] = slot;
    }
}

// The prepass of mmcv's box_overlap (iou3d_cuda_kernel.cuh, OpenPCDet-derived): the axis-aligned corners (x1,y1), (x2,y1),
// (x2,y2), (x1,y2), each turned about the centre by the heading, and check_in_box2d's cos / sin of -heading.
__device__ __forceinline__ RotBox rot_prep(const float* b) {
    RotBox r;
    r.x = b[0];
    r.y = b[1];
    r.dx = b[3];
    r.dy = b[4];
    const float hx = b[3] / 2.f, hy = b[4] / 2.f;
    const float x1 = b[0] - hx, y1 = b[1] - hy, x2 = b[0] + hx, y2 = b[1] + hy;
    const float ax[4] = {x1, x2, x2, x1}, ay[4] = {y1, y1, y2, y2};
    const float c = cosf(b[6]), s = sinf(b[6]);
    for (int k = 0; k < 4; ++k) {
        const float ux = ax[k] - b[0], uy = ay[k] - b[1];
        r.px[k] = (ux * c - uy * s) + b[0];
        r.py[k] = (ux * s + uy * c) + b[1];
    }
    r.cn = cosf(-b[6]);
    r.sn = sinf(-b[6]);
    return r;
}

// cross(p1, p2, p0) = (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y)
__device__ __forceinline__ float cross3(float p1x, float p1y, float p2x, float p2y, float p0x, float p0y) {
    return (p1x - p0x) * (p2y - p0y) - (p2x - p0x) * (p1y - p0y);
}

// mmcv's intersection(p1, p0, q1, q0): the bounding-rectangle rejection (fminf / fmaxf, as CUDA's min / max of floats), the
// straddle test s1 * s2 > 0 && s3 * s4 > 0, then the crossing point
__device__ __forceinline__ bool seg_cross(float p1x, float p1y, float p0x, float p0y, float q1x, float q1y, float q0x, float q0y,
                                          float& ox, float& oy) {
    if (!(fminf(p0x, p1x) <= fmaxf(q0x, q1x) && fminf(q0x, q1x) <= fmaxf(p0x, p1x) && fminf(p0y, p1y) <= fmaxf(q0y, q1y) &&
          fminf(q0y, q1y) <= fmaxf(p0y, p1y)))
        return false;
    const float s1 = cross3(q0x, q0y, p1x, p1y, p0x, p0y);
    const float s2 = cross3(p1x, p1y, q1x, q1y, p0x, p0y);
    const float s3 = cross3(p0x, p0y, q1x, q1y, q0x, q0y);
    const float s4 = cross3(q1x, q1y, p1x, p1y, q0x, q0y);
    if (!(s1 * s2 > 0.f && s3 * s4 > 0.f)) return false;
    const float s5 = cross3(q1x, q1y, p1x, p1y, p0x, p0y);
    if (fabsf(s5 - s1) > 1e-8f) {
        ox = (s5 * q0x - s1 * q1x) / (s5 - s1);
        oy = (s5 * q0y - s1 * q1y) / (s5 - s1);
    } else {
        const float a0 = p0y - p1y, b0 = p1x - p0x, c0 = p0x * p1y - p1x * p0y;
        const float a1 = q0y - q1y, b1 = q1x - q0x, c1 = q0x * q1y - q1x * q0y;
        const float D = a0 * b1 - a1 * b0;
        ox = (b0 * c1 - b1 * c0) / D;
        oy = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

// check_in_box2d: the point in the box's frame, MARGIN = 1e-2
__device__ __forceinline__ bool in_box(const RotBox& b, float x, float y) {
    const float rx = (x - b.x) * b.cn + (y - b.y) * -b.sn;
    const float ry = (x - b.x) * b.sn + (y - b.y) * b.cn;
    return fabsf(rx) < b.dx / 2.f + 1e-2f && fabsf(ry) < b.dy / 2.f + 1e-2f;
}

// box_overlap(a, b): edge crossings (a's edge i against b's edge j), then b's corner k in a and a's corner k in b; centroid;
// bubble sort by atan2 about it (on angles computed once per point: the comparisons see the same values); shoelace about point 0.
// 24 slots: mmcv's array has 16, which no real pair of boxes fills.
__device__ float box_overlap(const RotBox& a, const RotBox& b) {
    float qx[24], qy[24], ang[24];
    int cnt = 0;
    float sx = 0.f, sy = 0.f;
    for (int i = 0; i < 4; ++i) {
        const int i1 = (i + 1) & 3;
        for (int j = 0; j < 4; ++j) {
            const int j1 = (j + 1) & 3;
            float ox, oy;
            if (seg_cross(a.px[i1], a.py[i1], a.px[i], a.py[i], b.px[j1], b.py[j1], b.px[j], b.py[j], ox, oy)) {
                sx = sx + ox;
                sy = sy + oy;
                qx[cnt] = ox;
                qy[cnt] = oy;
                ++cnt;
            }
        }
    }
    for (int k = 0; k < 4; ++k) {
        if (in_box(a, b.px[k], b.py[k])) {
            sx = sx + b.px[k];
            sy = sy + b.py[k];
            qx[cnt] = b.px[k];
            qy[cnt] = b.py[k];
            ++cnt;
        }
        if (in_box(b, a.px[k], a.py[k])) {
            sx = sx + a.px[k];
            sy = sy + a.py[k];
            qx[cnt] = a.px[k];
            qy[cnt] = a.py[k];
            ++cnt;
        }
    }
    if (cnt < 2) return 0.f;   // no shoelace term (mmcv: area 0)
    const float cx = sx / (float)cnt, cy = sy / (float)cnt;
    for (int k = 0; k < cnt; ++k) ang[k] = atan2f(qy[k] - cy, qx[k] - cx);
    for (int j = 0; j < cnt - 1; ++j) {
        for (int i = 0; i < cnt - j - 1; ++i) {
            if (ang[i] > ang[i + 1]) {
                float t = ang[i];
                ang[i] = ang[i + 1];
                ang[i + 1] = t;
                t = qx[i];
                qx[i] = qx[i + 1];
                qx[i + 1] = t;
                t = qy[i];
                qy[i] = qy[i + 1];
                qy[i + 1] = t;
            }
        }
    }
    float area = 0.f;
    for (int k = 0; k < cnt - 1; ++k) {
        const float ax = qx[k] - qx[0], ay = qy[k] - qy[0], bx = qx[k + 1] - qx[0], by = qy[k + 1] - qy[0];
        area += ax * by - ay * bx;
    }
    return fabsf(area) / 2.f;
}

// iou_bev(a, b) = overlap / fmaxf(sa + sb - overlap, 1e-8).  Early exit with overlap 0 where box_overlap provably finds no point:
// every corner lies within half a diagonal of its centre (a crossing lies on both boxes' edges), and a corner inside the other box's
// margin lies within that box's half-diagonal + sqrt(2) * 1e-2; the test adds 2e-2 and 1e-5 of the coordinates' scale for the
// rounding of the corners.  NaN or infinite distances take the full path.
__device__ __forceinline__ float rot_iou(const RotBox& a, const RotBox& b) {
    const float ex = b.x - a.x, ey = b.y - a.y;
    const float ra = 0.5f * sqrtf(a.dx * a.dx + a.dy * a.dy), rb = 0.5f * sqrtf(b.dx * b.dx + b.dy * b.dy);
    const float reach = (ra + rb + 2e-2f) + 1e-5f * (fabsf(a.x) + fabsf(a.y) + fabsf(b.x) + fabsf(b.y) + ra + rb);
    const float sa = a.dx * a.dy, sb = b.dx * b.dy;
    const float ov = (ex * ex + ey * ey > reach * reach) ? 0.f : box_overlap(a, b);
    return ov / fmaxf((sa + sb) - ov, 1e-8f);
}

// ---------------------------------------------------------------------------------------------------------------- selection
// nn.Upsample(trilinear)(valid).round().bool() at voxel (x, y, z) of level lv, as 0 / 1 (head_points.h)
__device__ __forceinline__ float valid_at(const SelectParams& p, const DetLevel& lv, const float* valid, int x, int y, int z) {
    return upsampled_valid(valid, p.VX, p.VY, p.VZ, lv.sx, lv.sy, lv.sz, x, y, z);
}

// get_points of voxel i of a level: its (x, y, z), and the point = voxel * voxel size + new origin (g: a row of SelectParams::geom)
__device__ __forceinline__ void voxel_point(const DetLevel& lv, const float* g, int i, int& x, int& y, int& z, float& px, float& py,
                                            float& pz) {
    x = i / (lv.Y * lv.Z), y = (i / lv.Z) % lv.Y, z = i % lv.Z;
    grid_point(g, x, y, z, px, py, pz);
}

// kRot = false: the ScanNet head (6 regression channels, Work).  kRot = true: ImVoxelHead_ARKit (7 channels, RotWork): every
// top-k point is decoded into the scene's candidate list, and each of its (class, score > score_thr) pairs joins the (scene, class)
// segment (rotated part below).
template <bool kRot>
__global__ __launch_bounds__(kSelThreads) void detect_select_kernel(SelectParams p, std::conditional_t<kRot, RotWork, Work> w) {
    __shared__ int hist[256];
    __shared__ int wave_cnt[kSelThreads / 64];
    __shared__ int sel[2];
    constexpr int R = kRot ? 7 : 6;
    const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const DetLevel lv = p.lv[l];
    const int YZ = lv.Y * lv.Z, N = lv.X * YZ, C = p.C;
    const float* ctr = lv.center + (size_t)b * N;
    const float* cls = lv.cls + (size_t)b * C * N;
    const float* box = lv.bbox + (size_t)b * R * N;
    const float* valid = p.valid + (size_t)b * p.VX * p.VY * p.VZ;
    float* ps = w.pscore + (size_t)b * w.points + lv.pt_off;

    // 1. scores: nn.Upsample(trilinear)(valid).round().bool(); sigmoid(cls) * sigmoid(center) * valid; max / first argmax
    for (int i = tid; i < N; i += kSelThreads) {
        const int x = i / YZ, y = (i / lv.Z) % lv.Y, z = i % lv.Z;
        const float vm = valid_at(p, lv, valid, x, y, z);
        const float sc = sigmoidf_(ctr[i]);
        float best = (sigmoidf_(cls[i]) * sc) * vm;
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float s = (sigmoidf_(cls[(size_t)c * N + i]) * sc) * vm;
            if (!(best != best) && (s != s || s > best)) {
                best = s;
                arg = c;
            }
        }
        ps[i] = best;
        if constexpr (!kRot) w.plabel[(size_t)b * w.points + lv.pt_off + i] = arg;
    }
    __syncthreads();

    // 2. top-k threshold: the k-th largest score bits (scores are >= 0: their bits order like their values), 8 bits a pass
    unsigned T = 0;
    int need_eq = 0;
    if (lv.k > 0) {   // need_eq: points with bits == T to take, lowest voxel index first
        T = radix_select_kth(hist, sel, N, lv.k, need_eq, [&](int i, unsigned& u) {
            u = __float_as_uint(ps[i]);
            return true;
        });
    }

    // 3. compaction in voxel order: (top-k) and score > score_thr -> decoded box, score, label
    //    (rotated: every top-k point -> decoded box; its classes with score > score_thr -> their segments)
    const float* gp = p.geom + ((size_t)b * p.L + l) * 6;
    const float g[6] = {gp[0], gp[1], gp[2], gp[3], gp[4], gp[5]};
    const size_t cbase = (size_t)b * w.ncap + lv.seg_off;
    int base = 0, eq_base = 0;
    for (int c0 = 0; c0 < N; c0 += kSelThreads) {
        const int i = c0 + tid;
        const bool in = i < N;
        const float s = in ? ps[i] : 0.f;
        const unsigned u = __float_as_uint(s);
        bool take = in;
        if (lv.k > 0) {
            int eq_tot;
            const bool eq = in && u == T;
            const int r = block_scan(eq, wave_cnt, eq_tot);
            take = in && (u > T || (eq && eq_base + r < need_eq));
            eq_base += eq_tot;
        }
        if constexpr (kRot) {
            int tot;
            const int r = block_scan(take, wave_cnt, tot);
            float sc = 0.f, vm = 0.f;
            if (take) {
                int x, y, z;
                float px, py, pz;
                voxel_point(lv, g, i, x, y, z, px, py, pz);
                float d[7];
                for (int q = 0; q < 7; ++q) d[q] = box[(size_t)q * N + i];
                rotated_decode(px, py, pz, d, w.cbox + (cbase + base + r) * 7);
                sc = sigmoidf_(ctr[i]);
                vm = valid_at(p, lv, valid, x, y, z);
            }
            const int slot = lv.seg_off + base + r;   // scene-relative candidate index: level, then voxel order
            for (int c = 0; c < C; ++c) {
                float sv = 0.f;
                if (take) sv = (sigmoidf_(cls[(size_t)c * N + i]) * sc) * vm;
                rotated_append(w, b * C + c, take && sv > p.score_thr, slot, sv);
            }
            base += tot;
        } else {
            const bool keep = take && s > p.score_thr;
            int tot;
            const int r = block_scan(keep, wave_cnt, tot);
            if (keep) {
                int x, y, z;
                float px, py, pz;
                voxel_point(lv, g, i, x, y, z, px, py, pz);
                const size_t ci = cbase + base + r;
                float* ob = w.cbox + ci * 6;
                ob[0] = px - box[i];
                ob[1] = py - box[(size_t)2 * N + i];
                ob[2] = pz - box[(size_t)4 * N + i];
                ob[3] = px + box[(size_t)1 * N + i];
                ob[4] = py + box[(size_t)3 * N + i];
                ob[5] = pz + box[(size_t)5 * N + i];
                w.cscore[ci] = s;
                w.clabel[ci] = w.plabel[(size_t)b * w.points + lv.pt_off + i];
            }
            base += tot;
        }
    }
    if constexpr (!kRot) {
        if (tid == 0) w.seg_count[b * kMaxL + l] = base;
    }
}

// standalone NMS: the caller's boxes / scores / classes as the one-level candidate list of one scene
__global__ void detect_load_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, const long long* __restrict__ classes,
                                   int n, Work w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) w.seg_count[0] = n;
    if (i >= n) return;
    for (int c = 0; c < 6; ++c) w.cbox[(size_t)i * 6 + c] = boxes[(size_t)i * 6 + c];
    w.cscore[i] = scores[i];
    w.clabel[i] = classes[i];
}

// ---------------------------------------------------------------------------------------------------------------- sort
// float -> unsigned with the same order: every NaN, whatever its sign and payload, one key above +inf (torch.sort places NaN
// last, so the reference's greedy loop visits it first); -0 the key of +0, so equal scores fall back to the index
__device__ __forceinline__ unsigned order_bits(float f) {
    if (f != f) return 0xffffffffu;
    unsigned u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ascending bitonic sort of P (a power of two) keys in LDS by the whole workgroup (kSortThreads threads)
__device__ __forceinline__ void bitonic_sort(unsigned long long* keys, int P) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += kSortThreads) {
                const int i = 2 * t - (t & (j - 1));
                const unsigned long long a = keys[i], c = keys[i + j];
                if ((a > c) == ((i & k) == 0)) {
                    keys[i] = c;
                    keys[i + j] = a;
                }
            }
            __syncthreads();
        }
    }
}

struct ScoreIndex {
    float score;
    int index;
};

// One list of `total` elements by the whole workgroup: above `caps` elements n_sorted = -total and false; else the keys
// (~order_bits(score) << 32) | index of element_of(e), e < total, sorted ascending in keys[0, total) (score descending, NaN first,
// then index ascending; the padding up to the power of two sorts behind every element), n_sorted = total and true.
template <class ElementOf>
__device__ __forceinline__ bool sort_keys(unsigned long long* keys, int total, int caps, int* n_sorted, ElementOf element_of) {
    if (total > caps) {
        if (threadIdx.x == 0) *n_sorted = -total;
        return false;
    }
    int P = 1;
    while (P < total) P <<= 1;
    for (int e = threadIdx.x; e < P; e += kSortThreads) {
        unsigned long long key = ~0ull;
        if (e < total) {
            const ScoreIndex s = element_of(e);
            key = ((unsigned long long)(~order_bits(s.score)) << 32) | (unsigned)s.index;
        }
        keys[e] = key;
    }
    __syncthreads();
    bitonic_sort(keys, P);
    if (threadIdx.x == 0) *n_sorted = total;
    return true;
}

// one workgroup per scene: the levels' segments as one list, keyed by the level-major concatenated index
__global__ __launch_bounds__(kSortThreads) void detect_sort_kernel(SortParams q, Work w, int pmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];   // [pmax] keys, then the level counts / prefixes
    int* cnt = reinterpret_cast<int*>(keys + pmax);
    int* pre = cnt + kMaxL;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int acc = 0;
        for (int l = 0; l < q.L; ++l) {
            cnt[l] = w.seg_count[b * kMaxL + l];
            pre[l] = acc;
            acc += cnt[l];
        }
        pre[kMaxL] = acc;
    }
    __syncthreads();
    const int total = pre[kMaxL];
    auto cand = [&](int e) {   // concatenated (level-major) candidate index -> slot of the candidate buffer
        int l = 0;
        while (l + 1 < q.L && e >= pre[l + 1]) ++l;
        return (size_t)b * w.ncap + q.seg_off[l] + (e - pre[l]);
    };
    if (!sort_keys(keys, total, w.caps, w.n_sorted + b, [&](int e) { return ScoreIndex{w.cscore[cand(e)], e}; })) return;
    const size_t sb = (size_t)b * w.caps;
    for (int r = tid; r < total; r += kSortThreads) {
        const int e = (int)(keys[r] & 0xffffffffu);
        const size_t ci = cand(e);
        for (int c = 0; c < 6; ++c) w.sbox[(sb + r) * 6 + c] = w.cbox[ci * 6 + c];
        w.sscore[sb + r] = w.cscore[ci];
        w.slabel[sb + r] = w.clabel[ci];
        w.sidx[sb + r] = e;
    }
}

// ---------------------------------------------------------------------------------------------------------------- IoU mask
// Tile (rb, cbk) of one sorted list of n boxes by a 64-thread workgroup: the columns 64 cbk + t staged in LDS, then bit jj of word
// cbk of row i = 64 rb + t is pair(box i, box 64 cbk + jj) for 64 cbk + jj > i (the earlier box first).  load(r) is the record of
// sorted row r; `rows` the list's mask rows.
template <class Box, class Load, class Pair>
__device__ __forceinline__ void mask_tile(Box* cb, unsigned long long* rows, int words, int n, int rb, int cbk, Load load, Pair pair) {
    const int t = threadIdx.x;
    const int j = cbk * 64 + t;
    if (j < n) cb[t] = load(j);
    __syncthreads();
    const int i = rb * 64 + t;
    if (i >= n) return;
    const Box a = load(i);
    const int ncol = min(64, n - cbk * 64);
    unsigned long long bits = 0;
    for (int jj = 0; jj < ncol; ++jj)
        if (cbk * 64 + jj > i && pair(a, cb[jj])) bits |= 1ull << jj;
    rows[(size_t)i * words + cbk] = bits;
}

struct __attribute__((packed, aligned(4))) AlignedBox {   // 36 bytes: 64 of them take the LDS the separate arrays took
    float x[6];            // (x1, y1, z1, x2, y2, z2)
    float area;
    long long label;
};

// aligned_3d_nms's suppression test of the later box c by the earlier box a, op for op:
//   inter = max(0, min(x2) - max(x1)) * max(0, ..y..) * max(0, ..z..);  iou = inter / (area_i + area_j - inter) * (cls_i == cls_j)
//   j goes when !(iou <= thr): NaN (zero-volume / infinite boxes) suppresses, across classes too (NaN * 0)
__device__ __forceinline__ bool suppresses(const AlignedBox& a, const AlignedBox& c, float thr) {
    const float xx1 = nan_max(a.x[0], c.x[0]), yy1 = nan_max(a.x[1], c.x[1]), zz1 = nan_max(a.x[2], c.x[2]);
    const float xx2 = nan_min(a.x[3], c.x[3]), yy2 = nan_min(a.x[4], c.x[4]), zz2 = nan_min(a.x[5], c.x[5]);
    const float il = nan_max(0.f, xx2 - xx1), iw = nan_max(0.f, yy2 - yy1), ih = nan_max(0.f, zz2 - zz1);
    const float inter = (il * iw) * ih;
    float iou = inter / ((a.area + c.area) - inter);
    iou = iou * (a.label == c.label ? 1.f : 0.f);
    return !(iou <= thr);
}

// one tile per workgroup of a (words, words, B) grid; the tiles below the diagonal and behind the scene's boxes return at once
__global__ __launch_bounds__(64) void detect_mask_kernel(Work w, float thr) {
    __shared__ AlignedBox cb[64];
    const int cbk = blockIdx.x, rb = blockIdx.y, b = blockIdx.z;
    const int n = w.n_sorted[b];
    if (cbk < rb || rb * 64 >= n || cbk * 64 >= n) return;
    const size_t sb = (size_t)b * w.caps;
    auto load = [&](int r) {
        AlignedBox v;
        for (int c = 0; c < 6; ++c) v.x[c] = w.sbox[(sb + r) * 6 + c];
        v.area = ((v.x[3] - v.x[0]) * (v.x[4] - v.x[1])) * (v.x[5] - v.x[2]);
        v.label = w.slabel[sb + r];
        return v;
    };
    mask_tile(cb, w.mask + sb * w.words, w.words, n, rb, cbk, load,
              [thr](const AlignedBox& a, const AlignedBox& c) { return suppresses(a, c, thr); });
}

// ---------------------------------------------------------------------------------------------------------------- greedy walk
__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int lane) {
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, lane), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// The walk over one sorted list of n boxes (n <= 0: none) by a workgroup of kScanThreads, `rows` its mask rows.  Boxes 64 at a
// time: every wave loads the block's diagonal mask words (lane j: row 64 w + j, word w) and walks them with the block's entry of
// the removed set (the same decisions in every wave); the workgroup then ORs the kept rows into the removed words behind the block.
// Wave 0's lane of a kept row calls emit(k, row): the row is the k-th pick.  Returns the number kept, in every thread.
template <class Emit>
__device__ __forceinline__ int greedy_walk(const unsigned long long* rows, int words, int n, Emit emit) {
    __shared__ unsigned long long removed[kLimit / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = n > 0 ? (n + 63) / 64 : 0;
    for (int q = tid; q < W; q += kScanThreads) removed[q] = 0;
    __syncthreads();
    int kept = 0;
    unsigned long long diag = (W > 0 && lane < n) ? rows[(size_t)lane * words] : 0ull;
    for (int blk = 0; blk < W; ++blk) {
        const int nb = min(64, n - blk * 64);
        unsigned long long rem = removed[blk];
        if (nb < 64) rem |= ~0ull << nb;
        const unsigned long long row = diag;
        if (blk + 1 < W) {   // next block's diagonal words: they do not depend on this block's decisions
            const int i = (blk + 1) * 64 + lane;
            diag = i < n ? rows[(size_t)i * words + blk + 1] : 0ull;
        }
        unsigned long long keptmask = 0, todo = ~rem;
        while (todo) {
            const int j = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
            keptmask |= 1ull << j;
            rem |= readlane64(row, j);
            todo = j == 63 ? 0ull : (~rem & (~0ull << (j + 1)));
        }
        const int later = W - blk - 1;
        for (int pq = tid; pq < 64 * later; pq += kScanThreads) {
            const int j = pq / later, qw = blk + 1 + pq % later;
            if ((keptmask >> j) & 1ull) {
                const unsigned long long v = rows[(size_t)(blk * 64 + j) * words + qw];
                if (v) atomicOr(&removed[qw], v);
            }
        }
        if (wave == 0 && ((keptmask >> lane) & 1ull)) emit(kept + __popcll(keptmask & ((1ull << lane) - 1ull)), blk * 64 + lane);
        kept += __popcll(keptmask);
        __syncthreads();
    }
    return kept;
}

// one workgroup per scene.  Head route: the kept boxes converted to (centre, size), scores, labels, then the zero padding;
// standalone: the input indices.
__global__ __launch_bounds__(kScanThreads) void detect_scan_kernel(Work w, float* out_boxes, float* out_scores, long long* out_labels,
                                                                   long long* out_index, int* out_count, int nmax) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = w.n_sorted[b];
    const size_t sb = (size_t)b * w.caps;
    const int kept = greedy_walk(w.mask + sb * w.words, w.words, n, [&](int k, int row) {
        const size_t r = sb + row;
        if (out_index) {
            out_index[(size_t)b * nmax + k] = w.sidx[r];
        } else {
            const float* x = w.sbox + r * 6;
            float* o = out_boxes + ((size_t)b * nmax + k) * 6;
            o[0] = (x[0] + x[3]) / 2.f;
            o[1] = (x[1] + x[4]) / 2.f;
            o[2] = (x[2] + x[5]) / 2.f;
            o[3] = x[3] - x[0];
            o[4] = x[4] - x[1];
            o[5] = x[5] - x[2];
            out_scores[(size_t)b * nmax + k] = w.sscore[r];
            out_labels[(size_t)b * nmax + k] = w.slabel[r];
        }
    });
    if (!out_index) {
        for (int k = kept + tid; k < nmax; k += kScanThreads) {
            float* o = out_boxes + ((size_t)b * nmax + k) * 6;
            for (int c = 0; c < 6; ++c) o[c] = 0.f;
            out_scores[(size_t)b * nmax + k] = 0.f;
            out_labels[(size_t)b * nmax + k] = 0;
        }
    }
    if (tid == 0) out_count[b] = n < 0 ? n : kept;
}

// ---------------------------------------------------------------------------------------------------------------- rotated NMS
// standalone nms3d: the caller's boxes / scores as the one segment of one scene
__global__ void rot_load_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, int n, RotWork w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) w.ccount[0] = n;
    if (i >= n) return;
    for (int c = 0; c < 7; ++c) w.cbox[(size_t)i * 7 + c] = boxes[(size_t)i * 7 + c];
    w.dscore[i] = scores[i];
    w.eslot[i] = i;
}

// one workgroup per (scene, class) segment: the segment's candidates keyed by their scene-relative index (append order is sorted
// away), then the sorted boxes, scores, candidate indices and the IoU prepass of every box
__global__ __launch_bounds__(kSortThreads) void rot_sort_kernel(RotWork w, int pmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    const int seg = blockIdx.x, b = seg / w.C, tid = threadIdx.x;
    const int total = w.ccount[seg];
    const size_t eb = (size_t)seg * w.caps, db = (size_t)seg * w.ncap;
    auto element = [&](int e) {
        const int slot = w.eslot[eb + e];
        return ScoreIndex{w.dscore[db + slot], slot};
    };
    if (!sort_keys(keys, total, w.caps, w.n_sorted + seg, element)) return;
    for (int r = tid; r < total; r += kSortThreads) {
        const int slot = (int)(keys[r] & 0xffffffffu);
        const float* x = w.cbox + ((size_t)b * w.ncap + slot) * 7;
        float* o = w.sbox + (eb + r) * 7;
        for (int c = 0; c < 7; ++c) o[c] = x[c];
        w.sscore[eb + r] = w.dscore[db + slot];
        w.sidx[eb + r] = slot;
        w.sgeo[eb + r] = rot_prep(x);
    }
}

// 64 x 64 tiles of the upper triangle of every segment, gridDim.x workgroups striding over a segment's tiles: the pair test is
// iou_bev(box i, box j) > thr (mmcv's nms3d kernel), on the prepass records the sort left
__global__ __launch_bounds__(64) void rot_mask_kernel(RotWork w, float thr) {
    __shared__ RotBox cb[64];
    const int seg = blockIdx.y;
    const int n = w.n_sorted[seg];
    if (n <= 0) return;
    const int W = (n + 63) / 64, T = W * (W + 1) / 2;
    const size_t sb = (size_t)seg * w.caps;
    for (int tile = blockIdx.x; tile < T; tile += gridDim.x) {
        int rb = 0, rest = tile;
        while (rest >= W - rb) {
            rest -= W - rb;
            ++rb;
        }
        __syncthreads();   // the previous tile's columns are read
        mask_tile(cb, w.mask + sb * w.words, w.words, n, rb, rb + rest, [&](int r) { return w.sgeo[sb + r]; },
                  [thr](const RotBox& a, const RotBox& c) { return rot_iou(a, c) > thr; });
    }
}

// one workgroup per segment: kept sorted rows in pick order
__global__ __launch_bounds__(kScanThreads) void rot_scan_kernel(RotWork w) {
    const int seg = blockIdx.x;
    const size_t sb = (size_t)seg * w.caps;
    const int kept = greedy_walk(w.mask + sb * w.words, w.words, w.n_sorted[seg], [&](int k, int row) { w.kept[sb + k] = row; });
    if (threadIdx.x == 0) w.nkept[seg] = kept;
}

// one workgroup per scene: the kept boxes class-major (classes ascending, each in pick order), then the zero padding.  A scene with
// a segment above the limit: count -(the largest such segment), every row zero.  Standalone: the kept input indices.
__global__ __launch_bounds__(256) void rot_gather_kernel(RotWork w, float* out_boxes, float* out_scores, long long* out_labels,
                                                         long long* out_index, int* out_count, int nmax) {
    __shared__ int off[kRotMaxClasses + 1];
    __shared__ int worst;
    const int b = blockIdx.x, tid = threadIdx.x, C = w.C;
    if (tid == 0) {
        int acc = 0, bad = 0;
        for (int c = 0; c < C; ++c) {
            const int n = w.n_sorted[b * C + c];
            if (n < 0) bad = max(bad, -n);
            off[c] = acc;
            acc += n < 0 ? 0 : w.nkept[b * C + c];
        }
        off[C] = bad ? 0 : acc;
        worst = bad;
    }
    __syncthreads();
    const int total = off[C];
    if (total > 0) {
        for (int c = 0; c < C; ++c) {
            const int seg = b * C + c, nk = w.nkept[seg];
            const size_t sb = (size_t)seg * w.caps;
            for (int k = tid; k < nk; k += blockDim.x) {
                const size_t r = sb + w.kept[sb + k];
                const size_t o = (size_t)b * nmax + off[c] + k;
                if (out_index) {
                    out_index[o] = w.sidx[r];
                } else {
                    for (int q = 0; q < 7; ++q) out_boxes[o * 7 + q] = w.sbox[r * 7 + q];
                    out_scores[o] = w.sscore[r];
                    out_labels[o] = c;
                }
            }
        }
    }
    if (!out_index) {
        for (int k = total + tid; k < nmax; k += blockDim.x) {
            const size_t o = (size_t)b * nmax + k;
            for (int q = 0; q < 7; ++q) out_boxes[o * 7 + q] = 0.f;
            out_scores[o] = 0.f;
            out_labels[o] = 0;
        }
    }
    if (tid == 0) out_count[b] = worst ? -worst : total;
}

// every (i, j) pair of two box lists through the device IoU (early exit included)
__global__ void rot_iou_kernel(const float* __restrict__ a, int n, const float* __restrict__ b, int m, float* __restrict__ out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long long)n * m) return;
    const int i = (int)(q / m), j = (int)(q % m);
    out[q] = rot_iou(rot_prep(a + (size_t)i * 7), rot_prep(b + (size_t)j * 7));
}

// Hands out the arrays of a workspace in order, each aligned to 256 bytes; `off` ends as the bytes needed.  Without a base every
// pointer is null: the size query.
struct Carver {
    char* base;
    size_t off = 0;
    template <class T>
    void take(T*& ptr, size_t count) {
        ptr = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
    }
};

WorkSizes work_sizes(int points, int ncap) {
    const int caps = std::min(ncap, kLimit);
    return {points, ncap, caps, (caps + 63) / 64};
}

// workspace layout; returns the bytes needed
size_t carve(void* base, int B, int points, int ncap, Work* w) {
    Work t{work_sizes(points, ncap)};
    const size_t nb = B, cand = nb * ncap, rows = nb * t.caps;
    Carver c{static_cast<char*>(base)};
    c.take(t.seg_count, nb * kMaxL);
    c.take(t.n_sorted, nb);
    c.take(t.pscore, nb * points);
    c.take(t.plabel, nb * points);
    c.take(t.cbox, cand * 6);
    c.take(t.cscore, cand);
    c.take(t.clabel, cand);
    c.take(t.sbox, rows * 6);
    c.take(t.sscore, rows);
    c.take(t.slabel, rows);
    c.take(t.sidx, rows);
    c.take(t.mask, rows * t.words);
    if (w) *w = t;
    return c.off;
}

// rotated workspace layout; returns the bytes needed
size_t carve_rotated(void* base, int B, int points, int ncap, int C, RotWork* w) {
    RotWork t{work_sizes(points, ncap)};
    t.C = C;
    const size_t nb = B, S = nb * C, rows = S * t.caps;
    Carver c{static_cast<char*>(base)};
    c.take(t.ccount, S);
    c.take(t.n_sorted, S);
    c.take(t.nkept, S);
    c.take(t.pscore, nb * points);
    c.take(t.cbox, nb * ncap * 7);
    c.take(t.dscore, S * ncap);
    c.take(t.eslot, rows);
    c.take(t.sbox, rows * 7);
    c.take(t.sscore, rows);
    c.take(t.sidx, rows);
    c.take(t.sgeo, rows);
    c.take(t.kept, rows);
    c.take(t.mask, rows * t.words);
    if (w) *w = t;
    return c.off;
}

int check_workspace(const char* name, const void* workspace, size_t bytes, size_t need, const char* query) {
    if (workspace && bytes >= need) return MVSDET_OK;
    set_error("%s: workspace of %zu bytes, %zu needed (%s)", name, bytes, need, query);
    return MVSDET_ERR_WORKSPACE;
}

// LDS of a sort kernel: a power of two of keys that holds `caps`, then `extra` bytes; above 64 KiB the kernel is told so -- granted
// the LDS of a list at the candidate limit, not this list's: another host thread's larger list may be between its grant and its launch
template <class Kernel>
int sort_lds(Kernel* kernel, int caps, size_t extra, const char* name, int* pmax, size_t* lds) {
    *pmax = 1;
    while (*pmax < std::max(caps, 1)) *pmax <<= 1;
    *lds = (size_t)*pmax * 8 + extra;
    static_assert((kLimit & (kLimit - 1)) == 0, "the ceiling below: kLimit keys, a power of two");
    if (*lds > 64 * 1024) MVS_GRANT_LDS(name, kernel, *lds, (size_t)kLimit * 8 + extra);
    return MVSDET_OK;
}

// sort, mask and walk of the candidate lists in `w` (segments and counts written by the first launch)
int sort_mask_scan(const Work& w, const SortParams& q, int B, float thr, float* out_boxes, float* out_scores, long long* out_labels,
                   long long* out_index, int* out_count, int nmax, hipStream_t stream, const char* name) {
    int pmax;
    size_t lds;
    if (const int rc = sort_lds(detect_sort_kernel, w.caps, (2 * kMaxL + 1) * 4, name, &pmax, &lds)) return rc;
    hipLaunchKernelGGL(detect_sort_kernel, dim3(B), dim3(kSortThreads), lds, stream, q, w, pmax);
    if (w.words > 0) hipLaunchKernelGGL(detect_mask_kernel, dim3(w.words, w.words, B), dim3(64), 0, stream, w, thr);
    hipLaunchKernelGGL(detect_scan_kernel, dim3(B), dim3(kScanThreads), 0, stream, w, out_boxes, out_scores, out_labels, out_index,
                       out_count, nmax);
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}

// sort, mask, walk and gather of the segments in `w` (filled by the first launch; ccount zeroed before it)
int rotated_sort_mask_scan(const RotWork& w, int B, float thr, float* out_boxes, float* out_scores, long long* out_labels,
                           long long* out_index, int* out_count, int nmax, hipStream_t stream, const char* name) {
    const int S = B * w.C;
    int pmax;
    size_t lds;
    if (const int rc = sort_lds(rot_sort_kernel, w.caps, 0, name, &pmax, &lds)) return rc;
    hipLaunchKernelGGL(rot_sort_kernel, dim3(S), dim3(kSortThreads), lds, stream, w, pmax);
    if (w.words > 0) {
        // tiles of the largest possible segment, at most ~4096 workgroups in all: a segment's workgroups stride over its tiles
        const long long tiles = (long long)w.words * (w.words + 1) / 2;
        const int gx = (int)std::min<long long>(tiles, std::max(8, 4096 / S));
        hipLaunchKernelGGL(rot_mask_kernel, dim3(gx, S), dim3(64), 0, stream, w, thr);
    }
    hipLaunchKernelGGL(rot_scan_kernel, dim3(S), dim3(kScanThreads), 0, stream, w);
    hipLaunchKernelGGL(rot_gather_kernel, dim3(B), dim3(256), 0, stream, w, out_boxes, out_scores, out_labels, out_index, out_count,
                       nmax);
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}

// What both head entry points check and derive of their arguments: the pointers, B, L, n_classes (at most max_classes, and
// B x n_classes at most max_segments where that is not 0), the valid grid, nms_pre and every level.  Fills `p`; `points` and `ncap`
// are a scene's points and the most candidates it can have (per level nms_pre, or all its points).
int plan_select(const char* name, const float* const* center, const float* const* bbox, const float* const* cls, const int* level_dims,
                const float* valid, const float* level_geom, bool outputs, int B, int L, int n_classes, int max_classes,
                int max_segments, int VX, int VY, int VZ, int nms_pre, float score_thr, SelectParams* p, long long* points,
                long long* ncap) {
    MVS_REQUIRE(center && bbox && cls && level_dims && valid && level_geom && outputs, "%s: NULL pointer", name);
    MVS_REQUIRE(B >= 1 && B <= 65535, "%s: bad shape B=%d", name, B);
    MVS_REQUIRE(L >= 1 && L <= MVSDET_DETECT_MAX_LEVELS, "%s: bad shape L=%d (1..%d levels)", name, L, MVSDET_DETECT_MAX_LEVELS);
    MVS_REQUIRE(n_classes >= 1 && n_classes <= max_classes, "%s: bad shape n_classes=%d (1..%d)", name, n_classes, max_classes);
    MVS_REQUIRE(!max_segments || (long long)B * n_classes <= max_segments, "%s: bad shape: %d scenes x %d classes above %d segments",
                name, B, n_classes, max_segments);
    MVS_REQUIRE(VX > 0 && VY > 0 && VZ > 0 && (long long)VX * VY * VZ < (1 << 26), "%s: bad shape valid %dx%dx%d", name, VX, VY, VZ);
    MVS_REQUIRE(nms_pre >= 0, "%s: nms_pre=%d < 0", name, nms_pre);
    *p = SelectParams{};
    *points = *ncap = 0;
    for (int l = 0; l < L; ++l) {
        MVS_REQUIRE(center[l] && bbox[l] && cls[l], "%s: NULL pointer (level %d)", name, l);
        const int X = level_dims[3 * l], Y = level_dims[3 * l + 1], Z = level_dims[3 * l + 2];
        MVS_REQUIRE(X > 0 && Y > 0 && Z > 0 && (long long)X * Y * Z < (1 << 24), "%s: bad shape level %d: %dx%dx%d", name, l, X, Y, Z);
        const int N = X * Y * Z;
        DetLevel& lv = p->lv[l];
        lv.center = center[l];
        lv.bbox = bbox[l];
        lv.cls = cls[l];
        lv.X = X;
        lv.Y = Y;
        lv.Z = Z;
        lv.k = (N > nms_pre && nms_pre > 0) ? nms_pre : 0;
        lv.seg_off = (int)*ncap;
        lv.pt_off = (int)*points;
        lv.sx = (float)VX / (float)X;
        lv.sy = (float)VY / (float)Y;
        lv.sz = (float)VZ / (float)Z;
        *points += N;
        *ncap += lv.k > 0 ? lv.k : N;
    }
    p->valid = valid;
    p->geom = level_geom;
    p->L = L;
    p->C = n_classes;
    p->VX = VX;
    p->VY = VY;
    p->VZ = VZ;
    p->score_thr = score_thr;
    return MVSDET_OK;
}

}  // namespace
}  // namespace mvsdet

using namespace mvsdet;

extern "C" size_t mvsdet_detect_workspace_bytes(int B, int points, int ncap) {
    if (B <= 0 || points < 0 || ncap < 0) return 0;
    return carve(nullptr, B, points, ncap, nullptr);
}

extern "C" int mvsdet_detect_head_f32(const float* const* center, const float* const* bbox, const float* const* cls,
                                      const int* level_dims, const float* valid, const float* level_geom, int B, int L, int n_classes,
                                      int VX, int VY, int VZ, int nms_pre, float score_thr, float iou_thr, float* out_boxes,
                                      float* out_scores, int64_t* out_labels, int* out_count, int nmax, void* workspace,
                                      size_t workspace_bytes, mvsdet_stream_t stream) {
    const char* name = "detect_head";
    SelectParams p;
    long long points, ncap;
    if (const int rc = plan_select(name, center, bbox, cls, level_dims, valid, level_geom, out_boxes && out_scores && out_labels && out_count,
                                   B, L, n_classes, 1024, 0, VX, VY, VZ, nms_pre, score_thr, &p, &points, &ncap))
        return rc;
    MVS_REQUIRE((long long)B * points < (1ll << 31) && (long long)B * ncap < (1ll << 31), "%s: bad shape: %d scenes x %lld points", name,
                B, points);
    const int caps = (int)std::min<long long>(ncap, kLimit);
    MVS_REQUIRE(nmax >= caps, "%s: Nmax=%d < %d, the most boxes a scene can keep here (min(candidates, %d))", name, nmax, caps, kLimit);
    if (const int rc = check_workspace(name, workspace, workspace_bytes, mvsdet_detect_workspace_bytes(B, (int)points, (int)ncap),
                                       "mvsdet_detect_workspace_bytes"))
        return rc;
    Work w;
    carve(workspace, B, (int)points, (int)ncap, &w);
    SortParams q{};
    q.L = L;
    for (int l = 0; l < L; ++l) q.seg_off[l] = p.lv[l].seg_off;
    hipLaunchKernelGGL(detect_select_kernel<false>, dim3(L, B), dim3(kSelThreads), 0, (hipStream_t)stream, p, w);
    return sort_mask_scan(w, q, B, iou_thr, out_boxes, out_scores, reinterpret_cast<long long*>(out_labels), nullptr, out_count, nmax,
                          (hipStream_t)stream, name);
}

extern "C" int mvsdet_aligned_3d_nms_f32(const float* boxes, const float* scores, const int64_t* classes, int n, float thresh,
                                         int64_t* out_index, int* out_count, void* workspace, size_t workspace_bytes,
                                         mvsdet_stream_t stream) {
    const char* name = "aligned_3d_nms";
    MVS_REQUIRE(out_index && out_count, "%s: NULL pointer", name);
    MVS_REQUIRE(n >= 0, "%s: bad shape n=%d", name, n);
    MVS_REQUIRE(n <= MVSDET_DETECT_MAX_CANDIDATES, "%s: n=%d boxes above the candidate limit MVSDET_DETECT_MAX_CANDIDATES=%d", name, n,
                MVSDET_DETECT_MAX_CANDIDATES);
    MVS_REQUIRE(n == 0 || (boxes && scores && classes), "%s: NULL pointer", name);
    if (const int rc = check_workspace(name, workspace, workspace_bytes, mvsdet_detect_workspace_bytes(1, 0, n),
                                       "mvsdet_detect_workspace_bytes"))
        return rc;
    Work w;
    carve(workspace, 1, 0, n, &w);
    SortParams q{};
    q.L = 1;
    hipLaunchKernelGGL(detect_load_kernel, dim3(std::max(1, (n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, boxes, scores,
                       reinterpret_cast<const long long*>(classes), n, w);
    return sort_mask_scan(w, q, 1, thresh, nullptr, nullptr, nullptr, reinterpret_cast<long long*>(out_index), out_count, std::max(n, 1),
                          (hipStream_t)stream, name);
}

extern "C" size_t mvsdet_detect_rotated_workspace_bytes(int B, int points, int ncap, int n_classes) {
    if (B <= 0 || points < 0 || ncap < 0 || n_classes <= 0) return 0;
    return carve_rotated(nullptr, B, points, ncap, n_classes, nullptr);
}

extern "C" int mvsdet_detect_head_rotated_f32(const float* const* center, const float* const* bbox, const float* const* cls,
                                              const int* level_dims, const float* valid, const float* level_geom, int B, int L,
                                              int n_classes, int VX, int VY, int VZ, int nms_pre, float score_thr, float iou_thr,
                                              float* out_boxes, float* out_scores, int64_t* out_labels, int* out_count, int nmax,
                                              void* workspace, size_t workspace_bytes, mvsdet_stream_t stream) {
    const char* name = "detect_head_rotated";
    SelectParams p;
    long long points, ncap;
    if (const int rc = plan_select(name, center, bbox, cls, level_dims, valid, level_geom, out_boxes && out_scores && out_labels && out_count,
                                   B, L, n_classes, kRotMaxClasses, 65535, VX, VY, VZ, nms_pre, score_thr, &p, &points, &ncap))
        return rc;
    MVS_REQUIRE((long long)B * points < (1ll << 31) && (long long)B * n_classes * ncap < (1ll << 31),
                "%s: bad shape: %d scenes x %lld points x %d classes", name, B, points, n_classes);
    const long long caps = std::min<long long>(ncap, kLimit);
    MVS_REQUIRE(nmax >= n_classes * caps,
                "%s: Nmax=%d < %lld, the most boxes a scene can keep here (n_classes x min(candidates, %d))", name, nmax,
                n_classes * caps, kLimit);
    MVS_REQUIRE((long long)B * nmax < (1ll << 31), "%s: bad shape: %d scenes x Nmax=%d", name, B, nmax);
    if (const int rc = check_workspace(name, workspace, workspace_bytes,
                                       mvsdet_detect_rotated_workspace_bytes(B, (int)points, (int)ncap, n_classes),
                                       "mvsdet_detect_rotated_workspace_bytes"))
        return rc;
    RotWork w;
    carve_rotated(workspace, B, (int)points, (int)ncap, n_classes, &w);
    if (hipMemsetAsync(w.ccount, 0, (size_t)B * n_classes * 4, (hipStream_t)stream) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", name);
        return MVSDET_ERR_HIP;
    }
    hipLaunchKernelGGL(detect_select_kernel<true>, dim3(L, B), dim3(kSelThreads), 0, (hipStream_t)stream, p, w);
    return rotated_sort_mask_scan(w, B, iou_thr, out_boxes, out_scores, reinterpret_cast<long long*>(out_labels), nullptr, out_count,
                                  nmax, (hipStream_t)stream, name);
}

extern "C" int mvsdet_nms3d_f32(const float* boxes, const float* scores, int n, float thresh, int64_t* out_index, int* out_count,
                                void* workspace, size_t workspace_bytes, mvsdet_stream_t stream) {
    const char* name = "nms3d";
    MVS_REQUIRE(out_index && out_count, "%s: NULL pointer", name);
    MVS_REQUIRE(n >= 0, "%s: bad shape n=%d", name, n);
    MVS_REQUIRE(n <= MVSDET_DETECT_MAX_CANDIDATES, "%s: n=%d boxes above the candidate limit MVSDET_DETECT_MAX_CANDIDATES=%d", name, n,
                MVSDET_DETECT_MAX_CANDIDATES);
    MVS_REQUIRE(n == 0 || (boxes && scores), "%s: NULL pointer", name);
    if (const int rc = check_workspace(name, workspace, workspace_bytes, mvsdet_detect_rotated_workspace_bytes(1, 0, n, 1),
                                       "mvsdet_detect_rotated_workspace_bytes"))
        return rc;
    RotWork w;
    carve_rotated(workspace, 1, 0, n, 1, &w);
    hipLaunchKernelGGL(rot_load_kernel, dim3(std::max(1, (n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, boxes, scores, n, w);
    return rotated_sort_mask_scan(w, 1, thresh, nullptr, nullptr, nullptr, reinterpret_cast<long long*>(out_index), out_count,
                                  std::max(n, 1), (hipStream_t)stream, name);
}

extern "C" int mvsdet_bev_iou_rotated_f32(const float* a, int n, const float* b, int m, float* out, mvsdet_stream_t stream) {
    const char* name = "bev_iou_rotated";
    MVS_REQUIRE(n >= 0 && m >= 0 && (long long)n * m < (1ll << 31), "%s: bad shape n=%d m=%d", name, n, m);
    if ((long long)n * m == 0) return MVSDET_OK;
    MVS_REQUIRE(a && b && out, "%s: NULL pointer", name);
    const long long q = (long long)n * m;
    hipLaunchKernelGGL(rot_iou_kernel, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, n, b, m, out);
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}
