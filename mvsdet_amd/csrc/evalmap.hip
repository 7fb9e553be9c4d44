// Indoor detection metrics (mmdet3d's indoor_eval: eval_det_cls + average_precision, indoor_eval.py:8-161) on the device.
//
// State of one evaluator (one caller-owned buffer, mvsdet_eval_state_bytes): a header {records, ground-truth slots, flags, next
// scene serial}, per label the ground-truth count and the place where the label was first seen (the reference's dict order), and one
// record per detection: score, label, scene serial, row, the global slot of its best-overlapping ground-truth box and that IoU.
//
// mvsdet_eval_match_f32, two launches: eval_match_kernel, one thread per detection and per ground-truth box of the batch (a
// detection runs over the boxes of its scene with its label: the largest IoU and its FIRST index, strict >, indoor_eval.py:132-137;
// -inf without such a box), then eval_advance_kernel, one thread that moves the header on.  A record's place is the header's count
// plus the batch's counts before it, so records lie in (scene serial, row) order and no atomic decides a place.  A batch that
// would run over a capacity, a negative count and a scene serial below the header's set a flag and write nothing.
//
// mvsdet_eval_compute: keys (label : 12 | score descending, NaN last, -0 = +0 : 32 | record : 20 bits) are sorted by a bitonic
// network (2048 keys per block in LDS; one launch per step that crosses blocks), so equal scores of a label are visited by (scene
// serial, row).  The reference's walk is restated without its serial dependence: the index jmax of a detection's best box does not
// depend on the threshold and the reference never falls back to a second-best box, so a detection is a true positive at t exactly
// when iou_max > t and it has the lowest rank among the detections with the same slot and iou_max > t: an integer atomicMin per
// slot (eval_claim_kernel).  eval_ap_kernel, one block per (label, threshold): inclusive scan of the true positives over the
// label's segment, recall = tp / npos and precision = tp / (tp + fp) in float64, the precision envelope from the right and the sum
// over the positions where recall changes (the true positives; the two sentinels add 0), stored as float32.  Sums run in a fixed
// order: the same bits from run to run.
//
// The IoU is BaseInstance3DBoxes.overlaps (base_box3d.py:496-590) as a mathematical function, in float32: height overlap times the
// area of the intersection of the two footprints (extents clamped to >= 1e-4) over clamp(v1 + v2 - overlap, 1e-8).  The
// intersection is computed directly (rect_clip.h; the closed form where both headings are 0), where the reference recovers it from
// mmcv's box_iou_rotated as iou2d (a1 + a2) / (1 + iou2d): mmcv's own float32 rounding is not reproduced.
#include "common.h"
#include "rect_clip.h"

#include <climits>

namespace mvsdet {
namespace {

constexpr int kMaxRecords = MVSDET_EVAL_MAX_RECORDS;
constexpr int kMaxLabels = MVSDET_EVAL_MAX_LABELS;
constexpr int kMaxThr = MVSDET_EVAL_MAX_THRESHOLDS;
constexpr int kSortBlock = 2048;   // keys one block sorts in LDS
constexpr unsigned long long kPadKey = ~0ull;

enum { kHdrRecords = 0, kHdrSlots = 1, kHdrFlags = 2, kHdrSerial = 3, kHdrWords = 64 };

struct EvalState {
    int* hdr;
    int* npos;                    // [n_labels] ground-truth boxes of the label
    unsigned long long* first;    // [n_labels] (scene serial << 32 | ground truth << 31 | row) where the label was first seen
    float* score;
    float* iou;
    int* label;
    int* scene;
    int* row;
    int* slot;
};

__host__ __device__ inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

size_t state_bytes(int n_labels, int capacity) {
    return up256(kHdrWords * 4) + up256((size_t)n_labels * 4) + up256((size_t)n_labels * 8) + 6 * up256((size_t)capacity * 4);
}

EvalState state_of(void* buf, int n_labels, int capacity) {
    char* p = static_cast<char*>(buf);
    EvalState s;
    s.hdr = reinterpret_cast<int*>(p), p += up256(kHdrWords * 4);
    s.npos = reinterpret_cast<int*>(p), p += up256((size_t)n_labels * 4);
    s.first = reinterpret_cast<unsigned long long*>(p), p += up256((size_t)n_labels * 8);
    const size_t r = up256((size_t)capacity * 4);
    s.score = reinterpret_cast<float*>(p), p += r;
    s.iou = reinterpret_cast<float*>(p), p += r;
    s.label = reinterpret_cast<int*>(p), p += r;
    s.scene = reinterpret_cast<int*>(p), p += r;
    s.row = reinterpret_cast<int*>(p), p += r;
    s.slot = reinterpret_cast<int*>(p);
    return s;
}

struct MatchParams {
    const float* pred;
    const float* scores;
    const int64_t* labels;
    const int* counts;
    const float* gt;
    const int64_t* gt_labels;
    const int* gt_counts;
    int B, Nmax, G, scene0, n_labels, capacity, gt_capacity;
};

// IoU of two boxes (x, y, bottom z, dx, dy, dz, yaw): file header
__device__ __forceinline__ float eval_iou3d(const float* a, const float* b) {
    const float top_a = a[2] + a[5], top_b = b[2] + b[5];
    const float oh = fmaxf(fminf(top_a, top_b) - fmaxf(a[2], b[2]), 0.f);
    const float aw = fmaxf(a[3], 1e-4f), al = fmaxf(a[4], 1e-4f), bw = fmaxf(b[3], 1e-4f), bl = fmaxf(b[4], 1e-4f);
    float area;
    if (a[6] == 0.f && b[6] == 0.f) {
        const float ox = fminf(a[0] + aw / 2.f, b[0] + bw / 2.f) - fmaxf(a[0] - aw / 2.f, b[0] - bw / 2.f);
        const float oy = fminf(a[1] + al / 2.f, b[1] + bl / 2.f) - fmaxf(a[1] - al / 2.f, b[1] - bl / 2.f);
        area = fmaxf(ox, 0.f) * fmaxf(oy, 0.f);
    } else {
        area = rect_intersection_area(a[0], a[1], aw, al, a[6], b[0], b[1], bw, bl, b[6]);
    }
    const float ov = area * oh;
    const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
    return ov / fmaxf(va + vb - ov, 1e-8f);
}

// What both launches of a match call decide alike from the header and the counts: the batch's totals, the counts before scene b,
// and whether the batch is taken at all
struct BatchPlan {
    int flags, base_n, base_g, tot_n, tot_g, pre_n, pre_g;
};

__device__ __forceinline__ BatchPlan plan_batch(const EvalState& s, const MatchParams& p, int b) {
    BatchPlan q = {0, s.hdr[kHdrRecords], s.hdr[kHdrSlots], 0, 0, 0, 0};
    long long tn = 0, tg = 0;
    for (int k = 0; k < p.B; ++k) {
        const int c = p.counts[k], g = p.gt_counts[k];
        if (c < 0 || g < 0 || c > p.Nmax || g > p.G) q.flags |= MVSDET_EVAL_FLAG_BAD_COUNT;
        if (k == b) q.pre_n = (int)tn, q.pre_g = (int)tg;
        tn += c > 0 ? c : 0, tg += g > 0 ? g : 0;
    }
    if (q.base_n + tn > p.capacity) q.flags |= MVSDET_EVAL_FLAG_RECORDS_FULL;
    if (q.base_g + tg > p.gt_capacity) q.flags |= MVSDET_EVAL_FLAG_SLOTS_FULL;
    if (p.scene0 < s.hdr[kHdrSerial]) q.flags |= MVSDET_EVAL_FLAG_SERIAL;
    q.tot_n = (int)tn, q.tot_g = (int)tg;
    return q;
}

__global__ __launch_bounds__(kThreads) void eval_match_kernel(EvalState s, MatchParams p) {
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long n_det = (long long)p.B * p.Nmax, n_gt = (long long)p.B * p.G;
    if (t >= n_det && t >= n_gt) return;
    if (t < n_det) {
        const int b = (int)(t / p.Nmax), i = (int)(t % p.Nmax);
        const BatchPlan q = plan_batch(s, p, b);
        if (q.flags) return;
        if (i < p.counts[b]) {
            const long long lab64 = p.labels[(size_t)b * p.Nmax + i];
            const bool lab_ok = lab64 >= 0 && lab64 < p.n_labels;
            const int lab = lab_ok ? (int)lab64 : 0;
            float a[7];
            for (int k = 0; k < 7; ++k) a[k] = p.pred[((size_t)b * p.Nmax + i) * 7 + k];
            float best = -INFINITY;
            int jbest = -1;
            const int ng = p.gt_counts[b];
            for (int j = 0; j < ng && lab_ok; ++j) {
                if (p.gt_labels[(size_t)b * p.G + j] != lab64) continue;
                float g[7];
                for (int k = 0; k < 7; ++k) g[k] = p.gt[((size_t)b * p.G + j) * 7 + k];
                const float v = eval_iou3d(a, g);
                if (v > best) best = v, jbest = j;
            }
            const int pos = q.base_n + q.pre_n + i;   // < capacity: the plan refused the batch otherwise
            s.score[pos] = p.scores[(size_t)b * p.Nmax + i];
            s.iou[pos] = best;
            s.label[pos] = lab;
            s.scene[pos] = p.scene0 + b;
            s.row[pos] = i;
            s.slot[pos] = jbest < 0 ? -1 : q.base_g + q.pre_g + jbest;
            if (lab_ok) atomicMin(&s.first[lab], ((unsigned long long)(unsigned)(p.scene0 + b) << 32) | (unsigned)i);
            else atomicOr(&s.hdr[kHdrFlags], MVSDET_EVAL_FLAG_BAD_LABEL);
        }
    }
    if (t < n_gt) {
        const int b = (int)(t / p.G), j = (int)(t % p.G);
        const BatchPlan q = plan_batch(s, p, b);
        if (q.flags) return;
        if (j < p.gt_counts[b]) {
            const long long lab64 = p.gt_labels[(size_t)b * p.G + j];
            if (lab64 >= 0 && lab64 < p.n_labels) {
                atomicAdd(&s.npos[(int)lab64], 1);
                atomicMin(&s.first[(int)lab64], ((unsigned long long)(unsigned)(p.scene0 + b) << 32) | 0x80000000ull | (unsigned)j);
            } else {
                atomicOr(&s.hdr[kHdrFlags], MVSDET_EVAL_FLAG_BAD_LABEL);
            }
        }
    }
}

__global__ void eval_advance_kernel(EvalState s, MatchParams p) {
    const BatchPlan q = plan_batch(s, p, -1);
    if (q.flags) {
        atomicOr(&s.hdr[kHdrFlags], q.flags);
        return;
    }
    s.hdr[kHdrRecords] = q.base_n + q.tot_n;
    s.hdr[kHdrSlots] = q.base_g + q.tot_g;
    s.hdr[kHdrSerial] = p.scene0 + p.B;
}

__global__ __launch_bounds__(kThreads) void eval_reset_kernel(EvalState s, int n_labels) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t < kHdrWords) s.hdr[t] = 0;
    if (t < n_labels) s.npos[t] = 0, s.first[t] = ~0ull;
}

__global__ __launch_bounds__(kThreads) void eval_iou_kernel(const float* a, int n, const float* b, int m, float* out) {
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)n * m) return;
    float x[7], y[7];
    for (int k = 0; k < 7; ++k) x[k] = a[(t / m) * 7 + k], y[k] = b[(t % m) * 7 + k];
    out[t] = eval_iou3d(x, y);
}

// ------------------------------------------------------------------------------------------------------------ compute
struct ComputeParams {
    int n_labels, gt_capacity, n_sort, n_out, n_thr;
    float thr[kMaxThr];
    unsigned long long* keys;   // [n_sort]
    int* seg;                   // [2 * n_labels] begin, end of every label's ranks
    int* claim;                 // [n_thr * gt_capacity] lowest rank with iou_max > t that points at the slot
    int* cum;                   // [n_thr * n_sort] true positives of the label up to and including the rank
    float* out_ap;
    double* out_recall;
    int* out_npos;
    int* out_ndet;
    long long* out_first;
    unsigned char* out_tp;      // [n_thr * n_out]
    int* out_order;             // [n_out]
    int* out_info;              // [4] records, slots, flags, next serial
};

__device__ __forceinline__ int records_of(const EvalState& s, const ComputeParams& p) { return min(s.hdr[kHdrRecords], p.n_out); }

// score descending, NaN last (np.argsort(-confidence)), -0 equal to +0
__device__ __forceinline__ unsigned score_key(float v) {
    if (v != v) return 0xffffffffu;
    if (v == 0.f) v = 0.f;
    const unsigned f = __float_as_uint(v);
    const unsigned asc = (f & 0x80000000u) ? ~f : (f | 0x80000000u);   // +inf: 0xff800000, below every NaN pattern's image
    return ~asc;                                                       // -inf: 0xff7fffff < 0xffffffff
}

__global__ __launch_bounds__(kThreads) void eval_keys_kernel(EvalState s, ComputeParams p) {
    const int n = records_of(s, p);
    const int stride = gridDim.x * kThreads, t = blockIdx.x * kThreads + threadIdx.x;
    for (int r = t; r < p.n_sort; r += stride)
        p.keys[r] = r < n ? ((unsigned long long)s.label[r] << 52) | ((unsigned long long)score_key(s.score[r]) << 20) | (unsigned)r
                          : kPadKey;
    for (int k = t; k < p.n_thr * p.gt_capacity; k += stride) p.claim[k] = INT_MAX;
    for (int k = t; k < 2 * p.n_labels; k += stride) p.seg[k] = 0;
}

__device__ __forceinline__ void compare_exchange(unsigned long long& a, unsigned long long& b, bool ascending) {
    if ((a > b) == ascending) {
        const unsigned long long t = a;
        a = b, b = t;
    }
}

// Steps j = j_top .. 1 of the bitonic stages k = k_lo .. k_hi (powers of two) on the block's kSortBlock keys in LDS
__global__ __launch_bounds__(kThreads) void eval_sort_local_kernel(unsigned long long* keys, int k_lo, int k_hi) {
    __shared__ unsigned long long sk[kSortBlock];
    const int base = blockIdx.x * kSortBlock;
    for (int i = threadIdx.x; i < kSortBlock; i += kThreads) sk[i] = keys[base + i];
    __syncthreads();
    for (long long k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = (int)(k < kSortBlock ? k : kSortBlock) >> 1; j > 0; j >>= 1) {
            for (int q = threadIdx.x; q < kSortBlock / 2; q += kThreads) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                compare_exchange(sk[i], sk[i | j], ((long long)(base + i) & k) == 0);
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < kSortBlock; i += kThreads) keys[base + i] = sk[i];
}

// One step (k, j), j >= kSortBlock: the partners lie in different blocks' ranges
__global__ __launch_bounds__(kThreads) void eval_sort_step_kernel(unsigned long long* keys, int n_sort, long long k, int j) {
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= n_sort / 2) return;
    const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
    unsigned long long a = keys[i], b = keys[i | j];
    const unsigned long long a0 = a;
    compare_exchange(a, b, ((long long)i & k) == 0);
    if (a != a0) keys[i] = a, keys[i | j] = b;
}

__global__ __launch_bounds__(kThreads) void eval_claim_kernel(EvalState s, ComputeParams p) {
    const int n = records_of(s, p);
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n) return;
    const unsigned long long key = p.keys[r];
    const int lab = (int)(key >> 52), idx = (int)(key & 0xfffffu);
    if (r == 0 || (int)(p.keys[r - 1] >> 52) != lab) p.seg[2 * lab] = r;
    if (r == n - 1 || (int)(p.keys[r + 1] >> 52) != lab) p.seg[2 * lab + 1] = r + 1;
    p.out_order[r] = idx;
    const float v = s.iou[idx];
    const int slot = s.slot[idx];
    if (slot < 0 || slot >= p.gt_capacity) return;
    for (int t = 0; t < p.n_thr; ++t)
        if (v > p.thr[t]) atomicMin(&p.claim[(size_t)t * p.gt_capacity + slot], r);
}

// Inclusive scans over the block's 256 threads in thread order (wave shuffles, then the four wave totals through LDS)
__device__ __forceinline__ int block_scan_sum(int v, int* part, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    __syncthreads();
    if (lane == 63) part[wave] = v;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += part[w];
    total = part[0] + part[1] + part[2] + part[3];
    return v + before;
}

__device__ __forceinline__ double block_scan_max(double v, double* part, double& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, d, 64);
        if (lane >= d) v = fmax(v, o);
    }
    __syncthreads();
    if (lane == 63) part[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) v = fmax(v, part[w]);
    total = fmax(fmax(part[0], part[1]), fmax(part[2], part[3]));
    return v;
}

// Sum over the block in a fixed tree order
__device__ __forceinline__ double block_sum_f64(double v, double* buf) {
    __syncthreads();
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) buf[threadIdx.x] += buf[threadIdx.x + d];
        __syncthreads();
    }
    return buf[0];
}

__global__ __launch_bounds__(kThreads) void eval_ap_kernel(EvalState s, ComputeParams p) {
    __shared__ int part_i[4];
    __shared__ double part_d[4];
    __shared__ double buf[kThreads];
    const int lab = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int n = records_of(s, p);
    const int b = p.seg[2 * lab], e = p.seg[2 * lab + 1];
    const int ndet = e - b, npos = s.npos[lab];
    const float thr = p.thr[t];
    int* cum = p.cum + (size_t)t * p.n_sort;
    // forward: true positives and their running count
    int carry = 0;
    for (int c = b; c < e; c += kThreads) {
        const int r = c + tid;
        int flag = 0;
        if (r < e) {
            const int idx = (int)(p.keys[r] & 0xfffffu);
            const int slot = s.slot[idx];
            flag = s.iou[idx] > thr && slot >= 0 && slot < p.gt_capacity && p.claim[(size_t)t * p.gt_capacity + slot] == r;
            p.out_tp[(size_t)t * p.n_out + r] = (unsigned char)flag;
        }
        int total;
        const int inc = block_scan_sum(flag, part_i, total);
        if (r < e) cum[r] = carry + inc;
        carry += total;
    }
    __syncthreads();   // cum[] of this block's segment is read back by other threads below
    // backward: the precision envelope from the right and the area under it
    double env_carry = 0.0, sum = 0.0;
    const double dpos = (double)npos;
    for (int c = e; c > b; c -= kThreads) {
        const int r = c - 1 - tid;
        double prec = 0.0;
        int k = 0, k_prev = 0;
        if (r >= b) {
            k = cum[r];
            k_prev = r > b ? cum[r - 1] : 0;
            prec = (double)k / (double)(r - b + 1);   // tp + fp = r - b + 1 >= 1: the reference's eps floor never binds
        }
        double top;
        const double env = fmax(env_carry, block_scan_max(prec, part_d, top));
        const double term = (r >= b && k != k_prev) ? ((double)k / dpos - (double)k_prev / dpos) * env : 0.0;
        sum += block_sum_f64(term, buf);
        env_carry = fmax(env_carry, top);
    }
    if (tid == 0) {
        // a label that is predicted but has no ground truth anywhere: recall = 0 / 0, and the reference's AP is NaN with it
        const bool undefined = ndet > 0 && npos == 0;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        p.out_ap[t * p.n_labels + lab] = undefined ? (float)nan : (float)sum;
        p.out_recall[t * p.n_labels + lab] = undefined ? nan : ndet > 0 ? (double)carry / dpos : 0.0;
        if (t == 0) {
            p.out_npos[lab] = npos;
            p.out_ndet[lab] = ndet;
            p.out_first[lab] = (long long)s.first[lab];
            if (lab == 0) {
                p.out_info[0] = s.hdr[kHdrRecords], p.out_info[1] = s.hdr[kHdrSlots];
                p.out_info[2] = s.hdr[kHdrFlags] | (s.hdr[kHdrRecords] > n ? MVSDET_EVAL_FLAG_BOUND : 0);
                p.out_info[3] = s.hdr[kHdrSerial];
            }
        }
    }
}

int sort_size(int n_bound) {
    int n = kSortBlock;
    while (n < n_bound) n <<= 1;
    return n;
}

struct WsLayout {
    size_t keys, seg, claim, cum, total;
};

WsLayout ws_layout(int n_labels, int n_bound, int gt_capacity, int n_thr) {
    const size_t ns = (size_t)sort_size(n_bound);
    WsLayout w;
    w.keys = 0;
    w.seg = w.keys + up256(ns * 8);
    w.claim = w.seg + up256((size_t)2 * n_labels * 4);
    w.cum = w.claim + up256((size_t)n_thr * gt_capacity * 4);
    w.total = w.cum + up256((size_t)n_thr * ns * 4);
    return w;
}

bool sizes_ok(int n_labels, int capacity, int gt_capacity) {
    return n_labels > 0 && n_labels <= kMaxLabels && capacity > 0 && capacity <= kMaxRecords && gt_capacity > 0 &&
           gt_capacity <= (1 << 24);
}

}  // namespace
}  // namespace mvsdet

using namespace mvsdet;

extern "C" size_t mvsdet_eval_state_bytes(int n_labels, int capacity, int gt_capacity) {
    return sizes_ok(n_labels, capacity, gt_capacity) ? state_bytes(n_labels, capacity) : 0;
}

extern "C" size_t mvsdet_eval_workspace_bytes(int n_labels, int n_bound, int gt_capacity, int n_thr) {
    if (!sizes_ok(n_labels, 1, gt_capacity) || n_bound < 0 || n_bound > kMaxRecords || n_thr < 1 || n_thr > kMaxThr) return 0;
    return ws_layout(n_labels, n_bound, gt_capacity, n_thr).total;
}

extern "C" int mvsdet_eval_reset(void* state, size_t state_bytes_given, int n_labels, int capacity, int gt_capacity,
                                 mvsdet_stream_t stream) {
    MVS_REQUIRE(state, "eval_reset: NULL pointer");
    MVS_REQUIRE(sizes_ok(n_labels, capacity, gt_capacity),
                "eval_reset: bad sizes n_labels=%d (1..%d) capacity=%d (1..%d) gt_capacity=%d", n_labels, kMaxLabels, capacity,
                kMaxRecords, gt_capacity);
    MVS_REQUIRE((uintptr_t)state % 8 == 0, "eval_reset: state must be 8-byte aligned");
    if (state_bytes_given < state_bytes(n_labels, capacity)) {
        set_error("eval_reset: state of %zu bytes, %zu needed", state_bytes_given, state_bytes(n_labels, capacity));
        return MVSDET_ERR_WORKSPACE;
    }
    const EvalState s = state_of(state, n_labels, capacity);
    const int grid = (std::max(n_labels, (int)kHdrWords) + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(eval_reset_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, s, n_labels);
    MVS_LAUNCH_CHECK("eval_reset");
    return MVSDET_OK;
}

extern "C" int mvsdet_eval_match_f32(void* state, int n_labels, int capacity, int gt_capacity, const float* pred, const float* scores,
                                     const int64_t* labels, const int* counts, int B, int Nmax, const float* gt,
                                     const int64_t* gt_labels, const int* gt_counts, int G, int scene0, mvsdet_stream_t stream) {
    MVS_REQUIRE(state, "eval_match: NULL pointer (state)");
    MVS_REQUIRE(sizes_ok(n_labels, capacity, gt_capacity),
                "eval_match: bad sizes n_labels=%d (1..%d) capacity=%d (1..%d) gt_capacity=%d", n_labels, kMaxLabels, capacity,
                kMaxRecords, gt_capacity);
    MVS_REQUIRE(B >= 0 && Nmax >= 0 && G >= 0 && scene0 >= 0 && (long long)scene0 + B <= INT32_MAX,
                "eval_match: bad shape B=%d Nmax=%d G=%d scene0=%d", B, Nmax, G, scene0);
    MVS_REQUIRE((long long)B * Nmax <= INT32_MAX && (long long)B * G <= INT32_MAX, "eval_match: batch too large");
    if (B == 0) return MVSDET_OK;
    MVS_REQUIRE(counts && gt_counts, "eval_match: NULL pointer (counts)");
    MVS_REQUIRE(Nmax == 0 || (pred && scores && labels), "eval_match: NULL pointer (predictions)");
    MVS_REQUIRE(G == 0 || (gt && gt_labels), "eval_match: NULL pointer (ground truth)");
    const EvalState s = state_of(state, n_labels, capacity);
    const MatchParams p = {pred, scores, labels, counts, gt, gt_labels, gt_counts, B, Nmax, G, scene0, n_labels, capacity, gt_capacity};
    const long long work = std::max((long long)B * Nmax, (long long)B * G);
    if (work > 0)
        hipLaunchKernelGGL(eval_match_kernel, dim3((unsigned)((work + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                           s, p);
    hipLaunchKernelGGL(eval_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, s, p);
    MVS_LAUNCH_CHECK("eval_match");
    return MVSDET_OK;
}

extern "C" int mvsdet_eval_iou_f32(const float* a, int n, const float* b, int m, float* out, mvsdet_stream_t stream) {
    MVS_REQUIRE(n >= 0 && m >= 0 && (long long)n * m <= INT32_MAX, "eval_iou: bad shape n=%d m=%d", n, m);
    if (n == 0 || m == 0) return MVSDET_OK;
    MVS_REQUIRE(a && b && out, "eval_iou: NULL pointer");
    const long long work = (long long)n * m;
    hipLaunchKernelGGL(eval_iou_kernel, dim3((unsigned)((work + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, a, n,
                       b, m, out);
    MVS_LAUNCH_CHECK("eval_iou");
    return MVSDET_OK;
}

extern "C" int mvsdet_eval_compute(const void* state, int n_labels, int capacity, int gt_capacity, int n_bound, const float* thresholds,
                                   int n_thr, float* out_ap, double* out_recall, int* out_npos, int* out_ndet, int64_t* out_first,
                                   unsigned char* out_tp, int* out_order, int* out_info, void* workspace, size_t workspace_bytes,
                                   mvsdet_stream_t stream) {
    MVS_REQUIRE(state && thresholds && out_ap && out_recall && out_npos && out_ndet && out_first && out_info && workspace,
                "eval_compute: NULL pointer");
    MVS_REQUIRE(sizes_ok(n_labels, capacity, gt_capacity),
                "eval_compute: bad sizes n_labels=%d (1..%d) capacity=%d (1..%d) gt_capacity=%d", n_labels, kMaxLabels, capacity,
                kMaxRecords, gt_capacity);
    MVS_REQUIRE(n_bound >= 0 && n_bound <= capacity, "eval_compute: n_bound=%d outside [0, capacity=%d]", n_bound, capacity);
    MVS_REQUIRE(n_thr >= 1 && n_thr <= kMaxThr, "eval_compute: %d thresholds (1..%d)", n_thr, kMaxThr);
    MVS_REQUIRE(n_bound == 0 || (out_tp && out_order), "eval_compute: NULL pointer (flags, order)");
    MVS_REQUIRE((uintptr_t)workspace % 8 == 0 && (uintptr_t)out_recall % 8 == 0 && (uintptr_t)out_first % 8 == 0,
                "eval_compute: workspace, out_recall and out_first must be 8-byte aligned");
    const WsLayout w = ws_layout(n_labels, n_bound, gt_capacity, n_thr);
    MVS_REQUIRE_WORKSPACE("eval_compute", workspace_bytes, w.total);
    const EvalState s = state_of(const_cast<void*>(state), n_labels, capacity);
    char* ws = static_cast<char*>(workspace);
    ComputeParams p;
    p.n_labels = n_labels, p.gt_capacity = gt_capacity, p.n_sort = sort_size(n_bound), p.n_out = n_bound, p.n_thr = n_thr;
    for (int t = 0; t < kMaxThr; ++t) p.thr[t] = t < n_thr ? thresholds[t] : 0.f;
    p.keys = reinterpret_cast<unsigned long long*>(ws + w.keys);
    p.seg = reinterpret_cast<int*>(ws + w.seg);
    p.claim = reinterpret_cast<int*>(ws + w.claim);
    p.cum = reinterpret_cast<int*>(ws + w.cum);
    p.out_ap = out_ap, p.out_recall = out_recall, p.out_npos = out_npos, p.out_ndet = out_ndet;
    p.out_first = reinterpret_cast<long long*>(out_first), p.out_tp = out_tp, p.out_order = out_order, p.out_info = out_info;
    hipStream_t st = (hipStream_t)stream;
    const size_t init = std::max((size_t)p.n_sort, std::max((size_t)n_thr * gt_capacity, (size_t)2 * n_labels));
    hipLaunchKernelGGL(eval_keys_kernel, dim3((unsigned)std::min<size_t>((init + kThreads - 1) / kThreads, 4096)), dim3(kThreads), 0, st,
                       s, p);
    if (n_bound > 0) {
        const int blocks = p.n_sort / kSortBlock;
        hipLaunchKernelGGL(eval_sort_local_kernel, dim3(blocks), dim3(kThreads), 0, st, p.keys, 2, kSortBlock);
        for (long long k = 2ll * kSortBlock; k <= p.n_sort; k <<= 1) {
            for (int j = (int)(k >> 1); j >= kSortBlock; j >>= 1)
                hipLaunchKernelGGL(eval_sort_step_kernel, dim3(p.n_sort / 2 / kThreads), dim3(kThreads), 0, st, p.keys, p.n_sort, k, j);
            hipLaunchKernelGGL(eval_sort_local_kernel, dim3(blocks), dim3(kThreads), 0, st, p.keys, (int)k, (int)k);
        }
        hipLaunchKernelGGL(eval_claim_kernel, dim3((n_bound + kThreads - 1) / kThreads), dim3(kThreads), 0, st, s, p);
    }
    hipLaunchKernelGGL(eval_ap_kernel, dim3(n_labels, n_thr), dim3(kThreads), 0, st, s, p);
    MVS_LAUNCH_CHECK("eval_compute");
    return MVSDET_OK;
}
