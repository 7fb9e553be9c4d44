// Stage 2 of the MVSDet hot path on gfx950: depth probability (softmax over planes), offset sigmoid,
// top-k plane selection and depth expectation, fused.  Reference: mvsdet.py:470-475, :266-283
// (sample_depth_prob), :298-317 (compute_avg_depth) of Pixie8888/MVSDet.
//
// Roofline: HBM.  Algorithmic bytes per scene: read 2*N*D*H*W*4, write N*(2D+3*topk+1)*H*W*4 (0.82 GB at the headline shape).
// One thread per pixel, lanes along W so every plane access is a coalesced 256-byte run.  DREG > 0 (D <= DREG, DREG =
// 16 / 64): the D cost logits, then their exponentials, stay in registers -- every input is read once, one expf per
// plane instead of two, and all loads of a pass are in flight together.  DREG = 0 (D up to 512): the logits are re-read
// from L2 in the second / third pass.  Same operations in the same order either way.
//
// gfx950 retires loads and stores through ONE in-order vmcnt, so a load requested behind a store cannot be waited for without
// waiting for that store, and under a write stream a store is acknowledged thousands of cycles after it was issued.
// depth_prob_topk_ahead_kernel therefore requests what a pixel reads before it stores anything.  What bounds it then is its
// bytes: 0.165 ms at the headline shape against 0.138 ms for the same bytes at the packing kernel's rate, and about 0.12 ms of
// vector issue (docs/KERNEL_NOTES.md 4.2, profiles/r09_depth_prob_ab.txt).
#include "common.h"

namespace mvsdet {

// One plane's share of the depth expectation and its place in the sorted (descending) candidate list of a pixel; strict '>'
// keeps the lower plane on ties.  kNanAware: single planes can be NaN (ready-made probabilities) and rank above every number.
template <int KT, bool kNanAware>
__device__ __forceinline__ void take_plane(int d, float pd, float od, float near, float interval, float& avg, float (&bv)[KT],
                                           float (&bo)[KT], int (&bi)[KT]) {
    // mvsdet.py:278-282  depth = idx*interval + near + off*interval (each op rounded)
    const float dep = ((float)d * interval + near) + od * interval;
    avg = avg + dep * pd;
    float cv = pd, co = od;
    int cidx = d;
    // once the new plane is in, every entry below moves down one slot: a displaced entry is compared with nothing, or
    // an equal value further down (a lower plane) would overtake it
    bool moved = false;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const bool gt = kNanAware ? (moved || cv > bv[k] || (cv != cv && bv[k] == bv[k])) : (moved || cv > bv[k]);
        moved = gt;
        const float tv = bv[k], to = bo[k];
        const int ti = bi[k];
        bv[k] = gt ? cv : tv;
        bo[k] = gt ? co : to;
        bi[k] = gt ? cidx : ti;
        cv = gt ? tv : cv;
        co = gt ? to : co;
        cidx = gt ? ti : cidx;
    }
}

template <int KT>
__device__ __forceinline__ void write_candidates(const float (&bv)[KT], const float (&bo)[KT], const int (&bi)[KT],
                                                 float* __restrict__ est_depth, float* __restrict__ est_dens,
                                                 int32_t* __restrict__ est_idx, int n, int pix, int HW, int topk, float near,
                                                 float interval) {
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        if (k < topk) {
            const size_t oi = ((size_t)n * topk + k) * HW + pix;
            est_depth[oi] = ((float)bi[k] * interval + near) + bo[k] * interval;
            est_dens[oi] = bv[k];
            if (est_idx) est_idx[oi] = bi[k];
        }
    }
}

// KT = length of the candidate list kept per pixel (3 for the reference's topk = 3, MVSDET_MAX_TOPK otherwise): the
// insertion is 7 VALU instructions per entry and plane.  This kernel (option "depthprob_ahead" 0, and sample_depth_prob) requests the
// offset logit of plane d + 1 behind the two stores of plane d and so pays one store round trip per plane.
//
// Non-finite inputs follow torch.topk, which ranks NaN above every number: descending value, NaN
// first, the lower plane first among equals and among NaNs.  From logits, one NaN / +Inf logit (or all -Inf) makes the
// normaliser and with it every probability of the pixel NaN, so the ranking is planes 0 .. topk-1: one test of the
// normaliser after the loop, nothing per plane.  From ready-made probabilities (sample_depth_prob) single planes can be
// NaN, and the insertion itself compares NaN-aware.
template <bool kFromLogits, int DREG, int KT>
__global__ __launch_bounds__(kThreads) void depth_prob_topk_kernel(
    const float* __restrict__ cost_reg, const float* __restrict__ off_logit, float* __restrict__ prob,
    float* __restrict__ off, float* __restrict__ est_depth, float* __restrict__ est_dens,
    int32_t* __restrict__ est_idx, float* __restrict__ avg_depth, int D, int HW, int topk, float near, float interval,
    size_t in_view_stride) {
    const int pix = blockIdx.x * kThreads + threadIdx.x;
    const int n = blockIdx.y;
    if (pix >= HW) return;
    const size_t base = (size_t)n * D * HW + pix;
    // the two inputs may be the channel slices of one (N, 2, D, H, W) tensor (the network's output, mvsdet.py:469): a view
    // is in_view_stride floats after the previous one, its (D, H, W) block dense
    const float* c = cost_reg + (size_t)n * in_view_stride + pix;
    const float* o = off_logit + (size_t)n * in_view_stride + pix;

    constexpr int kReg = DREG > 0 ? DREG : 1;
    float e[kReg];   // logits, then exp(logit - max)
    float m = 0.0f, s = 1.0f;
    if (kFromLogits) {
        if (DREG > 0) {
#pragma unroll
            for (int d = 0; d < DREG; ++d) e[d] = d < D ? c[(size_t)d * HW] : 0.0f;
            m = e[0];
#pragma unroll
            for (int d = 1; d < DREG; ++d)
                if (d < D) m = e[d] > m ? e[d] : m;
            s = 0.0f;
#pragma unroll
            for (int d = 0; d < DREG; ++d)
                if (d < D) {
                    e[d] = expf(e[d] - m);
                    s += e[d];
                }
        } else {
            m = c[0];
#pragma unroll 4
            for (int d = 1; d < D; ++d) {
                const float v = c[(size_t)d * HW];
                m = v > m ? v : m;
            }
            s = 0.0f;
#pragma unroll 4
            for (int d = 0; d < D; ++d) s += expf(c[(size_t)d * HW] - m);
        }
    }

    // sorted (descending) candidate list in registers; strict '>' keeps the lower plane on ties
    float bv[KT], bo[KT];
    int bi[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        bv[k] = -1.0f;
        bo[k] = 0.0f;
        bi[k] = 0;
    }
    float avg = 0.0f;
    auto plane = [&](int d, float ed) {
        float pd, od;
        if (kFromLogits) {
            pd = (DREG > 0 ? ed : expf(c[(size_t)d * HW] - m)) / s;
            od = 1.0f / (1.0f + expf(-o[(size_t)d * HW]));
            prob[base + (size_t)d * HW] = pd;
            off[base + (size_t)d * HW] = od;
        } else {  // inputs already are prob / off (a6+a7 only)
            pd = c[(size_t)d * HW];
            od = o[(size_t)d * HW];
        }
        take_plane<KT, !kFromLogits>(d, pd, od, near, interval, avg, bv, bo, bi);
    };
    if (kFromLogits && DREG > 0) {
#pragma unroll
        for (int d = 0; d < DREG; ++d)
            if (d < D) plane(d, e[d]);
    } else {
#pragma unroll 4
        for (int d = 0; d < D; ++d) plane(d, 0.0f);
    }
    avg_depth[(size_t)n * HW + pix] = avg;
    if (kFromLogits && s != s) {
        // every probability is NaN and none was inserted (NaN > x is false): all planes tie as NaN, the lowest come first
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < topk) {   // topk <= D: plane k exists, and this thread wrote its offset above
                bv[k] = s;
                bo[k] = off[base + (size_t)k * HW];
                bi[k] = k;
            }
    }
    write_candidates<KT>(bv, bo, bi, est_depth, est_dens, est_idx, n, pix, HW, topk, near, interval);
}

// The same pixel in the same operations (option "depthprob_ahead" 1, the default): every output has the bits of the kernel above.
// What differs is when memory is asked.  DREG > 0: all 2 * D inputs of a pixel are requested, and the D sigmoids formed, before
// the first store; from there to the end of the kernel a thread only computes and stores -- no load, no wait on vmcnt.  The
// offsets stay in registers (logits, then sigmoids), and the NaN tail takes its offsets from there instead of reading off[]
// back.  DREG = 0 (D > 64): the third pass runs kChunk planes ahead -- both inputs of chunk k + 1 are requested before the
// stores of chunk k, so the wait for them covers no store younger than chunk k - 1's.  kFull: D == DREG, no plane is tested
// for being there (at D = 64 the 64 tests' masks alone overflow the scalar registers).
constexpr int kChunk = 8;
// A block-uniform pointer the optimiser cannot look into: left alone it folds the thread's index into the base and then adds every
// plane's offset in 64-bit vector arithmetic, one register pair per address.
template <typename T>
__device__ __forceinline__ __attribute__((address_space(1))) T* plane_ptr(T* p) {
    asm("" : "+s"(p));
    return (__attribute__((address_space(1))) T*)p;   // global memory: what the optimiser knew of p before
}
template <int DREG, int KT, bool kFull>
__global__ __launch_bounds__(kThreads) void depth_prob_topk_ahead_kernel(
    const float* __restrict__ cost_reg, const float* __restrict__ off_logit, float* __restrict__ prob,
    float* __restrict__ off, float* __restrict__ est_depth, float* __restrict__ est_dens,
    int32_t* __restrict__ est_idx, float* __restrict__ avg_depth, int D, int HW, int topk, float near, float interval,
    size_t in_view_stride) {
    const int pix = blockIdx.x * kThreads + threadIdx.x;
    const int n = blockIdx.y;
    if (pix >= HW) return;
    // every address is a block-uniform pointer (scalar registers, scalar arithmetic) plus the thread's index in the block
    const int t = threadIdx.x;
    const size_t blk = (size_t)blockIdx.x * kThreads;
    const float* c = cost_reg + (size_t)n * in_view_stride + blk;
    const float* o = off_logit + (size_t)n * in_view_stride + blk;
    float* p_out = prob + (size_t)n * D * HW + blk;
    float* o_out = off + (size_t)n * D * HW + blk;

    float bv[KT], bo[KT], fo[KT];   // fo: the offsets of planes 0 .. KT-1, for the NaN tail
    int bi[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        bv[k] = -1.0f;
        bo[k] = 0.0f;
        fo[k] = 0.0f;
        bi[k] = 0;
    }
    float avg = 0.0f, m, s = 0.0f;
    if constexpr (DREG > 0) {
        float e[DREG];   // cost logits, then exp(logit - max)
        float q[DREG];   // offset logits, then their sigmoids
#pragma unroll
        for (int d = 0; d < DREG; ++d) e[d] = kFull || d < D ? plane_ptr(c + (size_t)d * HW)[t] : 0.0f;
#pragma unroll
        for (int d = 0; d < DREG; ++d) q[d] = kFull || d < D ? plane_ptr(o + (size_t)d * HW)[t] : 0.0f;
        __builtin_amdgcn_sched_barrier(0);   // the scheduler sinks the requests back to their uses otherwise
        m = e[0];
#pragma unroll
        for (int d = 1; d < DREG; ++d)
            if (kFull || d < D) m = e[d] > m ? e[d] : m;
#pragma unroll
        for (int d = 0; d < DREG; ++d)
            if (kFull || d < D) {
                e[d] = expf(e[d] - m);
                s += e[d];
                if (d % 4 == 3) __builtin_amdgcn_sched_barrier(0);   // four planes at a time: 64 at once cost more registers than there are
            }
#pragma unroll
        for (int d = 0; d < DREG; ++d)
            if (kFull || d < D) {
                q[d] = 1.0f / (1.0f + expf(-q[d]));
                asm volatile("" : "+v"(q[d]));   // formed here, not next to the stores of its plane
                if (d % 4 == 3) __builtin_amdgcn_sched_barrier(0);
            }
        __builtin_amdgcn_sched_barrier(0);   // every input has been used: nothing below waits for memory
#pragma unroll
        for (int d = 0; d < DREG; ++d)
            if (kFull || d < D) {
                const float pd = e[d] / s;
                plane_ptr(p_out + (size_t)d * HW)[t] = pd;
                plane_ptr(o_out + (size_t)d * HW)[t] = q[d];
                take_plane<KT, false>(d, pd, q[d], near, interval, avg, bv, bo, bi);
                // a plane is finished before the next begins: with no test between the planes the optimiser otherwise puts off the
                // expectation and the last candidate of every plane to the end, and keeps what they need until then
                asm volatile("" : "+v"(avg));
#pragma unroll
                for (int k = 0; k < KT; ++k) asm volatile("" : "+v"(bv[k]), "+v"(bo[k]), "+v"(bi[k]));
            }
#pragma unroll
        for (int k = 0; k < KT; ++k) fo[k] = q[k < DREG ? k : 0];
    } else {
        const float* ct = c + t;
        m = ct[0];
#pragma unroll 4
        for (int d = 1; d < D; ++d) {
            const float v = ct[(size_t)d * HW];
            m = v > m ? v : m;
        }
#pragma unroll 4
        for (int d = 0; d < D; ++d) s += expf(ct[(size_t)d * HW] - m);

        float cc[kChunk], oc[kChunk], cn[kChunk], on[kChunk];   // the chunk at hand, the chunk requested
        // a chunk that reaches past D repeats plane D - 1: every request stays inside the view, none is tested plane by plane
        auto request = [&](int d0) {
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                const size_t at = (size_t)min(d0 + j, D - 1) * HW;
                cn[j] = plane_ptr(c + at)[t];
                on[j] = plane_ptr(o + at)[t];
            }
        };
        auto finish = [&](int d, int j) {
            const float pd = expf(cc[j] - m) / s;
            const float od = 1.0f / (1.0f + expf(-oc[j]));
            plane_ptr(p_out + (size_t)d * HW)[t] = pd;
            plane_ptr(o_out + (size_t)d * HW)[t] = od;
            if (j < KT) fo[j < KT ? j : 0] = d == j ? od : fo[j < KT ? j : 0];   // planes 0 .. KT-1 are in the first chunk
            take_plane<KT, false>(d, pd, od, near, interval, avg, bv, bo, bi);
        };
        request(0);
        int d0 = 0;
        for (; d0 + kChunk <= D; d0 += kChunk) {
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                cc[j] = cn[j];
                oc[j] = on[j];
            }
            if (d0 + kChunk < D) request(d0 + kChunk);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < kChunk; ++j) finish(d0 + j, j);
        }
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
            if (d0 + j < D) {
                cc[j] = cn[j];
                oc[j] = on[j];
                finish(d0 + j, j);
            }
    }
    avg_depth[(size_t)n * HW + pix] = avg;
    if (s != s) {
        // every probability is NaN and none was inserted (NaN > x is false): all planes tie as NaN, the lowest come first
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < topk) {   // topk <= D: plane k exists
                bv[k] = s;
                bo[k] = fo[k];
                bi[k] = k;
            }
    }
    write_candidates<KT>(bv, bo, bi, est_depth, est_dens, est_idx, n, pix, HW, topk, near, interval);
}

// backward: dL/dcost = p * (gp - sum_d gp_d p_d), dL/doff_logit = go * off * (1 - off), where gp / go
// collect the gradients that reach prob / off through prob itself, the top-k densities and depths and
// the depth expectation.
__global__ __launch_bounds__(kThreads) void depth_prob_topk_bwd_kernel(
    const float* __restrict__ prob, const float* __restrict__ off, const int32_t* __restrict__ est_idx,
    const float* __restrict__ g_prob, const float* __restrict__ g_depth, const float* __restrict__ g_dens,
    const float* __restrict__ g_avg, float* __restrict__ g_cost, float* __restrict__ g_offlogit, int D, int HW, int topk,
    float near, float interval) {
    const int pix = blockIdx.x * kThreads + threadIdx.x;
    const int n = blockIdx.y;
    if (pix >= HW) return;
    const size_t base = (size_t)n * D * HW + pix;
    const float ga = g_avg ? g_avg[(size_t)n * HW + pix] : 0.0f;
    int ki[MVSDET_MAX_TOPK];
    float kd[MVSDET_MAX_TOPK], kz[MVSDET_MAX_TOPK];
#pragma unroll
    for (int k = 0; k < MVSDET_MAX_TOPK; ++k) {
        ki[k] = -1;
        kd[k] = 0.0f;
        kz[k] = 0.0f;
        if (k < topk) {
            const size_t oi = ((size_t)n * topk + k) * HW + pix;
            ki[k] = est_idx[oi];
            kd[k] = g_dens ? g_dens[oi] : 0.0f;
            kz[k] = g_depth ? g_depth[oi] : 0.0f;
        }
    }
    // pass 1: dot = sum_d gp_d * p_d
    float dot = 0.0f;
    for (int d = 0; d < D; ++d) {
        const float p = prob[base + (size_t)d * HW];
        const float od = off[base + (size_t)d * HW];
        float gp = g_prob ? g_prob[base + (size_t)d * HW] : 0.0f;
        gp += ga * (((float)d * interval + near) + od * interval);
#pragma unroll
        for (int k = 0; k < MVSDET_MAX_TOPK; ++k) gp += (ki[k] == d) ? kd[k] : 0.0f;
        dot += gp * p;
    }
    for (int d = 0; d < D; ++d) {
        const float p = prob[base + (size_t)d * HW];
        const float od = off[base + (size_t)d * HW];
        float gp = g_prob ? g_prob[base + (size_t)d * HW] : 0.0f;
        gp += ga * (((float)d * interval + near) + od * interval);
        float go = ga * p * interval;
#pragma unroll
        for (int k = 0; k < MVSDET_MAX_TOPK; ++k) {
            gp += (ki[k] == d) ? kd[k] : 0.0f;
            go += (ki[k] == d) ? kz[k] * interval : 0.0f;
        }
        g_cost[base + (size_t)d * HW] = p * (gp - dot);
        g_offlogit[base + (size_t)d * HW] = go * od * (1.0f - od);
    }
}

}  // namespace mvsdet

using namespace mvsdet;

static int check_stage2(const char* name, int N, int D, int H, int W, int topk) {
    MVS_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "%s: bad shape N=%d D=%d H=%d W=%d", name, N, D, H, W);
    MVS_REQUIRE(N <= 65535, "%s: N > 65535", name);
    MVS_REQUIRE(D <= MVSDET_MAX_DEPTH, "%s: D=%d > %d", name, D, MVSDET_MAX_DEPTH);
    MVS_REQUIRE(topk >= 1 && topk <= MVSDET_MAX_TOPK && topk <= D, "%s: topk=%d outside [1,min(%d,D)]", name, topk,
                MVSDET_MAX_TOPK);
    MVS_REQUIRE((size_t)H * W < (size_t)INT32_MAX, "%s: H*W too large", name);
    return MVSDET_OK;
}

extern "C" int mvsdet_depth_prob_topk_strided_f32(const float* cost_reg, const float* off_logit, long long view_stride,
                                                  float* prob, float* off, float* est_depth, float* est_dens,
                                                  int32_t* est_idx, float* avg_depth, int N, int D, int H, int W, int topk,
                                                  float near, float interval, mvsdet_stream_t stream) {
    MVS_REQUIRE(cost_reg && off_logit && prob && off && est_depth && est_dens && avg_depth, "depth_prob_topk: NULL pointer");
    if (int rc = check_stage2("depth_prob_topk", N, D, H, W, topk)) return rc;
    MVS_REQUIRE(view_stride >= (long long)D * H * W, "depth_prob_topk: view stride %lld < D*H*W", view_stride);
    const int HW = H * W;
    dim3 grid((HW + kThreads - 1) / kThreads, N);
#define MVS_DP_LAUNCH(KERNEL)                                                                                          \
    hipLaunchKernelGGL(KERNEL, grid, dim3(kThreads), 0, (hipStream_t)stream, cost_reg, off_logit, prob, off, est_depth, est_dens, \
                       est_idx, avg_depth, D, HW, topk, near, interval, (size_t)view_stride)
#define MVS_DP_FORM(DR, KTV)                                                              \
    if (ahead && D == DR) MVS_DP_LAUNCH((depth_prob_topk_ahead_kernel<DR, KTV, true>));   \
    else if (ahead) MVS_DP_LAUNCH((depth_prob_topk_ahead_kernel<DR, KTV, false>));        \
    else MVS_DP_LAUNCH((depth_prob_topk_kernel<true, DR, KTV>))
#define MVS_DP_BY_D(KTV)                                                                  \
    if (D <= 16) { MVS_DP_FORM(16, KTV); }                                                \
    else if (D <= 64) { MVS_DP_FORM(64, KTV); }                                           \
    else if (ahead) MVS_DP_LAUNCH((depth_prob_topk_ahead_kernel<0, KTV, false>));         \
    else MVS_DP_LAUNCH((depth_prob_topk_kernel<true, 0, KTV>));
    const bool ahead = options().depthprob_ahead != 0;
    if (topk <= 3) { MVS_DP_BY_D(3) } else { MVS_DP_BY_D(MVSDET_MAX_TOPK) }
#undef MVS_DP_BY_D
#undef MVS_DP_FORM
#undef MVS_DP_LAUNCH
    MVS_LAUNCH_CHECK("depth_prob_topk");
    return MVSDET_OK;
}

extern "C" int mvsdet_depth_prob_topk_f32(const float* cost_reg, const float* off_logit, float* prob, float* off,
                                          float* est_depth, float* est_dens, int32_t* est_idx, float* avg_depth, int N,
                                          int D, int H, int W, int topk, float near, float interval,
                                          mvsdet_stream_t stream) {
    return mvsdet_depth_prob_topk_strided_f32(cost_reg, off_logit, (long long)D * H * W, prob, off, est_depth, est_dens, est_idx,
                                              avg_depth, N, D, H, W, topk, near, interval, stream);
}

extern "C" int mvsdet_sample_depth_prob_f32(const float* prob, const float* off, float* est_depth, float* est_dens,
                                            int32_t* est_idx, float* avg_depth, int N, int D, int H, int W, int topk,
                                            float near, float interval, mvsdet_stream_t stream) {
    MVS_REQUIRE(prob && off && est_depth && est_dens && avg_depth, "sample_depth_prob: NULL pointer");
    if (int rc = check_stage2("sample_depth_prob", N, D, H, W, topk)) return rc;
    const int HW = H * W;
    dim3 grid((HW + kThreads - 1) / kThreads, N);
    if (topk <= 3)
        hipLaunchKernelGGL((depth_prob_topk_kernel<false, 0, 3>), grid, dim3(kThreads), 0, (hipStream_t)stream, prob, off,
                           (float*)nullptr, (float*)nullptr, est_depth, est_dens, est_idx, avg_depth, D, HW, topk, near, interval,
                           (size_t)D * HW);
    else
    hipLaunchKernelGGL((depth_prob_topk_kernel<false, 0, MVSDET_MAX_TOPK>), grid, dim3(kThreads), 0, (hipStream_t)stream, prob, off,
                       (float*)nullptr, (float*)nullptr, est_depth, est_dens, est_idx, avg_depth, D, HW, topk, near, interval,
                       (size_t)D * HW);
    MVS_LAUNCH_CHECK("sample_depth_prob");
    return MVSDET_OK;
}

// ---------------------------------------------------------------------------------------------
// NVS-branch input: mvsdet.py:1158-1216 compute_depth_scale[_MultiIntrin] + :494.
//   ray = lift(x, y, 1) with the feature-level intrinsics (mvsdet.py:1300-1313), depth_scale = z of the normalised ray
//   = 1 / |ray| (get_camera_params with the identity pose, :1272-1297), est_ray_depth = est_depth / (depth_scale + 1e-8).
// One thread per pixel of the un-padded (h, w) feature map; the candidates come from the padded (H, W) maps.
// ---------------------------------------------------------------------------------------------
namespace mvsdet {
__global__ __launch_bounds__(kThreads) void ray_depth_kernel(const float* __restrict__ intr, const float* __restrict__ est_depth,
                                                             float* __restrict__ scale, float* __restrict__ ray_depth, int J,
                                                             int H, int W, int h, int w) {
    const int pix = blockIdx.x * kThreads + threadIdx.x;
    const int n = blockIdx.y;
    if (pix >= h * w) return;
    const int y = pix / w, x = pix - y * w;
    const float fx = intr[n * 5 + 0], fy = intr[n * 5 + 1], cx = intr[n * 5 + 2], cy = intr[n * 5 + 3], sk = intr[n * 5 + 4];
    // mvsdet.py:1308-1309, same operator order (z = 1)
    const float xl = ((float)x - cx + cy * sk / fy - sk * (float)y / fy) / fx * 1.0f;
    const float yl = ((float)y - cy) / fy * 1.0f;
    const float nrm = fmaxf(sqrtf(xl * xl + yl * yl + 1.0f), 1e-12f);   // F.normalize(dim=2): v / max(|v|, eps)
    const float sc = 1.0f / nrm;
    scale[(size_t)n * h * w + pix] = sc;
    if (ray_depth)
        for (int j = 0; j < J; ++j)
            ray_depth[((size_t)n * J + j) * h * w + pix] = est_depth[((size_t)n * J + j) * H * W + (size_t)y * W + x] / (sc + 1e-8f);
}
}  // namespace mvsdet

extern "C" int mvsdet_ray_depth_f32(const float* intr, const float* est_depth, float* depth_scale, float* est_ray_depth, int N,
                                    int J, int H, int W, int h, int w, mvsdet_stream_t stream) {
    MVS_REQUIRE(intr && depth_scale, "ray_depth: NULL pointer");
    MVS_REQUIRE((est_depth == nullptr) == (est_ray_depth == nullptr), "ray_depth: est_depth and est_ray_depth come together");
    MVS_REQUIRE(N > 0 && N <= 65535 && J >= 0 && h > 0 && w > 0 && h <= H && w <= W, "ray_depth: bad shape N=%d J=%d H=%d W=%d h=%d w=%d",
                N, J, H, W, h, w);
    dim3 grid((h * w + kThreads - 1) / kThreads, N);
    hipLaunchKernelGGL(ray_depth_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, intr, est_depth, depth_scale, est_ray_depth,
                       J, H, W, h, w);
    MVS_LAUNCH_CHECK("ray_depth");
    return MVSDET_OK;
}

extern "C" int mvsdet_depth_prob_topk_bwd_f32(const float* prob, const float* off, const int32_t* est_idx,
                                              const float* g_prob, const float* g_depth, const float* g_dens,
                                              const float* g_avg, float* g_cost, float* g_offlogit, int N, int D, int H,
                                              int W, int topk, float near, float interval, mvsdet_stream_t stream) {
    MVS_REQUIRE(prob && off && est_idx && g_cost && g_offlogit, "depth_prob_topk_bwd: NULL pointer");
    if (int rc = check_stage2("depth_prob_topk_bwd", N, D, H, W, topk)) return rc;
    const int HW = H * W;
    dim3 grid((HW + kThreads - 1) / kThreads, N);
    hipLaunchKernelGGL(depth_prob_topk_bwd_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, prob, off, est_idx, g_prob,
                       g_depth, g_dens, g_avg, g_cost, g_offlogit, D, HW, topk, near, interval);
    MVS_LAUNCH_CHECK("depth_prob_topk_bwd");
    return MVSDET_OK;
}
