// The fixed-order sums of the loss and metric kernels: no atomics, every sum in ONE association, the same bits on every run.
//   lanes    wave_sum: halving shuffles, ((v0+v32)+(v16+v48))+..., the sum in lane 0
//   waves    block_sums: lane 0 of every wave leaves its sum in LDS, thread 0 adds waves 0, 1, ... in ascending order
//   blocks   ordered_partial_sum: thread t adds its run of consecutive blocks ascending, thread 0 the 256 thread sums ascending
// Every walk starts from zero (T() / P{}), not from its first element.  The two differ in bits only where a total is -0.0:
//   depth_loss, photo_loss, depth_diag (pixel, voxel), nvs_score, bn3d: float64 sums of per-thread accumulators that start at +0.0,
//     which round-to-nearest never turns into -0.0; nvs_score seeded with wave 0's value before and keeps its bits for that reason.
//   assign_count, photo_select: integers.
//   head_loss: center, bbox and w are assigned, not accumulated, and w is the caller's centerness target, so a block of 256 positive
//     points could total -0.0f.  The block totals are workspace only, and head_loss_finish_kernel adds them to 0.f, which erases
//     that sign before any output: the argument relied on is the finishing kernel's seed, not the terms' range.
//
// Deliberately NOT here:
//   evalmap.hip's block_sum_f64 and block_scan_*: an LDS halving tree, another association; moving them would change AP bits.
//   The butterflies inside the MFMA kernels (costreg_head.hip, costreg_bf16.hip, costreg_mx.h's fmaxf ones): tuned inline.
#pragma once
#include "common.h"

namespace mvsdet {

// T = double, int, float.  Lane 0 holds ((v0+v32)+(v16+v48))+...; the other lanes hold sums of no use.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v = v + __shfl_down(v, o, kWave);
    return v;
}

// The butterfly: every lane holds the sum, and lane 0's has wave_sum's bits (at each step lane 0 adds the same two values, and
// IEEE addition commutes).  splat_render_bwd_kernel's form, kept as it is.
__device__ __forceinline__ float wave_sum_all(float x) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
    return x;
}

// The two halves of a block sum over NW waves: wave sums into LDS, and (after a barrier, in one thread) waves 0..NW-1 in order.
template <class T, int N, int NW>
__device__ __forceinline__ void wave_sums_to_lds(const T (&a)[N], T (&s)[N][NW]) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const T v = wave_sum(a[k]);
        if (lane == 0) s[k][wave] = v;
    }
}
template <class T, int N, int NW>
__device__ __forceinline__ void waves_in_order(T (&a)[N], const T (&s)[N][NW]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        a[k] = T();
        for (int w = 0; w < NW; ++w) a[k] = a[k] + s[k][w];
    }
}

// Sums over a block of NT threads, in place: true in thread 0, where a[] (and the counts n[]) then hold the block's sums; the other
// threads keep their own values.  One barrier.  The LDS is the function's own: a kernel that calls one instantiation twice puts a
// barrier between the calls.
template <int NT = kThreads, class T, int N>
__device__ __forceinline__ bool block_sums(T (&a)[N]) {
    __shared__ T s_a[N][NT / kWave];
    wave_sums_to_lds(a, s_a);
    __syncthreads();
    if (threadIdx.x != 0) return false;
    waves_in_order(a, s_a);
    return true;
}
template <int NT = kThreads, class T, int N, int NI>
__device__ __forceinline__ bool block_sums(T (&a)[N], int (&n)[NI]) {
    __shared__ T s_a[N][NT / kWave];
    __shared__ int s_n[NI][NT / kWave];
    wave_sums_to_lds(a, s_a);
    wave_sums_to_lds(n, s_n);
    __syncthreads();
    if (threadIdx.x != 0) return false;
    waves_in_order(a, s_a);
    waves_in_order(n, s_n);
    return true;
}

// The finishing walk of a one-block launch (kThreads threads) over the partials that nblocks blocks left: thread t adds blocks
// [t * run, min((t + 1) * run, nblocks)) ascending, thread 0 then adds thread sums 0..255 ascending: every partial enters in ascending
// block order.  P{} is the zero partial and P::add(const P&) adds one.  True in thread 0, where `total` is set.
template <class P>
__device__ __forceinline__ bool ordered_partial_sum(const P* __restrict__ part, int nblocks, P& total) {
    __shared__ P s_p[kThreads];
    const int run = (nblocks + kThreads - 1) / kThreads;
    const int first = threadIdx.x * run, last = min(first + run, nblocks);
    P a = {};
    for (int b = first; b < last; ++b) a.add(part[b]);
    s_p[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x != 0) return false;
    a = {};
    for (int t = 0; t < kThreads; ++t) a.add(s_p[t]);
    total = a;
    return true;
}

}  // namespace mvsdet
