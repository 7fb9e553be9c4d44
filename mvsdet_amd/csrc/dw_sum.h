// The last step of a split-K weight gradient (fpn_bwd.hip, resnet_bwd.hip): the splits' fp32 partials added in ascending order.
// Included after common.h.
#pragma once

namespace mvsdet {

// dw (Cout,C,kh,kw)[o][c][tap] = partial[0][tap][o][c] + partial[1][tap][o][c] + ... in ascending order; one thread per element,
// oc = Cout C.  No atomics: the same bits on every run.
__device__ __forceinline__ void dw_sum_splits(const float* __restrict__ partial, float* __restrict__ dw, int nsplit, int taps, long long oc) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;   // index into [tap][o][c]
    if (e >= oc * taps) return;
    float s = 0.0f;
    for (int k = 0; k < nsplit; ++k) s = s + partial[(size_t)k * taps * oc + e];
    const long long tap = e / oc, r = e - tap * oc;
    dw[r * taps + tap] = s;
}

}  // namespace mvsdet
