// Depth supervision on gfx950: the reference's two masked depth objectives and their gradients.
//   kind 0 (l1)         MVSDet.depth_loss_func_new (mvsdet.py:893-915), one scene: g = ATen's bilinear resize of gt (N,Hg,Wg) to the
//                       (h,w) of est, mask = g > 0, loss = mean over the mask of |est - g|
//   kind 1 (smooth_l1)  mvsnet_loss (mvs_models/mvsnet.py:292-294): mask > 0.5, gt at est's size, smooth-L1 with beta = 1, mean
// Forward: two launches on one stream, no atomics.  One thread per (view, y, x) forms its term in fp32; a block adds terms (float64)
// and count in block_reduce.h's fixed order and leaves ONE partial at its own index; the finishing launch adds the partials in
// ascending block order (the same header's walk) and writes loss = sum / count (fp32) and count (int32).  Backward: one launch, one
// thread per pixel, a dense (N,h,w) gradient; it forms g again from gt (the same inlined code as the forward, so the same bits)
// instead of reading a staged copy: 4 taps of a map that sits in L2 against a (N,h,w) buffer kept alive from forward to backward.
//
// Roofline: neither.  N*h*w = 1.9e5 pixels per scene, 1.5 MB read at the most: the launches bound it.
#include "block_reduce.h"
#include "depth_resize.h"

namespace mvsdet {

struct DepthLossPartial {
    double sum;
    long long n;
    __device__ void add(const DepthLossPartial& r) {
        sum = sum + r.sum;
        n += r.n;
    }
};

// est - target and whether the pixel is inside the mask.  p = (i * h + y) * w + x.
template <int KIND>
__device__ __forceinline__ bool depth_loss_diff(const float* __restrict__ est, int64_t es0, int64_t es1, int64_t es2,
                                                const float* __restrict__ gt, int64_t gs0, int64_t gs1, int64_t gs2,
                                                const float* __restrict__ mask, int64_t ms0, int64_t ms1, int64_t ms2, long long p,
                                                int h, int w, int Hg, int Wg, float scale_y, float scale_x, float& d) {
    const unsigned q = (unsigned)p, hw = (unsigned)(h * w);   // p < N*h*w < 2^31 (checked on the host)
    const int i = (int)(q / hw), r = (int)(q - (unsigned)i * hw);
    const int y = r / w, x = r - y * w;
    float g;
    bool in;
    if (KIND == 0) {
        g = resized_at(gt + (int64_t)i * gs0, gs1, gs2, y, x, h, w, Hg, Wg, scale_y, scale_x);
        in = g > 0.0f;   // NaN fails the test and stays outside the mask (mvsdet.py:912)
    } else {
        g = gt[(int64_t)i * gs0 + (int64_t)y * gs1 + (int64_t)x * gs2];
        in = mask[(int64_t)i * ms0 + (int64_t)y * ms1 + (int64_t)x * ms2] > 0.5f;   // mvsnet.py:293
    }
    d = 0.0f;
    if (in) d = est[(int64_t)i * es0 + (int64_t)y * es1 + (int64_t)x * es2] - g;   // est is read inside the mask only
    return in;
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void depth_loss_kernel(
    const float* __restrict__ est, int64_t es0, int64_t es1, int64_t es2, const float* __restrict__ gt, int64_t gs0, int64_t gs1,
    int64_t gs2, const float* __restrict__ mask, int64_t ms0, int64_t ms1, int64_t ms2, DepthLossPartial* __restrict__ part,
    long long total, int h, int w, int Hg, int Wg, float scale_y, float scale_x) {
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    float term = 0.0f;
    int in_mask = 0;
    if (p < total) {
        float d;
        if (depth_loss_diff<KIND>(est, es0, es1, es2, gt, gs0, gs1, gs2, mask, ms0, ms1, ms2, p, h, w, Hg, Wg, scale_y, scale_x, d)) {
            const float a = fabsf(d);
            if (KIND == 0) term = a;
            else term = a < 1.0f ? 0.5f * a * a : a - 0.5f;   // smooth_l1, beta = 1
            in_mask = 1;
        }
    }
    double sum[1] = {(double)term};
    int n[1] = {in_mask};
    if (block_sums(sum, n)) part[blockIdx.x] = {sum[0], n[0]};
}

// One block: every partial enters in ascending block order (ordered_partial_sum), the same association on every call.
__global__ __launch_bounds__(kThreads) void depth_loss_finish_kernel(const DepthLossPartial* __restrict__ part, int nblocks,
                                                                     float* __restrict__ loss, int32_t* __restrict__ count) {
    DepthLossPartial r;
    if (ordered_partial_sum(part, nblocks, r)) {
        loss[0] = (float)(r.sum / (double)r.n);   // an empty mask: 0 / 0 = NaN, as torch.mean of nothing
        count[0] = (int32_t)r.n;
    }
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void depth_loss_bwd_kernel(
    const float* __restrict__ est, int64_t es0, int64_t es1, int64_t es2, const float* __restrict__ gt, int64_t gs0, int64_t gs1,
    int64_t gs2, const float* __restrict__ mask, int64_t ms0, int64_t ms1, int64_t ms2, const float* __restrict__ g_loss,
    const int32_t* __restrict__ count, float* __restrict__ grad, long long total, int h, int w, int Hg, int Wg, float scale_y,
    float scale_x) {
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= total) return;
    float d, out = 0.0f;
    if (depth_loss_diff<KIND>(est, es0, es1, es2, gt, gs0, gs1, gs2, mask, ms0, ms1, ms2, p, h, w, Hg, Wg, scale_y, scale_x, d)) {
        const float per_term = g_loss[0] / (float)count[0];   // count >= 1 here; one IEEE division, as mean's backward
        float s;
        if (KIND == 0) s = (d > 0.0f ? 1.0f : 0.0f) - (d < 0.0f ? 1.0f : 0.0f);        // ATen's sgn: sign(0) = 0, and 0 for NaN
        else s = d > 1.0f ? 1.0f : (d < -1.0f ? -1.0f : d);                            // clamp(d, -1, 1), NaN stays NaN
        out = per_term * s;
    }
    grad[p] = out;
}

}  // namespace mvsdet

using namespace mvsdet;

static int check_depth_loss(const char* name, const float* est, const int64_t* es, const float* gt, const int64_t* gs,
                            const float* mask, const int64_t* ms, int N, int h, int w, int Hg, int Wg, int kind) {
    MVS_REQUIRE(est && es && gt && gs, "%s: NULL pointer", name);
    MVS_REQUIRE(kind == MVSDET_DEPTH_LOSS_L1 || kind == MVSDET_DEPTH_LOSS_SMOOTH_L1, "%s: kind=%d is neither l1 (0) nor smooth_l1 (1)",
                name, kind);
    MVS_REQUIRE(N > 0 && h > 0 && w > 0, "%s: bad shape N=%d h=%d w=%d", name, N, h, w);
    MVS_REQUIRE(Hg >= 1 && Wg >= 1, "%s: bad gt shape %dx%d", name, Hg, Wg);
    MVS_REQUIRE((long long)N * h * w < (long long)INT32_MAX, "%s: %dx%dx%d exceeds 2^31 pixels", name, N, h, w);
    if (kind == MVSDET_DEPTH_LOSS_SMOOTH_L1) {
        MVS_REQUIRE(mask && ms, "%s: smooth_l1 needs a mask", name);
        MVS_REQUIRE(Hg == h && Wg == w, "%s: smooth_l1 takes gt at the size of est (%dx%d), got %dx%d", name, h, w, Hg, Wg);
    }
    return MVSDET_OK;
}

// One thread per pixel of l1 (kernel<0>) or smooth_l1 (kernel<1>), picked by `kind`; `own` are the kernel's arguments between the
// maps and the sizes.  Returns the block count.
template <class Kernel, class... Own>
static int launch_by_kind(Kernel l1, Kernel smooth_l1, int kind, mvsdet_stream_t stream, const float* est, const int64_t* es,
                          const float* gt, const int64_t* gs, const float* mask, const int64_t* mask_strides, int N, int h, int w, int Hg,
                          int Wg, Own... own) {
    const long long total = (long long)N * h * w;
    const int nblocks = (int)blocks_of(total);
    const int64_t zero[3] = {0, 0, 0};
    const int64_t* ms = mask_strides ? mask_strides : zero;
    // at::native::area_pixel_compute_scale: (float)input_size / output_size
    const float scale_y = (float)Hg / (float)h, scale_x = (float)Wg / (float)w;
    hipLaunchKernelGGL(kind == MVSDET_DEPTH_LOSS_L1 ? l1 : smooth_l1, dim3(nblocks), dim3(kThreads), 0, (hipStream_t)stream, est, es[0],
                       es[1], es[2], gt, gs[0], gs[1], gs[2], mask, ms[0], ms[1], ms[2], own..., total, h, w, Hg, Wg, scale_y, scale_x);
    return nblocks;
}

extern "C" size_t mvsdet_depth_loss_workspace_bytes(int N, int h, int w) {
    if (N <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)blocks_of((long long)N * h * w) * sizeof(DepthLossPartial);
}

extern "C" int mvsdet_depth_loss_f32(const float* est, const int64_t* est_strides, const float* gt, const int64_t* gt_strides,
                                     const float* mask, const int64_t* mask_strides, float* loss, int32_t* count, void* workspace,
                                     size_t workspace_bytes, int N, int h, int w, int Hg, int Wg, int kind, mvsdet_stream_t stream) {
    if (int rc = check_depth_loss("depth_loss", est, est_strides, gt, gt_strides, mask, mask_strides, N, h, w, Hg, Wg, kind)) return rc;
    MVS_REQUIRE(loss && count && workspace, "depth_loss: NULL pointer");
    MVS_REQUIRE(((uintptr_t)workspace & 15) == 0, "depth_loss: workspace must be 16-byte aligned");
    MVS_REQUIRE_WORKSPACE("depth_loss", workspace_bytes, mvsdet_depth_loss_workspace_bytes(N, h, w));
    DepthLossPartial* part = (DepthLossPartial*)workspace;
    const int nblocks = launch_by_kind(depth_loss_kernel<0>, depth_loss_kernel<1>, kind, stream, est, est_strides, gt, gt_strides, mask,
                                       mask_strides, N, h, w, Hg, Wg, part);
    MVS_LAUNCH_CHECK("depth_loss (terms)");
    hipLaunchKernelGGL(depth_loss_finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, part, nblocks, loss, count);
    MVS_LAUNCH_CHECK("depth_loss (finish)");
    return MVSDET_OK;
}

extern "C" int mvsdet_depth_loss_bwd_f32(const float* est, const int64_t* est_strides, const float* gt, const int64_t* gt_strides,
                                         const float* mask, const int64_t* mask_strides, const float* g_loss, const int32_t* count,
                                         float* grad, int N, int h, int w, int Hg, int Wg, int kind, mvsdet_stream_t stream) {
    if (int rc = check_depth_loss("depth_loss_bwd", est, est_strides, gt, gt_strides, mask, mask_strides, N, h, w, Hg, Wg, kind))
        return rc;
    MVS_REQUIRE(g_loss && count && grad, "depth_loss_bwd: NULL pointer");
    launch_by_kind(depth_loss_bwd_kernel<0>, depth_loss_bwd_kernel<1>, kind, stream, est, est_strides, gt, gt_strides, mask, mask_strides, N,
                   h, w, Hg, Wg, g_loss, count, grad);
    MVS_LAUNCH_CHECK("depth_loss_bwd");
    return MVSDET_OK;
}
