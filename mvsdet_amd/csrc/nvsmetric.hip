// Scores of the rendered target views (the reference's test loop, mvsdet.py:1017-1040: save_rendered_img_Image and
// save_rendered_depth of nerf_utils/save_rendered_img.py:21-44, 178-235; averaged by NVSMetric, Indoor_NVS.py:15-106) on the device.
//
// Per view v of a scene: psnr_v = -10 log(mse_v) / log(10) with mse_v the mean of (pred - gt)^2 over its 3 H W elements (+inf for
// mse 0, as the reference), ssim_v = the mean over the three channels of skimage's structural_similarity(channel_axis=-1,
// data_range=1) with its defaults: 7x7 box means ux, uy, uxx, uyy, uxy, sample covariance (cov_norm = 49/48), C1 = 0.01^2,
// C2 = 0.03^2, S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) averaged over the (H-6)(W-6) windows that lie
// wholly inside the image (skimage's crop [3:H-3, 3:W-3], so no border mode enters).  The depth error of a view is mean((pred -
// gt)^2) over its H W pixels -- the number the reference calls rmse; there is no root.  The scene's triple is the mean over its views
// (rmse 0 without a depth pair).
//
// ALL ARITHMETIC AFTER THE LOAD IS FLOAT64.  The inputs are float32, so x*x, y*y, x*y and x - y are exact in float64 and a window sum
// of 49 of them carries an error near 1e-16: uxx - ux*ux does not cancel on flat image regions the way it does in float32 (where the
// reference's own float32 route lies up to 1.4e-7 from the exact value).  A scene is 6.9 M window sums; the cost does not matter.
//
// mvsdet_nvs_score_f32, two launches:
//   nvs_score_kernel, one block of 256 threads per (plane, tile): planes are the n_tgt x 3 colour planes and, with a depth pair, n_tgt
//     depth planes behind them; a tile is 32 x 16 window centres.  The block stages the tile and its 6-pixel halo (38 x 22 pixels) of
//     x and y as float32 in LDS with row loads (consecutive lanes, consecutive columns; every tensor is read in place through its
//     element strides), adds the squared error of the pixels it owns (its 32 x 16 corner of the staged box; the last tile of a row /
//     column owns the box to the image's edge, so every pixel has one owner), forms the five 7-tap row sums in float64 into LDS and the
//     7-tap column sums from them, evaluates S and reduces both sums inside the block (block_reduce.h).
//     Depth planes skip the windows.  No atomics: the block writes its two sums to the workspace slot of its block index.
//     LDS: 2 x 38 x 22 x 4 + 5 x 32 x 22 x 8 + 64 = 34912 bytes -> 4 blocks (16 waves) per CU, LDS-bound.
//   nvs_finish_kernel, one block: a thread per plane adds the plane's slots in slot order; thread 0 then adds the channels of a view,
//     writes (psnr_v, ssim_v) to the view's row, adds the views in order, writes the scene's (psnr, ssim, rmse) and adds them and a
//     scene count to the accumulator state (4 float64).  One fixed order everywhere: two runs give the same bits, and a view's two
//     values do not depend on the views beside it.
#include "block_reduce.h"

#include <climits>

namespace mvsdet {
namespace {

constexpr int kTW = 32, kTH = 16;          // window centres of a tile
constexpr int kHalo = 6;                   // a 7x7 window reaches 6 pixels past its first
constexpr int kSW = kTW + kHalo, kSH = kTH + kHalo;
constexpr int kStateDoubles = MVSDET_NVS_STATE_DOUBLES;

struct NvsParams {
    const float* pred;
    const float* gt;
    const float* pred_depth;
    const float* gt_depth;
    long long ps[4], gs[4];       // element strides (view, channel, row, column)
    long long pds[3], gds[3];     // (view, row, column)
    int n_tgt, H, W;
    int tiles_x, tiles;
    int colour_planes, planes;
    double* slots;                // [planes * tiles][2] = squared error, sum of S; then [planes][2] plane sums
};

__global__ __launch_bounds__(kThreads) void nvs_score_kernel(NvsParams p) {
    __shared__ float sx[kSH * kSW];
    __shared__ float sy[kSH * kSW];
    __shared__ double rs[5][kSH * kTW];
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const int tx = tile % p.tiles_x, ty = tile / p.tiles_x;
    const bool colour = plane < p.colour_planes;
    const float* xb;
    const float* yb;
    long long xr, xc, yr, yc;
    if (colour) {
        const int v = plane / 3, c = plane % 3;
        xb = p.pred + v * p.ps[0] + c * p.ps[1], xr = p.ps[2], xc = p.ps[3];
        yb = p.gt + v * p.gs[0] + c * p.gs[1], yr = p.gs[2], yc = p.gs[3];
    } else {
        const int v = plane - p.colour_planes;
        xb = p.pred_depth + v * p.pds[0], xr = p.pds[1], xc = p.pds[2];
        yb = p.gt_depth + v * p.gds[0], yr = p.gds[1], yc = p.gds[2];
    }
    const int x0 = tx * kTW, y0 = ty * kTH;
    const int sw = min(kSW, p.W - x0), sh = min(kSH, p.H - y0);          // staged box, >= 7 each way
    const int own_w = (x0 + kTW + kHalo >= p.W) ? sw : kTW;              // the last tile owns its box to the edge
    const int own_h = (y0 + kTH + kHalo >= p.H) ? sh : kTH;
    double se = 0.0, ss = 0.0;
    for (int i = tid; i < kSH * kSW; i += kThreads) {
        const int r = i / kSW, c = i % kSW;
        float x = 0.f, y = 0.f;
        if (r < sh && c < sw) {
            x = xb[(y0 + r) * xr + (x0 + c) * xc];
            y = yb[(y0 + r) * yr + (x0 + c) * yc];
            if (r < own_h && c < own_w) {
                const double d = (double)x - (double)y;
                se += d * d;
            }
        }
        sx[i] = x, sy[i] = y;
    }
    __syncthreads();
    if (colour) {
        const int nw = sw - kHalo, nh = sh - kHalo;                      // window centres of this tile
        for (int i = tid; i < kSH * kTW; i += kThreads) {
            const int r = i / kTW, c = i % kTW;
            double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
            if (r < sh && c < nw) {
                for (int k = 0; k <= kHalo; ++k) {
                    const double x = (double)sx[r * kSW + c + k], y = (double)sy[r * kSW + c + k];
                    a += x, b += y, aa += x * x, bb += y * y, ab += x * y;
                }
            }
            rs[0][i] = a, rs[1][i] = b, rs[2][i] = aa, rs[3][i] = bb, rs[4][i] = ab;
        }
        __syncthreads();
        const double C1 = (0.01 * 1.0) * (0.01 * 1.0), C2 = (0.03 * 1.0) * (0.03 * 1.0), cov_norm = 49.0 / 48.0;
        for (int i = tid; i < kTH * kTW; i += kThreads) {
            const int r = i / kTW, c = i % kTW;
            if (r < nh && c < nw) {
                double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
                for (int k = 0; k <= kHalo; ++k) {
                    const int j = (r + k) * kTW + c;
                    a += rs[0][j], b += rs[1][j], aa += rs[2][j], bb += rs[3][j], ab += rs[4][j];
                }
                const double ux = a / 49.0, uy = b / 49.0, uxx = aa / 49.0, uyy = bb / 49.0, uxy = ab / 49.0;
                const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
                const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
                const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
                ss += (A1 * A2) / (B1 * B2);
            }
        }
    }
    double sums[2] = {se, ss};
    if (block_sums(sums)) {
        p.slots[2 * (size_t)blockIdx.x] = sums[0];
        p.slots[2 * (size_t)blockIdx.x + 1] = sums[1];
    }
}

__global__ __launch_bounds__(kThreads) void nvs_finish_kernel(NvsParams p, double* __restrict__ out_views, double* __restrict__ out_scene,
                                                              double* __restrict__ state) {
    double* plane_sums = p.slots + 2 * (size_t)p.planes * p.tiles;
    for (int plane = threadIdx.x; plane < p.planes; plane += kThreads) {
        const double* s = p.slots + 2 * (size_t)plane * p.tiles;
        double a = 0.0, b = 0.0;
        for (int t = 0; t < p.tiles; ++t) a += s[2 * t], b += s[2 * t + 1];
        plane_sums[2 * plane] = a, plane_sums[2 * plane + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double pixels = (double)p.H * (double)p.W, windows = (double)(p.H - kHalo) * (double)(p.W - kHalo);
    double psnr = 0.0, ssim = 0.0, rmse = 0.0;
    for (int v = 0; v < p.n_tgt && p.colour_planes; ++v) {
        const double* c = plane_sums + 6 * v;
        const double mse = (c[0] + c[2] + c[4]) / (3.0 * pixels);
        const double psnr_v = -10.0 * log(mse) / log(10.0);
        const double ssim_v = (c[1] / windows + c[3] / windows + c[5] / windows) / 3.0;
        out_views[2 * v] = psnr_v, out_views[2 * v + 1] = ssim_v;
        psnr += psnr_v, ssim += ssim_v;
    }
    for (int v = 0; v < p.n_tgt && p.planes > p.colour_planes; ++v) rmse += plane_sums[2 * (p.colour_planes + v)] / pixels;
    psnr /= (double)p.n_tgt, ssim /= (double)p.n_tgt, rmse /= (double)p.n_tgt;
    out_scene[0] = psnr, out_scene[1] = ssim, out_scene[2] = rmse;
    if (state) state[0] += psnr, state[1] += ssim, state[2] += rmse, state[3] += 1.0;
}

__global__ void nvs_reset_kernel(double* state) {
    if (threadIdx.x < kStateDoubles) state[threadIdx.x] = 0.0;
}

// tiles of one plane; 0 for sizes the scoring launch does not take
long long tiles_of(int H, int W, int* tiles_x) {
    if (H < 7 || W < 7) return 0;
    const int nx = (W - kHalo + kTW - 1) / kTW, ny = (H - kHalo + kTH - 1) / kTH;
    if (tiles_x) *tiles_x = nx;
    return (long long)nx * ny;
}

bool sizes_ok(int n_tgt, int H, int W) {
    return n_tgt >= 1 && H >= 7 && W >= 7 && (long long)n_tgt * 3 * H * W <= INT32_MAX
           && 4ll * n_tgt * tiles_of(H, W, nullptr) <= INT32_MAX;
}

}  // namespace
}  // namespace mvsdet

using namespace mvsdet;

extern "C" size_t mvsdet_nvs_workspace_bytes(int n_tgt, int H, int W, int with_depth) {
    if (!sizes_ok(n_tgt, H, W)) return 0;
    const size_t planes = (size_t)n_tgt * (with_depth ? 4 : 3);
    return (planes * (size_t)tiles_of(H, W, nullptr) + planes) * 2 * sizeof(double);
}

extern "C" int mvsdet_nvs_reset(double* state, mvsdet_stream_t stream) {
    MVS_REQUIRE(state, "nvs_reset: NULL pointer");
    MVS_REQUIRE((uintptr_t)state % 8 == 0, "nvs_reset: state must be 8-byte aligned");
    hipLaunchKernelGGL(nvs_reset_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, state);
    MVS_LAUNCH_CHECK("nvs_reset");
    return MVSDET_OK;
}

extern "C" int mvsdet_nvs_score_f32(double* state, const float* pred, const int64_t* pred_strides, const float* gt,
                                    const int64_t* gt_strides, const float* pred_depth, const int64_t* pred_depth_strides,
                                    const float* gt_depth, const int64_t* gt_depth_strides, int n_tgt, int H, int W, double* out_views,
                                    double* out_scene, void* workspace, size_t workspace_bytes, mvsdet_stream_t stream) {
    MVS_REQUIRE(n_tgt >= 1 && H >= 7 && W >= 7, "nvs_score: bad shape n_tgt=%d H=%d W=%d (a 7x7 window needs sides of 7)", n_tgt, H, W);
    MVS_REQUIRE(sizes_ok(n_tgt, H, W), "nvs_score: n_tgt=%d H=%d W=%d: n_tgt * 3 * H * W must stay below 2^31", n_tgt, H, W);
    MVS_REQUIRE((pred != nullptr) == (gt != nullptr) && (pred_depth != nullptr) == (gt_depth != nullptr) && (pred || pred_depth),
                "nvs_score: an image pair, a depth pair or both are needed");
    MVS_REQUIRE(out_scene && workspace, "nvs_score: NULL pointer");
    MVS_REQUIRE(!pred || (pred_strides && gt_strides && out_views), "nvs_score: NULL pointer (image strides, out_views)");
    MVS_REQUIRE(!pred_depth || (pred_depth_strides && gt_depth_strides), "nvs_score: NULL pointer (depth strides)");
    MVS_REQUIRE(pred || !state, "nvs_score: a depth pair alone is not a scene of the state");
    MVS_REQUIRE((uintptr_t)workspace % 8 == 0 && (uintptr_t)out_views % 8 == 0 && (uintptr_t)out_scene % 8 == 0 && (uintptr_t)state % 8 == 0,
                "nvs_score: workspace, outputs and state must be 8-byte aligned");
    NvsParams p;
    p.pred = pred, p.gt = gt, p.pred_depth = pred_depth, p.gt_depth = gt_depth;
    for (int i = 0; i < 4; ++i) p.ps[i] = pred ? pred_strides[i] : 0, p.gs[i] = pred ? gt_strides[i] : 0;
    for (int i = 0; i < 3; ++i) p.pds[i] = pred_depth ? pred_depth_strides[i] : 0, p.gds[i] = pred_depth ? gt_depth_strides[i] : 0;
    p.n_tgt = n_tgt, p.H = H, p.W = W;
    p.tiles = (int)tiles_of(H, W, &p.tiles_x);
    p.colour_planes = pred ? 3 * n_tgt : 0, p.planes = p.colour_planes + (pred_depth ? n_tgt : 0);
    p.slots = static_cast<double*>(workspace);
    MVS_REQUIRE_WORKSPACE("nvs_score", workspace_bytes, ((size_t)p.planes * p.tiles + p.planes) * 2 * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nvs_score_kernel, dim3((unsigned)(p.planes * p.tiles)), dim3(kThreads), 0, st, p);
    hipLaunchKernelGGL(nvs_finish_kernel, dim3(1), dim3(kThreads), 0, st, p, out_views, out_scene, state);
    MVS_LAUNCH_CHECK("nvs_score");
    return MVSDET_OK;
}
