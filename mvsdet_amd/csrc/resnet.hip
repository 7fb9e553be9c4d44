// The bottleneck layers of a ResNet (v1.5: the stride sits on the 3x3) with frozen BatchNorm, on the bf16 matrix cores with three-term
// split operands: the cut, the three products and the 1x1's GEMM block are mfma.h's, shared with fpn.hip and neck_gemm.hip.
//
// The shipped backbone is ResNet(depth=50, style='pytorch', norm_eval=True, norm_cfg=dict(type='BN', requires_grad=False)): every
// BatchNorm is the fixed affine y * scale + shift, no convolution has a bias.  mmdet is not part of this tree; the definition is the
// builder's reading of ResNet v1.5 (include/mvsdet_hip.h has it).  Every layer is
//
//   out = [relu]( (W' x + shift) [+ residual] ),   W' = the weight rows times `scale`, folded on the host before the split
//
// in exactly that order of additions; ReLU is `v < 0 ? 0 : v`, so a NaN stays a NaN as under torch.relu.
//
// resnet_conv1x1_kernel: fpn_lateral_kernel's GEMM (gemm_bf16x3_block, 128 rows x 64 columns) with a strided gather: the columns run
//   over ALL views' OUTPUT pixels, v = n Ho Wo + pixel, and the fetch reads the source pixel (s y, s x).
//
// resnet_conv3x3_kernel<S> (its tile and main loop are resnet_conv3x3.h's, shared with resnet_bwd.hip; the epilogue is here):
//   fpn_conv3x3_kernel's halo-tile form (implicit GEMM, K = 9 Cin tap-major, the halo staged once per 32 input channels as [piece][k-group of 8][halo pixel] 16-byte units, two stages).  S = 1: 16 x 8 output pixels, four accumulators, an
//   18 x 10 halo.  S = 2: 16 x 4 output pixels, two accumulators, a 33 x 9 halo (37.1 KiB per stage: two blocks per CU); its halo rows
//   are stored EVEN columns first (17 of them), ODD columns after (16), so that the sixteen lanes of an output row, whose halo columns
//   2 lx + dx lie two apart, still read sixteen consecutive 16-byte units under every tap.
//
// The matrix handed in has ceil(Cout / 128) * 128 rows, those from Cout on zero (mvsdet_gemm_split_weight wants M % 128 == 0, layer 1
// has Cout = 64).  A wave whose 32 rows lie at or beyond Cout stores nothing; it still stages its share and reaches every barrier.
//
// No atomics: the same bits on every run.  Element offsets are 64-bit.
#include "common.h"
#include "mfma.h"
#include "resnet_conv3x3.h"

namespace mvsdet {

__device__ __forceinline__ float rn_relu(float v, int relu) { return relu && v < 0.0f ? 0.0f : v; }

// x (N,K,H,W), out and residual (N,M,Ho,Wo); columns v = n HWo + output pixel, V = N HWo of them
__global__ __launch_bounds__(kThreads) void resnet_conv1x1_kernel(const float* __restrict__ x, const uint4* __restrict__ ws,
                                                                  const float* __restrict__ shift, const float* __restrict__ residual,
                                                                  float* __restrict__ out, int M, int K, int HW, int W, int HWo, int Wo, int V,
                                                                  int stride, int relu) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.y * kGemmBM, v0 = blockIdx.x * kGemmBN;

    // staging duty: column v0 + (tid & 63), channels 8 * (tid >> 6) .. + 7 of the step
    const int sv = v0 + (tid & 63), skq = tid >> 6;
    const bool sv_ok = sv < V;
    const int sn = sv_ok ? sv / HWo : 0, spix = sv_ok ? sv - sn * HWo : 0;
    const int sy = spix / Wo, sx = spix - sy * Wo;
    const float* xs = x + ((size_t)sn * K + 8 * skq) * HW + (size_t)(stride * sy) * W + stride * sx;
    float f[8];
    auto fetch = [&](int ks) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = sv_ok ? xs[(size_t)(ks * kGemmBK + j) * HW] : 0.0f;
    };

    f32x16 acc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.0f;
    gemm_bf16x3_block(acc, f, fetch, ws, m0, K, tid, wave);

    // ---- epilogue: (acc + shift) [+ residual], then ReLU
    const int mw = m0 + 32 * wave;
    if (mw >= M) return;                                   // rows of the zero padding: nothing to store (after the last barrier)
    const int half = lane >> 5;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int v = v0 + 32 * c + (lane & 31);
        if (v >= V) continue;
        const int n = v / HWo, pix = v - n * HWo;
        const size_t base = ((size_t)n * M + mw) * HWo + pix;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = mfma32_row(i, half);
            const size_t o = base + (size_t)row * HWo;
            float val = acc[c][i] + shift[mw + row];
            if (residual) val += residual[o];
            out[o] = rn_relu(val, relu);
        }
    }
}

// x (N,Cin,H,W), ws = split (ceil128(M), 9 Cin) tap-major matrix, out (N,M,Ho,Wo)
template <int S>
__global__ __launch_bounds__(kThreads) void resnet_conv3x3_kernel(const float* __restrict__ x, const uint4* __restrict__ ws,
                                                                  const float* __restrict__ shift, float* __restrict__ out, int M, int Cin,
                                                                  int H, int W, int Ho, int Wo, int tiles_x, int relu) {
    using T = RnTile<S>;
    const size_t HWo = (size_t)Ho * Wo;
    // ---- epilogue: acc + shift, then ReLU; fp32 NCHW rows
    rn_conv3x3_block<S>(x, ws, M, Cin, H, W, tiles_x, [&](const f32x16 (&acc)[T::NT], int n, int mw, int y0, int x0, int lx, int ly, int half) {
        float b[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) b[i] = shift[mw + mfma32_row(i, half)];
#pragma unroll
        for (int t = 0; t < T::NT; ++t) {
            const int y = y0 + 2 * t + ly, xx = x0 + lx;
            if (y >= Ho || xx >= Wo) continue;
            float* o = out + ((size_t)n * M + mw) * HWo + (size_t)y * Wo + xx;
#pragma unroll
            for (int i = 0; i < 16; ++i) o[(size_t)mfma32_row(i, half) * HWo] = rn_relu(acc[t][i] + b[i], relu);
        }
    });
}

template <int S>
static int launch_conv3x3(const float* x, const void* wsplit, const float* shift, float* out, int N, int Cin, int Cout, int H, int W, int Ho,
                          int Wo, int relu, hipStream_t stream) {
    using T = RnTile<S>;
    const long long tiles_x = (Wo + T::TW - 1) / T::TW, tiles_y = (Ho + T::TH - 1) / T::TH;
    MVS_GRANT_LDS("resnet_conv3x3_bf16x3", resnet_conv3x3_kernel<S>, T::LdsBytes, T::LdsBytes);
    dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)((Cout + kGemmBM - 1) / kGemmBM), (unsigned)N);
    hipLaunchKernelGGL(resnet_conv3x3_kernel<S>, grid, dim3(kThreads), T::LdsBytes, stream, x, static_cast<const uint4*>(wsplit), shift, out, Cout,
                       Cin, H, W, Ho, Wo, (int)tiles_x, relu);
    MVS_LAUNCH_CHECK("resnet_conv3x3_bf16x3");
    return MVSDET_OK;
}

}  // namespace mvsdet

using namespace mvsdet;

extern "C" int mvsdet_resnet_conv1x1_bf16x3(const float* x, const void* wsplit, const float* shift, const float* residual, float* out, int N,
                                            int Cin, int Cout, int H, int W, int stride, int relu, mvsdet_stream_t stream) {
    MVS_REQUIRE(x && wsplit && shift && out, "resnet_conv1x1_bf16x3: NULL pointer");
    MVS_REQUIRE(N > 0 && H > 0 && W > 0, "resnet_conv1x1_bf16x3: bad shape N=%d H=%d W=%d", N, H, W);
    MVS_REQUIRE(stride == 1 || stride == 2, "resnet_conv1x1_bf16x3: stride=%d must be 1 or 2", stride);
    MVS_REQUIRE(Cin > 0 && Cin % kGemmBK == 0 && Cout > 0 && Cout % 32 == 0, "resnet_conv1x1_bf16x3: Cin=%d must be a multiple of %d and Cout=%d of 32",
                Cin, kGemmBK, Cout);
    MVS_REQUIRE(Cout <= 65535 * kGemmBM, "resnet_conv1x1_bf16x3: too many rows");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    MVS_REQUIRE((long long)H * W < INT32_MAX, "resnet_conv1x1_bf16x3: map %d x %d too large", H, W);
    MVS_REQUIRE((long long)N * Ho * Wo <= INT32_MAX - kGemmBN, "resnet_conv1x1_bf16x3: N Ho Wo = %lld columns exceed 2^31", (long long)N * Ho * Wo);
    MVS_REQUIRE(((uintptr_t)wsplit & 15u) == 0 && ((uintptr_t)x & 3u) == 0 && ((uintptr_t)out & 3u) == 0 && ((uintptr_t)shift & 3u) == 0 &&
                    ((uintptr_t)residual & 3u) == 0,
                "resnet_conv1x1_bf16x3: wsplit must be 16-byte, the tensors 4-byte aligned");
    const int V = N * Ho * Wo;
    dim3 grid((unsigned)((V + kGemmBN - 1) / kGemmBN), (unsigned)((Cout + kGemmBM - 1) / kGemmBM));
    hipLaunchKernelGGL(resnet_conv1x1_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, x, static_cast<const uint4*>(wsplit), shift, residual,
                       out, Cout, Cin, H * W, W, Ho * Wo, Wo, V, stride, relu ? 1 : 0);
    MVS_LAUNCH_CHECK("resnet_conv1x1_bf16x3");
    return MVSDET_OK;
}

extern "C" int mvsdet_resnet_conv3x3_bf16x3(const float* x, const void* wsplit, const float* shift, float* out, int N, int Cin, int Cout, int H,
                                            int W, int stride, int relu, mvsdet_stream_t stream) {
    MVS_REQUIRE(x && wsplit && shift && out, "resnet_conv3x3_bf16x3: NULL pointer");
    MVS_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "resnet_conv3x3_bf16x3: bad shape N=%d H=%d W=%d", N, H, W);
    MVS_REQUIRE(stride == 1 || stride == 2, "resnet_conv3x3_bf16x3: stride=%d must be 1 or 2", stride);
    MVS_REQUIRE(Cin > 0 && Cin % kGemmBK == 0 && Cout > 0 && Cout % 32 == 0, "resnet_conv3x3_bf16x3: Cin=%d must be a multiple of %d and Cout=%d of 32",
                Cin, kGemmBK, Cout);
    MVS_REQUIRE(Cout <= 65535 * kGemmBM && Cin <= INT32_MAX / 9, "resnet_conv3x3_bf16x3: too many channels");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    MVS_REQUIRE((long long)H * W < INT32_MAX && (long long)N * Ho * Wo < INT32_MAX, "resnet_conv3x3_bf16x3: map %d x %d of %d views too large", H,
                W, N);
    MVS_REQUIRE(((uintptr_t)wsplit & 15u) == 0 && ((uintptr_t)x & 3u) == 0 && ((uintptr_t)out & 3u) == 0 && ((uintptr_t)shift & 3u) == 0,
                "resnet_conv3x3_bf16x3: wsplit must be 16-byte, the tensors 4-byte aligned");
    if (stride == 1) return launch_conv3x3<1>(x, wsplit, shift, out, N, Cin, Cout, H, W, Ho, Wo, relu ? 1 : 0, (hipStream_t)stream);
    return launch_conv3x3<2>(x, wsplit, shift, out, N, Cin, Cout, H, W, Ho, Wo, relu ? 1 : 0, (hipStream_t)stream);
}
