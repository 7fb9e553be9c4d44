// The 3-D neck's two GEMM-shaped layers on the bf16 matrix cores with three-term split operands:
//
//   * the 1x1x1 stride-2 shortcut of a down-sampling ResModule (mmdet3d/models/necks/imvoxel_neck.py:196-217 `downsample`):
//       out[n][o][d][h][w] = sum_c W[o][c] x[n][c][2d][2h][2w] + bias[o]                        (BatchNorm folded into W, bias)
//   * the kernel-2 stride-2 transposed convolution of an up block (imvoxel_neck.py:166-180, first three layers):
//       out[n][o][2d+p][2h+q][2w+r] = relu(sum_c x[n][c][d][h][w] W[c][o][p][q][r] + bias[o])   -- 8 single-tap classes
//
// Both are C[M][v] = A[M][K] B[K][v] with B = the activations as they lie in memory (NCDHW: a channel is a row of voxels).
// Rounds 2-4 ran them as rocBLAS fp32 GEMMs plus ATen glue around them (the strided sub-sampling copy, the bias broadcast, a
// permuting clamp for the 2x2x2 interleave: four Cijk kernels, ~20 small launches and ~0.35 ms of a 2.2 ms neck).  Here:
// one kernel per layer, bias, ReLU and the interleave in its epilogue, the sub-sampling in its gather.
//
// Block = 128 rows (M) x 64 voxels, K in steps of 32 channels: gemm_bf16x3_block of mfma.h (the weight matrix cut into bf16 hi / mid ONCE
// per weight version by mvsdet_gemm_split_weight and kept on the module, read in fragment order from L2; the activations cut on the way
// into a double-buffered LDS stage).  A thread fetches the 8 channels of its voxel, coalesced along the voxels.
//
// Training (autograd) adds the two layers' input gradients as MODEs 2 and 3 of the same kernel (A = the transposed / reshaped
// weight matrix, split per call) and their weight gradients as one NT GEMM that reduces over the voxels (neck_gemm_dw_bf16x3_kernel:
// both operands activations, cut into bf16 pieces on the way into the LDS; split-K partial sums added in a fixed order).
//
// Row order for the transposed layer: m = 8 o + 4 p + 2 q + r, so that the 32x32 accumulator's rows (mfma32_row of mfma.h: (reg & 3)
// + 4 (lane >> 5) + 8 (reg >> 2)) give a lane four output channels (reg >> 2) at depth parity p = lane >> 5 with (q, r) = reg & 3: a float2
// store {r = 0, 1} per (channel, q), contiguous along w across the lanes of a row.
#include "common.h"
#include "mfma.h"

#include <algorithm>

namespace mvsdet {

// wmat (M, K) fp32 row-major -> [M/32][K/16][2 pieces][64 lanes][8 bf16]: lane = 32 * (k-group of 8) + row of the tile
__global__ __launch_bounds__(kThreads) void gemm_split_weight_kernel(const float* __restrict__ wmat, uint4* __restrict__ ws, int M, int K) {
    const size_t u = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const size_t units = (size_t)(M / 32) * (K / 16) * 64;
    if (u >= units) return;
    const int lane = (int)(u & 63);
    const size_t t = u >> 6;
    const int k16 = (int)(t % (K / 16)), rt = (int)(t / (K / 16));
    const float* src = wmat + (size_t)(rt * 32 + (lane & 31)) * K + k16 * 16 + 8 * (lane >> 5);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = src[j];
    u32x4 hi, mid;
    bf16x3_cut8(f, hi, mid);
    ws[(t * 2 + 0) * 64 + lane] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    ws[(t * 2 + 1) * 64 + lane] = make_uint4(mid[0], mid[1], mid[2], mid[3]);
}

// MODE 0: pointwise stride-2 convolution (x (N,K,D,H,W), out (N,M,D/2,H/2,W/2), voxel = coarse voxel, gather at 2x);
// MODE 1: transposed k2 s2 (x (N,K,D,H,W), rows m = 8 o + 4 p + 2 q + r, out (N,M/8,2D,2H,2W));
// MODE 2: input gradient of MODE 0 (x = grad_out (N,K,D/2,H/2,W/2), rows m = input channels, out (N,M,D,H,W) ACCUMULATED at the even
//         positions only -- the other positions are not touched; bias unused);
// MODE 3: input gradient of MODE 1 (x = grad_out (N,K/8,2D,2H,2W), k = 8 o + 4 p + 2 q + r gathered from each voxel's 2x2x2 cube,
//         rows m = input channels, out (N,M,D,H,W); bias unused)
template <int MODE>
__global__ __launch_bounds__(kThreads) void neck_gemm_bf16x3_kernel(const float* __restrict__ x, const uint4* __restrict__ ws,
                                                                    const float* __restrict__ bias, float* __restrict__ out, int M,
                                                                    int K, int D, int H, int W, int relu) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.z, m0 = blockIdx.y * kGemmBM, v0 = blockIdx.x * kGemmBN;
    // the voxel grid the columns run over: MODEs 0 and 2 the coarse grid of D x H x W, MODEs 1 and 3 the grid D x H x W itself
    const bool coarse = MODE == 0 || MODE == 2;
    const int Dv = coarse ? D / 2 : D, Hv = coarse ? H / 2 : H, Wv = coarse ? W / 2 : W;
    const int V = Dv * Hv * Wv;
    // channel pitch of the B operand: MODE 0 / 1 x on D x H x W, MODE 2 grad_out on the coarse grid, MODE 3 grad_out on 2D x 2H x 2W
    const size_t plane = MODE == 2 ? (size_t)V : MODE == 3 ? (size_t)8 * D * H * W : (size_t)D * H * W;

    // staging duty: voxel v0 + (tid & 63), channels 8 * (tid >> 6) .. + 7 of the step
    const int sv = v0 + (tid & 63), skq = tid >> 6;
    const bool sv_ok = sv < V;
    size_t soff = 0;
    if (sv_ok) {
        if (MODE == 0) {
            const int d = sv / (Hv * Wv), r = sv - d * Hv * Wv, h = r / Wv, w = r - h * Wv;
            soff = ((size_t)2 * d * H + 2 * h) * W + 2 * w;
        } else if (MODE == 3) {   // corner (2d, 2h, 2w) of the voxel's cube in grad_out
            const int d = sv / (Hv * Wv), r = sv - d * Hv * Wv, h = r / Wv, w = r - h * Wv;
            soff = ((size_t)2 * d * 2 * H + 2 * h) * 2 * W + 2 * w;
        } else {
            soff = (size_t)sv;
        }
    }
    // MODE 3: the 8 k of a staging duty are the 8 taps of ONE grad_out channel o = 4 ks + skq
    const float* xs = MODE == 3 ? x + ((size_t)n * (K / 8) + skq) * plane + soff : x + ((size_t)n * K + 8 * skq) * plane + soff;
    float f[8];
    auto fetch = [&](int ks) {
        if (MODE == 3) {
            const size_t W2 = 2 * (size_t)W, HW2 = 4 * (size_t)H * W;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                f[j] = sv_ok ? xs[(size_t)(4 * ks) * plane + (j >> 2) * HW2 + ((j >> 1) & 1) * W2 + (j & 1)] : 0.0f;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = sv_ok ? xs[(size_t)(ks * kGemmBK + j) * plane] : 0.0f;
        }
    };

    f32x16 acc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.0f;
    gemm_bf16x3_block(acc, f, fetch, ws, m0, K, tid, wave);

    // ---- epilogue
    const int half = lane >> 5;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int v = v0 + 32 * c + (lane & 31);
        if (v >= V) continue;
        if (MODE == 2) {   // += at the even positions of the (D, H, W) input gradient: one thread per element, no atomics
            const int d = v / (Hv * Wv), r = v - d * Hv * Wv, h = r / Wv, w = r - h * Wv;
            const size_t vol = (size_t)D * H * W;
            float* o = out + ((size_t)n * M + m0 + 32 * wave) * vol + ((size_t)2 * d * H + 2 * h) * W + 2 * w;
#pragma unroll
            for (int i = 0; i < 16; ++i) o[(size_t)mfma32_row(i, half) * vol] += acc[c][i];
        } else if (MODE == 3) {
            float* o = out + ((size_t)n * M + m0 + 32 * wave) * V + v;
#pragma unroll
            for (int i = 0; i < 16; ++i) o[(size_t)mfma32_row(i, half) * V] = acc[c][i];
        } else if (MODE == 0) {
            float* o = out + ((size_t)n * M + m0 + 32 * wave) * V + v;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = mfma32_row(i, half);
                float val = acc[c][i] + bias[m0 + 32 * wave + row];
                if (relu) val = fmaxf(val, 0.0f);
                o[(size_t)row * V] = val;
            }
        } else {
            const int d = v / (Hv * Wv), r = v - d * Hv * Wv, h = r / Wv, w = r - h * Wv;
            const int Co = M / 8, H2 = 2 * H, W2 = 2 * W;
            const int o0 = (m0 + 32 * wave) / 8;          // four output channels per row tile
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const float b = bias[o0 + ch];
                float* o = out + (((size_t)n * Co + o0 + ch) * (2 * D) + 2 * d + half) * H2 * W2 + (size_t)(2 * h) * W2 + 2 * w;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    float a0 = acc[c][4 * ch + 2 * q] + b, a1 = acc[c][4 * ch + 2 * q + 1] + b;
                    if (relu) { a0 = fmaxf(a0, 0.0f); a1 = fmaxf(a1, 0.0f); }
                    *reinterpret_cast<float2*>(o + (size_t)q * W2) = make_float2(a0, a1);
                }
            }
        }
    }
}

// Weight gradients of the two layers: D[m][j] = sum_k A[m][k] B[j][k] over the voxels k = (n, v) of the coarse grid D x H x W,
// both operands activations (NCDHW fp32), cut into bf16 pieces on the way into the LDS:
//   MODE 0 (1x1x1 stride 2):  m = o, A = grad_out (N,M,D,H,W);  j = c, B = x (N,J,2D,2H,2W) at (2d, 2h, 2w)      -> dW (Cout, Cin)
//   MODE 1 (k2 s2 transposed): m = c, A = x (N,M,D,H,W);  j = 8 o + 4 p + 2 q + r, B = grad_out (N,J/8,2D,2H,2W) at (2d+p, 2h+q, 2w+r)
//                                                                                                                -> dW (Cin, Cout, 2,2,2)
// Block = 64 x 64 outputs, 4 waves of one 32 x 32 accumulator each; k in steps of 32 voxels, a thread stages 8 consecutive voxels of
// one A row and of one B row (a staging pass for both operands shares the voxel coordinates).  LDS image [row][k-group of 8] per
// piece, the k-group XOR-swizzled by (row >> 2) & 3 so that 16 consecutive rows of one k-group fill all 64 banks.  Split-K: block
// (tile, s) sums the steps of chunk s and writes partial[s] (or the output itself with one split); neck_gemm_dw_reduce_kernel adds
// the chunks in order 0, 1, ...: the same bits on every run.
constexpr int kNdT = 64, kNdBK = 32;

template <int MODE>
__global__ __launch_bounds__(kThreads) void neck_gemm_dw_bf16x3_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                       float* __restrict__ out, int M, int J, int N, int D, int H, int W,
                                                                       int steps_per_split) {
    __shared__ uint4 s_t[2][2][2][kNdT][4];   // [stage][operand A/B][piece][row][k-group (swizzled)]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_j = (J + kNdT - 1) / kNdT;
    const int m0 = (blockIdx.x / tiles_j) * kNdT, j0 = (blockIdx.x % tiles_j) * kNdT, split = blockIdx.y;
    const int V = D * H * W;
    const long long K = (long long)N * V;
    const long long kbeg = (long long)split * steps_per_split * kNdBK;
    const long long kend = kbeg + (long long)steps_per_split * kNdBK < K ? kbeg + (long long)steps_per_split * kNdBK : K;
    const int nsteps = kend > kbeg ? (int)((kend - kbeg + kNdBK - 1) / kNdBK) : 0;

    // staging duty: row r of both tiles, voxels 8 kg .. 8 kg + 7 of the step
    const int r = tid >> 2, kg = tid & 3, kgs = kg ^ ((r >> 2) & 3);
    const int am = min(m0 + r, M - 1), bj = min(j0 + r, J - 1);
    const bool a_ok = m0 + r < M, b_ok = j0 + r < J;
    const int Jc = MODE == 1 ? J / 8 : J;                      // channels of the B tensor
    const int bc = MODE == 1 ? bj >> 3 : bj;
    const int H2 = 2 * H, W2 = 2 * W;
    const size_t bplane = (size_t)8 * V;
    const size_t btap = MODE == 1 ? ((size_t)((bj >> 2) & 1) * H2 + ((bj >> 1) & 1)) * W2 + (bj & 1) : 0;
    float fa[8], fb[8];
    auto fetch = [&](int step) {
        long long k = kbeg + (long long)step * kNdBK + 8 * kg;
        int n = 0, d = 0, h = 0, w = 0;
        if (k < kend) {
            n = (int)(k / V);
            int v = (int)(k - (long long)n * V);
            d = v / (H * W);
            v -= d * H * W;
            h = v / W;
            w = v - h * W;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = k + i < kend;
            const size_t av = ((size_t)n * M + am) * V + ((size_t)d * H + h) * W + w;
            const size_t bv = ((size_t)n * Jc + bc) * bplane + ((size_t)2 * d * H2 + 2 * h) * W2 + 2 * w + btap;
            fa[i] = ok && a_ok ? a[av] : 0.0f;
            fb[i] = ok && b_ok ? b[bv] : 0.0f;
            if (++w == W) { w = 0; if (++h == H) { h = 0; if (++d == D) { d = 0; ++n; } } }
        }
    };
    auto put = [&](int buf) {
        u32x4 hi, mid;
        bf16x3_cut8(fa, hi, mid);
        s_t[buf][0][0][r][kgs] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        s_t[buf][0][1][r][kgs] = make_uint4(mid[0], mid[1], mid[2], mid[3]);
        bf16x3_cut8(fb, hi, mid);
        s_t[buf][1][0][r][kgs] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        s_t[buf][1][1][r][kgs] = make_uint4(mid[0], mid[1], mid[2], mid[3]);
    };

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    const int ar = 32 * (wave >> 1) + (lane & 31), br = 32 * (wave & 1) + (lane & 31);
    if (nsteps > 0) {
        fetch(0);
        put(0);
    }
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const int buf = st & 1;
        if (st + 1 < nsteps) fetch(st + 1);               // in flight under the MFMAs below
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int q = 2 * s + (lane >> 5);
            const bf16x8 Ah = __builtin_bit_cast(bf16x8, s_t[buf][0][0][ar][q ^ ((ar >> 2) & 3)]);
            const bf16x8 Am = __builtin_bit_cast(bf16x8, s_t[buf][0][1][ar][q ^ ((ar >> 2) & 3)]);
            const bf16x8 Bh = __builtin_bit_cast(bf16x8, s_t[buf][1][0][br][q ^ ((br >> 2) & 3)]);
            const bf16x8 Bm = __builtin_bit_cast(bf16x8, s_t[buf][1][1][br][q ^ ((br >> 2) & 3)]);
            bf16x3_mfma32(acc, Ah, Am, Bh, Bm);
        }
        if (st + 1 < nsteps) put(buf ^ 1);
        __syncthreads();
    }
    // column = lane & 31 (j), row = mfma32_row (m)
    const int j = j0 + 32 * (wave & 1) + (lane & 31);
    if (j >= J) return;
    float* o = out + (size_t)split * M * J;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = m0 + 32 * (wave >> 1) + mfma32_row(i, lane >> 5);
        if (m < M) o[(size_t)m * J + j] = acc[i];
    }
}

// out[i] = sum_s partial[s][i], s = 0, 1, ... in order
__global__ __launch_bounds__(kThreads) void neck_gemm_dw_reduce_kernel(const float* __restrict__ partial, float* __restrict__ out, size_t count,
                                                                       int nsplit) {
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += (size_t)gridDim.x * kThreads) {
        float s = partial[i];
        for (int p = 1; p < nsplit; ++p) s += partial[(size_t)p * count + i];
        out[i] = s;
    }
}

}  // namespace mvsdet

using namespace mvsdet;

extern "C" size_t mvsdet_gemm_split_weight_bytes(int M, int K) {
    if (M <= 0 || K <= 0 || M % kGemmBM || K % kGemmBK) return 0;
    return (size_t)(M / 32) * (K / 16) * 2 * 64 * 16;
}

extern "C" int mvsdet_gemm_split_weight(const float* wmat, void* wsplit, int M, int K, mvsdet_stream_t stream) {
    MVS_REQUIRE(wmat && wsplit, "gemm_split_weight: NULL pointer");
    MVS_REQUIRE(M > 0 && K > 0 && M % kGemmBM == 0 && K % kGemmBK == 0, "gemm_split_weight: M=%d must be a multiple of %d, K=%d of %d", M, kGemmBM, K, kGemmBK);
    MVS_REQUIRE(((uintptr_t)wsplit & 15u) == 0, "gemm_split_weight: wsplit must be 16-byte aligned");
    const size_t units = (size_t)(M / 32) * (K / 16) * 64;
    hipLaunchKernelGGL(gemm_split_weight_kernel, dim3((unsigned)((units + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       wmat, static_cast<uint4*>(wsplit), M, K);
    MVS_LAUNCH_CHECK("gemm_split_weight");
    return MVSDET_OK;
}

static int neck_gemm_check(const char* name, const void* x, const void* ws, const void* bias, const void* out, int N, int K, int M,
                           int D, int H, int W) {
    MVS_REQUIRE(x && ws && bias && out, "%s: NULL pointer", name);
    MVS_REQUIRE(N > 0 && N <= 65535 && D > 0 && H > 0 && W > 0, "%s: bad shape N=%d D=%d H=%d W=%d", name, N, D, H, W);
    MVS_REQUIRE(K > 0 && K % kGemmBK == 0 && M > 0 && M % kGemmBM == 0, "%s: Cin=%d must be a multiple of %d and the row count %d of %d", name, K,
                kGemmBK, M, kGemmBM);
    MVS_REQUIRE(M / kGemmBM <= 65535, "%s: too many rows", name);
    MVS_REQUIRE(((uintptr_t)ws & 15u) == 0 && ((uintptr_t)out & 7u) == 0, "%s: wsplit must be 16-byte, out 8-byte aligned", name);
    MVS_REQUIRE((long long)D * H * W < INT32_MAX / 8, "%s: volume too large", name);
    return MVSDET_OK;
}

extern "C" int mvsdet_conv3d_k1_s2_bf16x3(const float* x, const void* wsplit, const float* bias, float* out, int N, int Cin, int Cout,
                                          int D, int H, int W, int relu, mvsdet_stream_t stream) {
    if (int rc = neck_gemm_check("conv3d_k1_s2_bf16x3", x, wsplit, bias, out, N, Cin, Cout, D, H, W)) return rc;
    MVS_REQUIRE(D % 2 == 0 && H % 2 == 0 && W % 2 == 0, "conv3d_k1_s2_bf16x3: D, H, W must be even");
    const int V = (D / 2) * (H / 2) * (W / 2);
    dim3 grid((unsigned)((V + kGemmBN - 1) / kGemmBN), (unsigned)(Cout / kGemmBM), (unsigned)N);
    hipLaunchKernelGGL(neck_gemm_bf16x3_kernel<0>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, static_cast<const uint4*>(wsplit), bias,
                       out, Cout, Cin, D, H, W, relu);
    MVS_LAUNCH_CHECK("conv3d_k1_s2_bf16x3");
    return MVSDET_OK;
}

extern "C" int mvsdet_convT3d_k2_s2_bf16x3(const float* x, const void* wsplit, const float* bias, float* out, int N, int Cin, int Cout,
                                           int D, int H, int W, int relu, mvsdet_stream_t stream) {
    MVS_REQUIRE(Cout > 0 && Cout <= INT32_MAX / 8, "convT3d_k2_s2_bf16x3: bad Cout");
    if (int rc = neck_gemm_check("convT3d_k2_s2_bf16x3", x, wsplit, bias, out, N, Cin, 8 * Cout, D, H, W)) return rc;
    const int V = D * H * W;
    dim3 grid((unsigned)((V + kGemmBN - 1) / kGemmBN), (unsigned)(8 * Cout / kGemmBM), (unsigned)N);
    hipLaunchKernelGGL(neck_gemm_bf16x3_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, static_cast<const uint4*>(wsplit), bias,
                       out, 8 * Cout, Cin, D, H, W, relu);
    MVS_LAUNCH_CHECK("convT3d_k2_s2_bf16x3");
    return MVSDET_OK;
}

// ---------------------------------------------------------------------------------------------- training: gradients
// Input gradients: wsplit = mvsdet_gemm_split_weight of the (Cin, Cout) matrix W^T (shortcut) or of the (Cin, 8 Cout) matrix
// W.reshape(Cin, 8 Cout) (transposed layer, columns 8 o + 4 p + 2 q + r).
extern "C" int mvsdet_conv3d_k1_s2_dx_bf16x3(const float* grad_out, const void* wsplit, float* grad_x, int N, int Cin, int Cout, int D,
                                             int H, int W, mvsdet_stream_t stream) {
    const float* one = grad_out;   // the shared check asks for a bias pointer: none here
    if (int rc = neck_gemm_check("conv3d_k1_s2_dx_bf16x3", grad_out, wsplit, one, grad_x, N, Cout, Cin, D, H, W)) return rc;
    MVS_REQUIRE(D % 2 == 0 && H % 2 == 0 && W % 2 == 0, "conv3d_k1_s2_dx_bf16x3: D, H, W must be even");
    MVS_REQUIRE(((uintptr_t)grad_out & 3u) == 0 && ((uintptr_t)grad_x & 3u) == 0, "conv3d_k1_s2_dx_bf16x3: tensors must be 4-byte aligned");
    const int V = (D / 2) * (H / 2) * (W / 2);
    dim3 grid((unsigned)((V + kGemmBN - 1) / kGemmBN), (unsigned)(Cin / kGemmBM), (unsigned)N);
    hipLaunchKernelGGL(neck_gemm_bf16x3_kernel<2>, grid, dim3(kThreads), 0, (hipStream_t)stream, grad_out, static_cast<const uint4*>(wsplit),
                       nullptr, grad_x, Cin, Cout, D, H, W, 0);
    MVS_LAUNCH_CHECK("conv3d_k1_s2_dx_bf16x3");
    return MVSDET_OK;
}

extern "C" int mvsdet_convT3d_k2_s2_dx_bf16x3(const float* grad_out, const void* wsplit, float* grad_x, int N, int Cin, int Cout, int D,
                                              int H, int W, mvsdet_stream_t stream) {
    MVS_REQUIRE(Cout > 0 && Cout <= INT32_MAX / 8, "convT3d_k2_s2_dx_bf16x3: bad Cout");
    const float* one = grad_out;
    if (int rc = neck_gemm_check("convT3d_k2_s2_dx_bf16x3", grad_out, wsplit, one, grad_x, N, 8 * Cout, Cin, D, H, W)) return rc;
    MVS_REQUIRE((long long)8 * D * H * W < INT32_MAX / 8, "convT3d_k2_s2_dx_bf16x3: volume too large");
    const int V = D * H * W;
    dim3 grid((unsigned)((V + kGemmBN - 1) / kGemmBN), (unsigned)(Cin / kGemmBM), (unsigned)N);
    hipLaunchKernelGGL(neck_gemm_bf16x3_kernel<3>, grid, dim3(kThreads), 0, (hipStream_t)stream, grad_out, static_cast<const uint4*>(wsplit),
                       nullptr, grad_x, Cin, 8 * Cout, D, H, W, 0);
    MVS_LAUNCH_CHECK("convT3d_k2_s2_dx_bf16x3");
    return MVSDET_OK;
}

extern "C" size_t mvsdet_neck_gemm_dw_partial_bytes(int Cin, int Cout, int transposed, int nsplit) {
    if (Cin <= 0 || Cout <= 0 || nsplit <= 1 || Cout > INT32_MAX / 8) return 0;
    return (size_t)nsplit * Cin * Cout * (transposed ? 8 : 1) * sizeof(float);
}

// Weight gradients.  transposed = 0: x (N,Cin,2D,2H,2W), grad_out (N,Cout,D,H,W) -> dW (Cout, Cin) of the 1x1x1 stride-2 layer;
// transposed = 1: x (N,Cin,D,H,W), grad_out (N,Cout,2D,2H,2W) -> dW (Cin, Cout, 2, 2, 2) of ConvTranspose3d(k=2, s=2).  (D, H, W) is
// the coarse grid either way.  nsplit > 1: chunks of the voxels summed into `partial` (mvsdet_neck_gemm_dw_partial_bytes) and added
// in a fixed order.
extern "C" int mvsdet_neck_gemm_dw_bf16x3(const float* x, const float* grad_out, float* dw, float* partial, size_t partial_bytes, int nsplit,
                                          int transposed, int N, int Cin, int Cout, int D, int H, int W, mvsdet_stream_t stream) {
    MVS_REQUIRE(x && grad_out && dw, "neck_gemm_dw_bf16x3: NULL pointer");
    MVS_REQUIRE(transposed == 0 || transposed == 1, "neck_gemm_dw_bf16x3: transposed must be 0 or 1");
    MVS_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && D > 0 && H > 0 && W > 0, "neck_gemm_dw_bf16x3: bad shape N=%d Cin=%d Cout=%d D=%d H=%d W=%d",
                N, Cin, Cout, D, H, W);
    MVS_REQUIRE(Cout <= INT32_MAX / 8 && (long long)8 * D * H * W < INT32_MAX, "neck_gemm_dw_bf16x3: too large");
    MVS_REQUIRE(nsplit >= 1 && nsplit <= 65535, "neck_gemm_dw_bf16x3: nsplit=%d outside [1,65535]", nsplit);
    MVS_REQUIRE(((uintptr_t)x & 3u) == 0 && ((uintptr_t)grad_out & 3u) == 0 && ((uintptr_t)dw & 3u) == 0,
                "neck_gemm_dw_bf16x3: tensors must be 4-byte aligned");
    if (nsplit > 1) {
        MVS_REQUIRE(partial && ((uintptr_t)partial & 3u) == 0, "neck_gemm_dw_bf16x3: nsplit=%d needs a partial buffer", nsplit);
        const size_t need = mvsdet_neck_gemm_dw_partial_bytes(Cin, Cout, transposed, nsplit);
        if (partial_bytes < need) {
            set_error("neck_gemm_dw_bf16x3: partial buffer %zu B < %zu B", partial_bytes, need);
            return MVSDET_ERR_WORKSPACE;
        }
    }
    const int M = transposed ? Cin : Cout, J = transposed ? 8 * Cout : Cin;
    const long long tiles = (long long)((M + kNdT - 1) / kNdT) * ((J + kNdT - 1) / kNdT);
    MVS_REQUIRE(tiles < INT32_MAX, "neck_gemm_dw_bf16x3: too many tiles");
    const long long K = (long long)N * D * H * W;
    const long long steps = (K + kNdBK - 1) / kNdBK;
    const int per = (int)((steps + nsplit - 1) / nsplit);
    float* dst = nsplit > 1 ? partial : dw;
    dim3 grid((unsigned)tiles, (unsigned)nsplit);
    if (transposed)
        hipLaunchKernelGGL(neck_gemm_dw_bf16x3_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, grad_out, dst, M, J, N, D, H, W, per);
    else
        hipLaunchKernelGGL(neck_gemm_dw_bf16x3_kernel<0>, grid, dim3(kThreads), 0, (hipStream_t)stream, grad_out, x, dst, M, J, N, D, H, W, per);
    if (nsplit > 1) {
        const size_t count = (size_t)M * J;
        hipLaunchKernelGGL(neck_gemm_dw_reduce_kernel, dim3((unsigned)std::min<size_t>((count + kThreads - 1) / kThreads, 1024)), dim3(kThreads), 0,
                           (hipStream_t)stream, partial, dw, count, nsplit);
    }
    MVS_LAUNCH_CHECK("neck_gemm_dw_bf16x3");
    return MVSDET_OK;
}
