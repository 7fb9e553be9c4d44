// The Gaussian head of the novel-view branch: `to_gaussians` = nn.Sequential(ReLU, Linear) (mvsdet.py:210-216) on the rows that
// extract_feat concatenates per source pixel (:561-569: the chosen views' feature rows, depth_coding, and with use_rgb_gaussian the
// quarter-size image of process_rgb_raw, :319-333), without the row matrix:
//
//   raw[v][r][m] = bias[m] + sum_k weight[m][k] relu(x[k]),  x[k] = feature[ids[v]][k][y][x]            k < C
//                                                                   depth_coding[ids[v]][y][x]           k = C
//                                                                   rgb of channel k - C - 1             C < k < K  (K = C + 4)
//
// with r = y w + x over the cropped h x w map.  The rgb value is a precomputed row (V,R,3) or the mean of the four image pixels
// around source position 4 d + 1.5: 0.25 ((I[4y+1][4x+1] + I[4y+1][4x+2]) + (I[4y+2][4x+1] + I[4y+2][4x+2])), which is what
// F.interpolate(scale_factor=0.25, mode='bilinear') gives there.
//
// This is C[M][pixel] = A[M][K] B[K][pixel] with B = the activations as they lie in memory (an NCHW channel is a row of pixels), the
// form of neck_gemm.hip, but in exact fp32 on the matrix cores: v_mfma_f32_32x32x2_f32, lane l supplies A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31]; the products of one output are added in k order.  The bias is one more k with x = 1.
//
//   forward          block = 128 pixels of one view x 96 rows of M; wave = 32 pixels x 3 row tiles.  B: a plain global load, coalesced
//                    along the pixels, the channel index selecting the source, ReLU in the register.  A: 32 k of the weight rows at a
//                    time through the LDS, transposed so that a lane's m is adjacent.  A lane ends with runs of four m of its pixel.
//                    The next stage's weights and activations are fetched into registers under this stage's MFMAs.
//   input gradient   the same shape with A = weight^T (read in place: adjacent lanes, adjacent k), reducing over m; B = the rows of g,
//                    32 m at a time through the LDS (a block's rows are one contiguous piece of g).  Masked by x > 0, written
//                    pixel-contiguous into NCHW.  Only the selected views' cropped pixels are written.
//   weight gradient  D[m][k] = sum_pixels g[pixel][m] relu(x[k][pixel]): A = g read in place (adjacent lanes, adjacent m), B = x
//                    transposed through the LDS.  The pixels (v, r) are cut into chunks; block (k group, chunk) writes partial[chunk],
//                    gshead_reduce_kernel adds the chunks in order 0, 1, ...: no atomics, the same bits on every run.
//
// K + 1, M, R and the pixel tiles all have tails: they are zeros in registers / LDS, never a read past a row.  An id outside [0, N)
// reads nothing: that view's x is NaN (so is its raw), and it gets no gradient.
#include "common.h"
#include "mfma.h"

#include <algorithm>

namespace mvsdet {

constexpr int kGhKB = 32;        // k per LDS stage (16 MFMA steps)
constexpr int kGhRowTiles = 3;   // forward: row tiles of 32 m per block
constexpr int kGhRows = 32 * kGhRowTiles;
constexpr int kGhPix = 128;      // pixels per block, 32 per wave
constexpr int kGhDxTiles = 5;    // input gradient: tiles of 32 k per block
constexpr int kGhDwK = 128;      // weight gradient: k per block, 32 per wave

struct GhSrc {
    const float* feature;        // (N,C,Hf,Wf), w stride 1
    int64_t fN, fC, fH;
    const float* depth;          // (N,h,w) view, w stride 1
    int64_t dN, dH;
    const float* rgb_rows;       // (V,R,3) contiguous, or NULL
    const float* image;          // (N,3,Hi,Wi), w stride 1, or NULL
    int64_t iN, iC, iH;
    const int64_t* ids;          // (V) on the device
    int N, C, K, h, w, R;
};

// torch's relu: NaN stays NaN, -0.0 and 0.0 give 0
__device__ __forceinline__ float gh_relu(float x) { return x > 0.0f ? x : (x == x ? 0.0f : x); }

// x[k] of pixel (y, x) = r of view v (source view id; ok = id inside [0, N)), k <= K; before the ReLU.  k = K is the bias' 1.
__device__ __forceinline__ float gh_x(const GhSrc& s, int64_t id, bool ok, int v, int k, int r, int y, int x) {
    if (k >= s.K) return k == s.K ? 1.0f : 0.0f;
    if (!ok) return __builtin_nanf("");
    if (k < s.C) return s.feature[id * s.fN + (int64_t)k * s.fC + (int64_t)y * s.fH + x];
    if (k == s.C) return s.depth[id * s.dN + (int64_t)y * s.dH + x];
    const int c = k - s.C - 1;
    if (s.rgb_rows) return s.rgb_rows[((size_t)v * s.R + r) * 3 + c];
    const float* p = s.image + id * s.iN + (int64_t)c * s.iC + (int64_t)(4 * y + 1) * s.iH + (4 * x + 1);
    return 0.25f * ((p[0] + p[1]) + (p[s.iH] + p[s.iH + 1]));
}

__device__ __forceinline__ void gh_zero(f32x16& a) {
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.0f;
}

// ---------------------------------------------------------------------------------------------- forward
// grid (ceil(R / 128), ceil(M / 96), V)
__global__ __launch_bounds__(kThreads) void gshead_forward_kernel(GhSrc s, const float* __restrict__ weight, const float* __restrict__ bias,
                                                                  float* __restrict__ out, int M) {
    __shared__ float s_w[kGhKB][kGhRows + 1];   // [k of the stage][m of the block]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, col = lane & 31;
    const int v = blockIdx.z, m0 = blockIdx.y * kGhRows;
    const int r = blockIdx.x * kGhPix + 32 * wave + col;
    const int64_t id = s.ids[v];
    const bool ok = id >= 0 && id < s.N, in = r < s.R;
    const int y = in ? r / s.w : 0, x = in ? r - y * s.w : 0;
    const int K = s.K, Kt = K + 1;

    f32x16 acc[kGhRowTiles];
#pragma unroll
    for (int t = 0; t < kGhRowTiles; ++t) gh_zero(acc[t]);

    // a stage's operands in registers: wv = this thread's 12 weights of the LDS image, b = the lane's 16 activations
    float wv[kGhRows / 8], b[kGhKB / 2];
    auto fetch = [&](int k0) {
        const int k = k0 + (tid & 31);
#pragma unroll
        for (int i = 0; i < kGhRows / 8; ++i) {
            const int m = m0 + (tid >> 5) + 8 * i;
            float val = 0.0f;
            if (m < M && k < K) val = weight[(size_t)m * K + k];
            else if (m < M && k == K) val = bias[m];
            wv[i] = val;
        }
        if (in && k0 + kGhKB <= s.C) {                    // a stage of feature channels only
            const float* p = s.feature + id * s.fN + (int64_t)(k0 + half) * s.fC + (int64_t)y * s.fH + x;
#pragma unroll
            for (int st = 0; st < kGhKB / 2; ++st) b[st] = ok ? gh_relu(p[(int64_t)(2 * st) * s.fC]) : __builtin_nanf("");
        } else {
#pragma unroll
            for (int st = 0; st < kGhKB / 2; ++st) {
                const int kk = k0 + 2 * st + half;
                b[st] = in && kk <= K ? gh_relu(gh_x(s, id, ok, v, kk, r, y, x)) : 0.0f;
            }
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < Kt; k0 += kGhKB) {
        __syncthreads();                                  // the previous stage's readers are done
#pragma unroll
        for (int i = 0; i < kGhRows / 8; ++i) s_w[tid & 31][(tid >> 5) + 8 * i] = wv[i];
        float bc[kGhKB / 2];
#pragma unroll
        for (int st = 0; st < kGhKB / 2; ++st) bc[st] = b[st];
        __syncthreads();
        if (k0 + kGhKB < Kt) fetch(k0 + kGhKB);           // in flight under the MFMAs below
#pragma unroll
        for (int st = 0; st < kGhKB / 2; ++st) {
#pragma unroll
            for (int t = 0; t < kGhRowTiles; ++t) {
                if (m0 + 32 * t >= M) continue;           // a row tile past M: nothing to do (uniform)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[2 * st + half][32 * t + col], bc[st], acc[t], 0, 0, 0);
            }
        }
    }
    if (!in) return;
    // C map: column = lane & 31 (the pixel), row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5): four runs of four m
    float* o = out + ((size_t)v * s.R + r) * M;
#pragma unroll
    for (int t = 0; t < kGhRowTiles; ++t) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = m0 + 32 * t + 8 * q + 4 * half;
            if (m >= M) continue;
            if (m + 3 < M && (((uintptr_t)(o + m)) & 15u) == 0) {
                *reinterpret_cast<float4*>(o + m) = make_float4(acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (m + j < M) o[m + j] = acc[t][4 * q + j];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- the image form alone
// rows (V,R,3) = the four-pixel means of process_rgb_raw; one thread per (v, r, c)
__global__ __launch_bounds__(kThreads) void gshead_rgb_rows_kernel(GhSrc s, float* __restrict__ rows, int V) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (size_t)V * s.R * 3) return;
    const int c = (int)(i % 3);
    const size_t q = i / 3;
    const int v = (int)(q / s.R), r = (int)(q - (size_t)v * s.R);
    const int y = r / s.w, x = r - y * s.w;
    const int64_t id = s.ids[v];
    rows[i] = gh_x(s, id, id >= 0 && id < s.N, v, s.C + 1 + c, r, y, x);
}

// ---------------------------------------------------------------------------------------------- input gradient
// grid (ceil(R / 128), ceil((C + 1) / 160), V); g (V,R,M) contiguous
__global__ __launch_bounds__(kThreads) void gshead_backward_input_kernel(GhSrc s, const float* __restrict__ weight, const float* __restrict__ g,
                                                                         float* __restrict__ g_feature, int64_t gfN, int64_t gfC, int64_t gfH,
                                                                         float* __restrict__ g_depth, int64_t gdN, int64_t gdH, int M) {
    __shared__ float s_g[kGhKB][kGhPix + 1];    // [m of the stage][pixel of the block]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, col = lane & 31;
    const int v = blockIdx.z, k0 = blockIdx.y * (32 * kGhDxTiles), r0 = blockIdx.x * kGhPix;
    const int r = r0 + 32 * wave + col;
    const int64_t id = s.ids[v];
    if (id < 0 || id >= s.N) return;                     // uniform: a view that does not exist gets no gradient
    const int K = s.K, Kout = s.C + 1;

    f32x16 acc[kGhDxTiles];
#pragma unroll
    for (int t = 0; t < kGhDxTiles; ++t) gh_zero(acc[t]);

    for (int mb = 0; mb < M; mb += kGhKB) {
        __syncthreads();
        {
            const int m = mb + (tid & 31);
            for (int p = tid >> 5; p < kGhPix; p += kThreads / 32)
                s_g[tid & 31][p] = (m < M && r0 + p < s.R) ? g[((size_t)v * s.R + r0 + p) * M + m] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kGhDxTiles; ++t) {
            const int k = k0 + 32 * t + col;
            if (k0 + 32 * t >= Kout) continue;            // uniform
            float a[kGhKB / 2];
#pragma unroll
            for (int st = 0; st < kGhKB / 2; ++st) {
                const int m = mb + 2 * st + half;
                a[st] = (k < Kout && m < M) ? weight[(size_t)m * K + k] : 0.0f;
            }
#pragma unroll
            for (int st = 0; st < kGhKB / 2; ++st)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[st], s_g[2 * st + half][32 * wave + col], acc[t], 0, 0, 0);
        }
    }
    if (r >= s.R) return;
    const int y = r / s.w, x = r - y * s.w;
#pragma unroll
    for (int t = 0; t < kGhDxTiles; ++t) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int k = mfma32_row(i, half, k0 + 32 * t);
            if (k < s.C) {
                const float xv = s.feature[id * s.fN + (int64_t)k * s.fC + (int64_t)y * s.fH + x];
                g_feature[id * gfN + (int64_t)k * gfC + (int64_t)y * gfH + x] = xv > 0.0f ? acc[t][i] : 0.0f;
            } else if (k == s.C) {
                const float xv = s.depth[id * s.dN + (int64_t)y * s.dH + x];
                g_depth[id * gdN + (int64_t)y * gdH + x] = xv > 0.0f ? acc[t][i] : 0.0f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- weight gradient
// grid (ceil((K + 1) / 128), chunks, ceil(M / 96)); the pixels q = v R + r of chunk c are [c chunk, (c + 1) chunk), chunk % 32 == 0;
// partial (chunks, M, K + 1)
__global__ __launch_bounds__(kThreads) void gshead_backward_weight_kernel(GhSrc s, const float* __restrict__ g, float* __restrict__ partial,
                                                                          int M, int V, int chunk) {
    __shared__ float s_x[kGhDwK][kGhKB + 1];    // [k of the block][pixel of the stage]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, col = lane & 31;
    const int k0 = blockIdx.x * kGhDwK, m0 = blockIdx.z * kGhRows;
    const int K = s.K, Kt = K + 1;
    const long long P = (long long)V * s.R;
    const long long qbeg = (long long)blockIdx.y * chunk, qend = qbeg + chunk < P ? qbeg + chunk : P;

    f32x16 acc[kGhRowTiles];
#pragma unroll
    for (int t = 0; t < kGhRowTiles; ++t) gh_zero(acc[t]);

    for (long long q0 = qbeg; q0 < qend; q0 += kGhKB) {
        float a[kGhRowTiles][kGhKB / 2];
#pragma unroll
        for (int t = 0; t < kGhRowTiles; ++t) {
            const int m = m0 + 32 * t + col;
#pragma unroll
            for (int st = 0; st < kGhKB / 2; ++st) {
                const long long q = q0 + 2 * st + half;
                a[t][st] = (m < M && q < qend) ? g[(size_t)q * M + m] : 0.0f;
            }
        }
        __syncthreads();
        {
            const long long q = q0 + (tid & 31);          // this thread's pixel of the stage
            const bool in = q < qend;
            const int v = in ? (int)(q / s.R) : 0, r = in ? (int)(q - (long long)v * s.R) : 0;
            const int y = r / s.w, x = r - y * s.w;
            const int64_t id = s.ids[v];
            const bool ok = id >= 0 && id < s.N;
            if (k0 + kGhDwK <= s.C) {                     // a block of feature channels only (uniform): 16 loads in flight
                const float* p = s.feature + id * s.fN + (int64_t)(k0 + (tid >> 5)) * s.fC + (int64_t)y * s.fH + x;
                float xv[kGhDwK / 8];
#pragma unroll
                for (int i = 0; i < kGhDwK / 8; ++i) xv[i] = !in ? 0.0f : ok ? gh_relu(p[(int64_t)(8 * i) * s.fC]) : __builtin_nanf("");
#pragma unroll
                for (int i = 0; i < kGhDwK / 8; ++i) s_x[(tid >> 5) + 8 * i][tid & 31] = xv[i];
            } else {
                const int live = min(kGhDwK, Kt - k0);    // the rows of s_x that a wave of this block reads are below 32 ceil(live / 32)
                for (int kk = tid >> 5; kk < (live + 31) / 32 * 32; kk += kThreads / 32) {
                    const int k = k0 + kk;
                    s_x[kk][tid & 31] = in && k <= K ? gh_relu(gh_x(s, id, ok, v, k, r, y, x)) : 0.0f;
                }
            }
        }
        __syncthreads();
        if (k0 + 32 * wave >= Kt) continue;               // uniform per wave; the barriers above are passed by everyone
#pragma unroll
        for (int st = 0; st < kGhKB / 2; ++st) {
            const float bx = s_x[32 * wave + col][2 * st + half];
#pragma unroll
            for (int t = 0; t < kGhRowTiles; ++t) {
                if (m0 + 32 * t >= M) continue;
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][st], bx, acc[t], 0, 0, 0);
            }
        }
    }
    const int k = k0 + 32 * wave + col;
    if (k >= Kt) return;
    float* o = partial + (size_t)blockIdx.y * M * Kt;
#pragma unroll
    for (int t = 0; t < kGhRowTiles; ++t) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = mfma32_row(i, half, m0 + 32 * t);
            if (m < M) o[(size_t)m * Kt + k] = acc[t][i];
        }
    }
}

// g_weight[m][k] / g_bias[m] = sum_c partial[c][m][k], c = 0, 1, ... in order
__global__ __launch_bounds__(kThreads) void gshead_reduce_kernel(const float* __restrict__ partial, float* __restrict__ g_weight,
                                                                 float* __restrict__ g_bias, int M, int K, int chunks) {
    const size_t count = (size_t)M * (K + 1);
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += (size_t)gridDim.x * kThreads) {
        float sum = partial[i];
        int c = 1;
        for (; c + 8 <= chunks; c += 8) {               // eight loads in flight, added in chunk order all the same
            float t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = partial[(size_t)(c + j) * count + i];
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += t[j];
        }
        for (; c < chunks; ++c) sum += partial[(size_t)c * count + i];
        const int m = (int)(i / (K + 1)), k = (int)(i - (size_t)m * (K + 1));
        if (k < K) g_weight[(size_t)m * K + k] = sum;
        else g_bias[m] = sum;
    }
}

}  // namespace mvsdet

using namespace mvsdet;

static const int kGhDefaultChunk = 256;

// the shared argument check; fills `s`.  The largest element offset of every tensor must fit the 64-bit arithmetic of the kernels
// without overflow: strides and extents are bounded so that their products stay below 2^62.
static int gshead_source(const char* name, GhSrc& s, const float* feature, const int64_t* fs, const float* depth, const int64_t* ds,
                         const float* rgb_rows, const float* image, const int64_t* is, const int64_t* ids, int N, int V, int C, int K, int h,
                         int w, int Hf, int Wf, int Hi, int Wi) {
    MVS_REQUIRE(feature && fs && depth && ds && ids, "%s: NULL pointer", name);
    MVS_REQUIRE(N > 0 && V > 0 && V <= 65535 && C > 0 && h > 0 && w > 0 && h <= Hf && w <= Wf,
                "%s: bad shape N=%d V=%d C=%d map %dx%d of %dx%d (V <= 65535, h <= Hf, w <= Wf)", name, N, V, C, h, w, Hf, Wf);
    MVS_REQUIRE((long long)h * w < INT32_MAX / 4, "%s: map %dx%d too large", name, h, w);
    MVS_REQUIRE(!(rgb_rows && image), "%s: rgb comes as rows or as images, not both", name);
    const bool rgb = rgb_rows || image;
    MVS_REQUIRE(K == C + (rgb ? 4 : 1), "%s: K=%d must be C + %d = %d %s rgb", name, K, rgb ? 4 : 1, C + (rgb ? 4 : 1), rgb ? "with" : "without");
    const int64_t lim = (int64_t)1 << 40;
    MVS_REQUIRE(fs[0] >= 0 && fs[1] >= 0 && fs[2] >= 0 && fs[0] < lim && fs[1] < lim && fs[2] < lim && ds[0] >= 0 && ds[1] >= 0 &&
                    ds[0] < lim && ds[1] < lim,
                "%s: feature / depth_coding strides must lie in [0, 2^40)", name);
    if (image) {
        MVS_REQUIRE(is, "%s: NULL image strides", name);
        MVS_REQUIRE(Hi >= 4 * h - 1 && Wi >= 4 * w - 1, "%s: images %dx%d are smaller than 4 x the %dx%d map - 1 (only ratio 4)", name, Hi, Wi, h, w);
        MVS_REQUIRE(is[0] >= 0 && is[1] >= 0 && is[2] >= 0 && is[0] < lim && is[1] < lim && is[2] < lim, "%s: image strides must lie in [0, 2^40)",
                    name);
    }
    MVS_REQUIRE(((uintptr_t)feature & 3u) == 0 && ((uintptr_t)depth & 3u) == 0 && ((uintptr_t)rgb_rows & 3u) == 0 && ((uintptr_t)image & 3u) == 0 &&
                    ((uintptr_t)ids & 7u) == 0,
                "%s: tensors must be 4-byte, ids 8-byte aligned", name);
    s.feature = feature; s.fN = fs[0]; s.fC = fs[1]; s.fH = fs[2];
    s.depth = depth; s.dN = ds[0]; s.dH = ds[1];
    s.rgb_rows = rgb_rows;
    s.image = image; s.iN = image ? is[0] : 0; s.iC = image ? is[1] : 0; s.iH = image ? is[2] : 0;
    s.ids = ids;
    s.N = N; s.C = C; s.K = K; s.h = h; s.w = w; s.R = h * w;
    return MVSDET_OK;
}

extern "C" int mvsdet_gshead_forward_f32(const float* feature, const int64_t* feature_strides, const float* depth_coding,
                                         const int64_t* depth_strides, const float* rgb_rows, const float* images, const int64_t* image_strides,
                                         const int64_t* ids, const float* weight, const float* bias, float* raw, int N, int V, int C, int K,
                                         int M, int h, int w, int Hf, int Wf, int Hi, int Wi, mvsdet_stream_t stream) {
    GhSrc s;
    MVS_TRY(gshead_source("gshead_forward", s, feature, feature_strides, depth_coding, depth_strides, rgb_rows, images, image_strides, ids, N, V,
                          C, K, h, w, Hf, Wf, Hi, Wi));
    MVS_REQUIRE(weight && bias && raw, "gshead_forward: NULL pointer");
    MVS_REQUIRE(M > 0 && (M + kGhRows - 1) / kGhRows <= 65535, "gshead_forward: bad M=%d", M);
    MVS_REQUIRE(((uintptr_t)weight & 3u) == 0 && ((uintptr_t)bias & 3u) == 0 && ((uintptr_t)raw & 3u) == 0, "gshead_forward: tensors must be 4-byte aligned");
    dim3 grid((unsigned)((s.R + kGhPix - 1) / kGhPix), (unsigned)((M + kGhRows - 1) / kGhRows), (unsigned)V);
    hipLaunchKernelGGL(gshead_forward_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, s, weight, bias, raw, M);
    MVS_LAUNCH_CHECK("gshead_forward");
    return MVSDET_OK;
}

extern "C" int mvsdet_gshead_rgb_rows_f32(const float* images, const int64_t* image_strides, const int64_t* ids, float* rows, int N, int V, int h,
                                          int w, int Hi, int Wi, mvsdet_stream_t stream) {
    MVS_REQUIRE(images && image_strides && ids && rows, "gshead_rgb_rows: NULL pointer");
    MVS_REQUIRE(N > 0 && V > 0 && h > 0 && w > 0 && (long long)h * w < INT32_MAX / 4, "gshead_rgb_rows: bad shape N=%d V=%d map %dx%d", N, V, h, w);
    MVS_REQUIRE(Hi >= 4 * h - 1 && Wi >= 4 * w - 1, "gshead_rgb_rows: images %dx%d are smaller than 4 x the %dx%d map - 1 (only ratio 4)", Hi, Wi,
                h, w);
    const int64_t lim = (int64_t)1 << 40;
    MVS_REQUIRE(image_strides[0] >= 0 && image_strides[1] >= 0 && image_strides[2] >= 0 && image_strides[0] < lim && image_strides[1] < lim &&
                    image_strides[2] < lim,
                "gshead_rgb_rows: image strides must lie in [0, 2^40)");
    MVS_REQUIRE(((uintptr_t)images & 3u) == 0 && ((uintptr_t)rows & 3u) == 0 && ((uintptr_t)ids & 7u) == 0,
                "gshead_rgb_rows: tensors must be 4-byte, ids 8-byte aligned");
    GhSrc s = {};
    s.image = images; s.iN = image_strides[0]; s.iC = image_strides[1]; s.iH = image_strides[2];
    s.ids = ids;
    s.N = N; s.C = 0; s.K = 4; s.h = h; s.w = w; s.R = h * w;
    const long long total = (long long)V * s.R * 3;
    MVS_REQUIRE(blocks_of(total) < INT32_MAX, "gshead_rgb_rows: too many rows");
    hipLaunchKernelGGL(gshead_rgb_rows_kernel, dim3((unsigned)blocks_of(total)), dim3(kThreads), 0, (hipStream_t)stream, s, rows, V);
    MVS_LAUNCH_CHECK("gshead_rgb_rows");
    return MVSDET_OK;
}

extern "C" int mvsdet_gshead_backward_input_f32(const float* feature, const int64_t* feature_strides, const float* depth_coding,
                                                const int64_t* depth_strides, const int64_t* ids, const float* weight, const float* g,
                                                float* g_feature, const int64_t* g_feature_strides, float* g_depth_coding,
                                                const int64_t* g_depth_strides, int N, int V, int C, int K, int M, int h, int w, int Hf, int Wf,
                                                mvsdet_stream_t stream) {
    GhSrc s;
    MVS_REQUIRE(K == C + 1 || K == C + 4, "gshead_backward_input: K=%d must be C + 1 or C + 4 (C=%d)", K, C);
    // the rgb columns carry no gradient: the source is described without them, K stays the weight's row length
    MVS_TRY(gshead_source("gshead_backward_input", s, feature, feature_strides, depth_coding, depth_strides, nullptr, nullptr, nullptr, ids, N, V,
                          C, C + 1, h, w, Hf, Wf, 0, 0));
    s.K = K;
    MVS_REQUIRE(weight && g && g_feature && g_feature_strides && g_depth_coding && g_depth_strides, "gshead_backward_input: NULL pointer");
    MVS_REQUIRE(M > 0, "gshead_backward_input: bad M=%d", M);
    const int64_t lim = (int64_t)1 << 40;
    for (int i = 0; i < 3; ++i)
        MVS_REQUIRE(g_feature_strides[i] >= 0 && g_feature_strides[i] < lim, "gshead_backward_input: g_feature strides must lie in [0, 2^40)");
    for (int i = 0; i < 2; ++i)
        MVS_REQUIRE(g_depth_strides[i] >= 0 && g_depth_strides[i] < lim, "gshead_backward_input: g_depth_coding strides must lie in [0, 2^40)");
    MVS_REQUIRE(((uintptr_t)weight & 3u) == 0 && ((uintptr_t)g & 3u) == 0 && ((uintptr_t)g_feature & 3u) == 0 && ((uintptr_t)g_depth_coding & 3u) == 0,
                "gshead_backward_input: tensors must be 4-byte aligned");
    const int per = 32 * kGhDxTiles;
    MVS_REQUIRE((C + 1 + per - 1) / per <= 65535, "gshead_backward_input: too many channels");
    dim3 grid((unsigned)((s.R + kGhPix - 1) / kGhPix), (unsigned)((C + 1 + per - 1) / per), (unsigned)V);
    hipLaunchKernelGGL(gshead_backward_input_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, s, weight, g, g_feature, g_feature_strides[0],
                       g_feature_strides[1], g_feature_strides[2], g_depth_coding, g_depth_strides[0], g_depth_strides[1], M);
    MVS_LAUNCH_CHECK("gshead_backward_input");
    return MVSDET_OK;
}

static int gshead_chunk(int chunk_pixels) { return chunk_pixels > 0 ? (chunk_pixels + kGhKB - 1) / kGhKB * kGhKB : kGhDefaultChunk; }

extern "C" size_t mvsdet_gshead_partial_bytes(int V, int R, int M, int K, int chunk_pixels) {
    if (V <= 0 || R <= 0 || M <= 0 || K <= 0 || chunk_pixels < 0 || chunk_pixels > (1 << 24)) return 0;
    const long long P = (long long)V * R, chunk = gshead_chunk(chunk_pixels);
    return (size_t)((P + chunk - 1) / chunk) * M * ((size_t)K + 1) * sizeof(float);
}

extern "C" int mvsdet_gshead_backward_weight_f32(const float* feature, const int64_t* feature_strides, const float* depth_coding,
                                                 const int64_t* depth_strides, const float* rgb_rows, const float* images,
                                                 const int64_t* image_strides, const int64_t* ids, const float* g, float* g_weight, float* g_bias,
                                                 float* partial, size_t partial_bytes, int chunk_pixels, int N, int V, int C, int K, int M, int h,
                                                 int w, int Hf, int Wf, int Hi, int Wi, mvsdet_stream_t stream) {
    GhSrc s;
    MVS_TRY(gshead_source("gshead_backward_weight", s, feature, feature_strides, depth_coding, depth_strides, rgb_rows, images, image_strides, ids,
                          N, V, C, K, h, w, Hf, Wf, Hi, Wi));
    MVS_REQUIRE(g && g_weight && g_bias && partial, "gshead_backward_weight: NULL pointer");
    MVS_REQUIRE(M > 0 && (M + kGhRows - 1) / kGhRows <= 65535, "gshead_backward_weight: bad M=%d", M);
    MVS_REQUIRE(chunk_pixels >= 0 && chunk_pixels <= (1 << 24), "gshead_backward_weight: chunk_pixels=%d outside [0, 2^24]", chunk_pixels);
    MVS_REQUIRE(((uintptr_t)g & 3u) == 0 && ((uintptr_t)g_weight & 3u) == 0 && ((uintptr_t)g_bias & 3u) == 0 && ((uintptr_t)partial & 3u) == 0,
                "gshead_backward_weight: tensors must be 4-byte aligned");
    const int chunk = gshead_chunk(chunk_pixels);
    const long long P = (long long)V * s.R, chunks = (P + chunk - 1) / chunk;
    MVS_REQUIRE(chunks <= 65535, "gshead_backward_weight: %lld chunks of %d pixels (at most 65535): raise chunk_pixels", chunks, chunk);
    MVS_REQUIRE_WORKSPACE("gshead_backward_weight", partial_bytes, mvsdet_gshead_partial_bytes(V, s.R, M, K, chunk_pixels));
    dim3 grid((unsigned)((K + 1 + kGhDwK - 1) / kGhDwK), (unsigned)chunks, (unsigned)((M + kGhRows - 1) / kGhRows));
    hipLaunchKernelGGL(gshead_backward_weight_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, s, g, partial, M, V, chunk);
    const size_t count = (size_t)M * (K + 1);
    hipLaunchKernelGGL(gshead_reduce_kernel, dim3((unsigned)std::min<size_t>((count + kThreads - 1) / kThreads, 1024)), dim3(kThreads), 0,
                       (hipStream_t)stream, partial, g_weight, g_bias, M, K, (int)chunks);
    MVS_LAUNCH_CHECK("gshead_backward_weight");
    return MVSDET_OK;
}
