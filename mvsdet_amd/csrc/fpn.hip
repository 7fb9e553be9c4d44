// Level 0 of the 2-D feature pyramid that feeds the sweep (mvsdet.py:374-376: `x = self.neck(x)[0]`) on the bf16 matrix cores with
// three-term split operands: the hi / mid cut, the three products and the laterals' GEMM block are mfma.h's, shared with neck_gemm.hip.
//
// The module is mmdet.models.necks.FPN in the shipped configuration (in_channels=[256,512,1024,2048], out_channels=256, num_outs=4,
// start_level=0, no add_extra_convs, no norm, no activation, upsample_cfg=dict(mode='nearest')).  mmdet is not part of this tree; the
// definition is the builder's reading of that module:
//
//   L3 = lat3(c5)                                  lat_i: 1x1 convolution with bias
//   L2 = lat2(c4) + up(L3 -> size of c4)           up: F.interpolate(size=..., mode='nearest')
//   L1 = lat1(c3) + up(L2 -> size of c3)
//   L0 = lat0(c2) + up(L1 -> size of c2)
//   out0 = conv3x3(L0), padding 1, with bias       == FPN(inputs)[0]
//
// MVSDet keeps only out0: the 3x3 output convolutions of levels 1-3 are not computed.  `up` goes by SIZE: the source index is ATen's
// float32 computation min((int)floorf(dst * ((float)in / (float)out)), in - 1) (the integer form dst*in/out differs from it for
// 88 pairs in <= out < 130, e.g. 46 <- 14); the two scales are divided on the host and handed to the kernel.
//
// fpn_lateral_kernel: C[256][v] = W[256][Cin] x[Cin][v] + bias [+ top at the nearest source index], the plain sibling of
//   neck_gemm_bf16x3_kernel MODE 0 on the same gemm_bf16x3_block (128 rows x 64 columns, A from L2 in mvsdet_gemm_split_weight's
//   fragment order).  The columns run over ALL views' pixels, v = n H W + pixel: the 8x10 level of 40 views is 3200 columns = 50 full
//   blocks, not 40 x two blocks of which the second is three quarters empty.
//
// fpn_conv3x3_kernel: implicit GEMM, M = Cout, K = 9 Cin tap-major (k = Cin tap + c, tap = 3 dy + dx; the matrix is
//   w.permute(0,2,3,1).reshape(Cout, 9 Cin)).  Block = 128 rows x a tile of kFcTW x kFcTH = 16 x 8 pixels of one view, 4 waves of 32
//   rows x four 32-pixel accumulators (accumulator t = tile rows 2t, 2t+1).  Per 32 input channels the block stages the HALO tile
//   (18 x 10 pixels, zero outside the map) ONCE, cut into bf16 hi / mid, as [piece][k-group of 8][halo pixel] 16-byte units; the nine
//   taps read their B fragments from it at shifted addresses (16 consecutive lanes = 256 consecutive bytes: conflict-free), so an
//   input value is fetched and cut once per block, not nine times.  Two stages (2 x 22.5 KiB): the next 32 channels are fetched into
//   registers under this chunk's 216 MFMAs per wave.  The epilogue writes fp32 NCHW and / or the packed maps: a lane's sixteen rows
//   mfma32_row(i, lane >> 5) = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) of a 32-row tile are, for each i & 3, the four channels 8 i' + g (g = (i & 3) + 4 (lane >> 5))
//   = packed q = 4 g .. 4 g + 3: one 16-byte store per (i & 3), no shuffle.
//
// No atomics: the same bits on every run.
#include "common.h"
#include "mfma.h"

namespace mvsdet {

constexpr int kFcTW = 16, kFcTH = 8;                        // the 3x3 kernel's pixel tile
constexpr int kFcHW = kFcTW + 2, kFcHH = kFcTH + 2;          // its halo tile
constexpr int kFcHalo = kFcHW * kFcHH;                       // 180 halo pixels
constexpr int kFcUnits = 4 * kFcHalo;                        // (k-group of 8, halo pixel) staging units per 32 channels
constexpr int kFcRounds = (kFcUnits + kThreads - 1) / kThreads;

// ATen's nearest source index (UpSample.h: nearest_neighbor_compute_source_index), scale = (float)in / (float)out
__device__ __forceinline__ int fp_nearest(int dst, float scale, int in) { return min((int)floorf((float)dst * scale), in - 1); }

// x (N,K,H,W), out (N,M,H,W), top (N,M,Ht,Wt) or NULL; columns v = n HW + pixel, V = N HW of them
__global__ __launch_bounds__(kThreads) void fpn_lateral_kernel(const float* __restrict__ x, const uint4* __restrict__ ws,
                                                               const float* __restrict__ bias, const float* __restrict__ top,
                                                               float* __restrict__ out, int M, int K, int HW, int W, int V, int Ht, int Wt,
                                                               float scale_h, float scale_w) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.y * kGemmBM, v0 = blockIdx.x * kGemmBN;

    // staging duty: column v0 + (tid & 63), channels 8 * (tid >> 6) .. + 7 of the step
    const int sv = v0 + (tid & 63), skq = tid >> 6;
    const bool sv_ok = sv < V;
    const int sn = sv_ok ? sv / HW : 0, spix = sv_ok ? sv - sn * HW : 0;
    const float* xs = x + ((size_t)sn * K + 8 * skq) * HW + spix;
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

    // ---- epilogue: + bias [+ top at the nearest source pixel]
    const int half = lane >> 5;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int v = v0 + 32 * c + (lane & 31);
        if (v >= V) continue;
        const int n = v / HW, pix = v - n * HW;
        float* o = out + ((size_t)n * M + m0 + 32 * wave) * HW + pix;
        const float* t = nullptr;
        size_t tplane = 0;
        if (top) {
            const int y = pix / W, xx = pix - y * W;
            tplane = (size_t)Ht * Wt;
            t = top + ((size_t)n * M + m0 + 32 * wave) * tplane + (size_t)fp_nearest(y, scale_h, Ht) * Wt + fp_nearest(xx, scale_w, Wt);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = mfma32_row(i, half);
            float val = acc[c][i] + bias[m0 + 32 * wave + row];
            if (t) val += t[(size_t)row * tplane];
            o[(size_t)row * HW] = val;
        }
    }
}

// x (N,Cin,H,W), ws = split (M, 9 Cin) tap-major matrix, out (N,M,H,W) or NULL, packed (N, M/32, H W, 32) or NULL
__global__ __launch_bounds__(kThreads) void fpn_conv3x3_kernel(const float* __restrict__ x, const uint4* __restrict__ ws,
                                                               const float* __restrict__ bias, float* __restrict__ out,
                                                               float* __restrict__ packed, int M, int Cin, int H, int W, int tiles_x) {
    __shared__ uint4 s_h[2][2][4][kFcHalo];   // [stage][piece][k-group of 8][halo pixel]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.z, m0 = blockIdx.y * kGemmBM;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kFcTH, x0 = tx * kFcTW;
    const size_t HW = (size_t)H * W;

    // staging duties: unit u = tid + kThreads r -> k-group u / 180, halo pixel u % 180 (zero outside the map)
    const float* xn = x + (size_t)n * Cin * HW;
    size_t soff[kFcRounds];
    bool sok[kFcRounds];
    int skq[kFcRounds], shp[kFcRounds];
#pragma unroll
    for (int r = 0; r < kFcRounds; ++r) {
        const int u = tid + kThreads * r;
        const int kq = u / kFcHalo, hp = u - kq * kFcHalo;
        const int hy = hp / kFcHW, hx = hp - hy * kFcHW;
        const int y = y0 - 1 + hy, xx = x0 - 1 + hx;
        skq[r] = kq;
        shp[r] = hp;
        sok[r] = u < kFcUnits && y >= 0 && y < H && xx >= 0 && xx < W;
        soff[r] = sok[r] ? (size_t)(8 * kq) * HW + (size_t)y * W + xx : 0;
    }
    float f[kFcRounds][8];
    auto fetch = [&](int chunk) {
        const float* xc = xn + (size_t)(chunk * kGemmBK) * HW;
#pragma unroll
        for (int r = 0; r < kFcRounds; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) f[r][j] = sok[r] ? xc[soff[r] + (size_t)j * HW] : 0.0f;
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int r = 0; r < kFcRounds; ++r) {
            if (tid + kThreads * r < kFcUnits) {
                u32x4 hi, mid;
                bf16x3_cut8(f[r], hi, mid);
                s_h[buf][0][skq[r]][shp[r]] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
                s_h[buf][1][skq[r]][shp[r]] = make_uint4(mid[0], mid[1], mid[2], mid[3]);
            }
        }
    };

    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    const int rt = (m0 >> 5) + wave;                       // the wave's row tile
    const int K16 = 9 * Cin / 16;
    const uint4* wa = ws + (size_t)rt * K16 * 2 * 64 + lane;
    // the lane's pixel inside accumulator t: tile row 2 t + ly, column lx; its halo pixel under tap (dy, dx) is hbase + t 2 kFcHW + dy kFcHW + dx
    const int lx = lane & 15, ly = (lane >> 4) & 1, half = lane >> 5;
    const int hbase = ly * kFcHW + lx;
    const int nch = Cin / kGemmBK;
    fetch(0);
    put(0);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nch) fetch(ch + 1);                   // in flight under the nine taps below
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap - 3 * dy;
            const int k16 = (tap * Cin + ch * kGemmBK) / 16;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 Ah = __builtin_bit_cast(bf16x8, wa[((size_t)(k16 + s) * 2 + 0) * 64]);
                const bf16x8 Am = __builtin_bit_cast(bf16x8, wa[((size_t)(k16 + s) * 2 + 1) * 64]);
                const int kq = 2 * s + half;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int hp = hbase + (2 * t + dy) * kFcHW + dx;
                    const bf16x8 Bh = __builtin_bit_cast(bf16x8, s_h[buf][0][kq][hp]);
                    const bf16x8 Bm = __builtin_bit_cast(bf16x8, s_h[buf][1][kq][hp]);
                    bf16x3_mfma32(acc[t], Ah, Am, Bh, Bm);
                }
            }
        }
        if (ch + 1 < nch) put(buf ^ 1);                    // the other stage: its readers finished before the last barrier
        __syncthreads();
    }

    // ---- epilogue: + bias; fp32 NCHW rows and / or packed lines
    const int mw = m0 + 32 * wave;
    float b[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = bias[mw + mfma32_row(i, half)];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int y = y0 + 2 * t + ly, xx = x0 + lx;
        if (y >= H || xx >= W) continue;
        const size_t pix = (size_t)y * W + xx;
        if (out) {
            float* o = out + ((size_t)n * M + mw) * HW + pix;
#pragma unroll
            for (int i = 0; i < 16; ++i) o[(size_t)mfma32_row(i, half) * HW] = acc[t][i] + b[i];
        }
        if (packed) {   // slab mw / 32; registers a, a + 4, a + 8, a + 12 are channels 8 i' + g of the slab, g = a + 4 half: q = 4 g + i'
            float* p = packed + (((size_t)n * (M / 32) + (mw >> 5)) * HW + pix) * 32 + 16 * half;
#pragma unroll
            for (int a = 0; a < 4; ++a)
                *reinterpret_cast<float4*>(p + 4 * a) =
                    make_float4(acc[t][a] + b[a], acc[t][a + 4] + b[a + 4], acc[t][a + 8] + b[a + 8], acc[t][a + 12] + b[a + 12]);
        }
    }
}

}  // namespace mvsdet

using namespace mvsdet;

extern "C" int mvsdet_fpn_lateral_bf16x3(const float* x, const void* wsplit, const float* bias, const float* top, float* out, int N,
                                         int Cin, int Cout, int H, int W, int Ht, int Wt, mvsdet_stream_t stream) {
    MVS_REQUIRE(x && wsplit && bias && out, "fpn_lateral_bf16x3: NULL pointer");
    MVS_REQUIRE(N > 0 && H > 0 && W > 0, "fpn_lateral_bf16x3: bad shape N=%d H=%d W=%d", N, H, W);
    MVS_REQUIRE(Cin > 0 && Cin % kGemmBK == 0 && Cout > 0 && Cout % kGemmBM == 0, "fpn_lateral_bf16x3: Cin=%d must be a multiple of %d and Cout=%d of %d",
                Cin, kGemmBK, Cout, kGemmBM);
    MVS_REQUIRE(Cout / kGemmBM <= 65535, "fpn_lateral_bf16x3: too many rows");
    MVS_REQUIRE((long long)N * H * W <= INT32_MAX - kGemmBN, "fpn_lateral_bf16x3: N H W = %lld columns exceed 2^31", (long long)N * H * W);
    MVS_REQUIRE(((uintptr_t)wsplit & 15u) == 0 && ((uintptr_t)x & 3u) == 0 && ((uintptr_t)out & 3u) == 0 && ((uintptr_t)bias & 3u) == 0,
                "fpn_lateral_bf16x3: wsplit must be 16-byte, the tensors 4-byte aligned");
    if (top) {
        MVS_REQUIRE(Ht >= 1 && Ht <= H && Wt >= 1 && Wt <= W, "fpn_lateral_bf16x3: the top level %d x %d must lie within 1 x 1 .. %d x %d", Ht, Wt,
                    H, W);
        MVS_REQUIRE(((uintptr_t)top & 3u) == 0, "fpn_lateral_bf16x3: top must be 4-byte aligned");
    } else {
        Ht = Wt = 1;
    }
    const int V = N * H * W;
    dim3 grid((unsigned)((V + kGemmBN - 1) / kGemmBN), (unsigned)(Cout / kGemmBM));
    hipLaunchKernelGGL(fpn_lateral_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, x, static_cast<const uint4*>(wsplit), bias, top, out, Cout,
                       Cin, H * W, W, V, Ht, Wt, (float)Ht / (float)H, (float)Wt / (float)W);
    MVS_LAUNCH_CHECK("fpn_lateral_bf16x3");
    return MVSDET_OK;
}

extern "C" int mvsdet_fpn_conv3x3_bf16x3(const float* x, const void* wsplit, const float* bias, float* out, float* packed, int N, int Cin,
                                         int Cout, int H, int W, mvsdet_stream_t stream) {
    MVS_REQUIRE(x && wsplit && bias, "fpn_conv3x3_bf16x3: NULL pointer");
    MVS_REQUIRE(out || packed, "fpn_conv3x3_bf16x3: NULL pointer: at least one of out and packed must be given");
    MVS_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "fpn_conv3x3_bf16x3: bad shape N=%d H=%d W=%d", N, H, W);
    MVS_REQUIRE(Cin > 0 && Cin % kGemmBK == 0 && Cout > 0 && Cout % kGemmBM == 0, "fpn_conv3x3_bf16x3: Cin=%d must be a multiple of %d and Cout=%d of %d",
                Cin, kGemmBK, Cout, kGemmBM);
    MVS_REQUIRE(Cout / kGemmBM <= 65535 && Cin <= INT32_MAX / 9, "fpn_conv3x3_bf16x3: too many channels");
    const long long tiles_x = (W + kFcTW - 1) / kFcTW, tiles_y = (H + kFcTH - 1) / kFcTH;
    MVS_REQUIRE((long long)H * W < INT32_MAX && tiles_x * tiles_y < INT32_MAX, "fpn_conv3x3_bf16x3: map %d x %d too large", H, W);
    MVS_REQUIRE(((uintptr_t)wsplit & 15u) == 0 && ((uintptr_t)x & 3u) == 0 && ((uintptr_t)out & 3u) == 0 && ((uintptr_t)bias & 3u) == 0 &&
                    ((uintptr_t)packed & 15u) == 0,
                "fpn_conv3x3_bf16x3: wsplit and packed must be 16-byte, the tensors 4-byte aligned");
    dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(Cout / kGemmBM), (unsigned)N);
    hipLaunchKernelGGL(fpn_conv3x3_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, x, static_cast<const uint4*>(wsplit), bias, out, packed,
                       Cout, Cin, H, W, (int)tiles_x);
    MVS_LAUNCH_CHECK("fpn_conv3x3_bf16x3");
    return MVSDET_OK;
}
